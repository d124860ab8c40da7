// Patch-staged 3x7x7 stride-(1,2,2) pad-(1,3,3) convolution in bf16 over up to
// 4 input channels (the stem of torchvision's r3d_18 and mc3_18) on CDNA4.
//
// Why: with 3 channels stored as 8 the generic implicit-GEMM kernel
// (conv_igemm.hip) gathers 147 16-byte chunks per output pixel, 3/8 of each
// data, and runs K = 1176 for 441 useful entries. Here a block owns a BOX of
// one clip -- TF = 2 output frames x R output rows x the full output width Wo
// -- times all Cout_p <= 64 output channels, and stages the (TF+2) x (2R+5) x
// (W+6) input PATCH the box touches once, keeping only channels 0..3 of every
// pixel. The patch is PAIR-PACKED: its rows are the padded pixels at 8 bytes
// each, so the 16-byte LDS entry q of a row holds padded columns 2q and 2q+1
// x 4 channels, and because the conv steps 2 in x, output pixel wo reads
// entries wo .. wo+3 of a row: always 16-byte aligned. This is StemConv's
// packing (ops/conv.py) done in LDS instead of by a pass over HBM.
//
// K order. One MFMA K-step of 32 is one (dt, dy) pair: k = 4 * dx + c for dx
// in 0..7, c in 0..3, and lane group g = lane >> 4 reads entry wo + g of patch
// row 2 * ho + dy of patch frame to + dt. 21 K-steps, K = 672 for 441 useful;
// dx = 7 and the channels past cin carry zero weights. The padding is real
// zeros in LDS: patch loads go through a buffer resource and every pixel
// outside the clip's T x H x W (spatial border, frames -1 and T -- clips are
// adjacent in memory -- and the box frame past an odd T) gets an out-of-range
// offset, which reads 0.
//
// Weights: a repacked copy [Cout_p rows in pair_permutation order][21][32]
// (ConvLayer.stem3d_weight), copied once per block into LDS as [21][Cout_p]
// [32] so that a wave's A-fragment read of a K-step is 1 KB contiguous, and
// resident there for the life of the block. The grid is persistent: block b
// takes boxes b, b + grid, ... (static stride); boxes are numbered (clip,
// frame pair, row band) with the band fastest, so the boxes that run at the
// same time are neighbours and their halos (2x in frames, (2R+5) / 2R in
// rows) come from L2.
//
// Pipeline: one patch buffer, prefetched through registers. While a box's
// MFMAs run, the 8-byte global loads of the block's next box are in flight
// into S3_PL register pairs per lane; they are written to LDS (ds_write_b64)
// after the barrier that ends the box. At 112 x 112 (R = 4): 86 016 B of
// weights + 49 088 B of patch, one block of 8 waves per CU.
//
// Geometry: the box's pixels (frame, row, column raster) form 16-pixel MFMA
// tiles; wave w owns tiles w, w + 8, w + 16, w + 24 (at Wo = 56 the 28 tiles
// of a box fall 7 to each SIMD) x all channel sub-tiles, with
// v_mfma_f32_16x16x32_bf16, A = weights, B = patch: 4 + 4 fragment reads per
// 16 MFMAs. The epilogue is conv_epilogue.h.
#include <hip/hip_runtime.h>
#include "lds_attr.h"
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "conv_epilogue.h"

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define S3_INVALID 0xFFFFFFF0u
#define S3_TF 2            // output frames per box
#define S3_NW 8            // waves per block
#define S3_HP 4            // 16-pixel tiles per wave
#define S3_PL 14           // patch loads (8 bytes) per lane and box
#define S3_STEPS 21        // (dt, dy) pairs
#define S3_LDS_LIMIT (160 * 1024)

// Mirrored by rnb_amd/ops/native.py:Stem3dParams.
struct Stem3dParams {
  const uint16_t* x;   // NDHWC input, 8 channels of which 0..3 are read
  const uint16_t* w;   // [Cout_p][21][32], k = 4 * dx + c within a (dt, dy) step
  const float* bias;
  const uint16_t* res;
  uint16_t* y;
  int N, T, H, W;
  int Ho, Wo;
  int Cout_p, y_stride, res_stride;
  int M, relu;
  int grid;            // blocks of the persistent grid (clamped to the boxes)
  int R;               // output rows per box
  int bands;           // ceil(Ho / R)
  int tboxes;          // ceil(T / 2)
  int nboxes;          // N * tboxes * bands
  int Q;               // 16-byte entries per patch row = Wo + 3
  int PR;              // patch rows per frame = 2R + 5
  int CW;              // 64-lane column chunks per patch row = ceil(2Q / 64)
  int units;           // (row, column chunk) load units = 4 * PR * CW
  uint32_t x_bytes;
};

template <int TC>
__global__ __launch_bounds__(64 * S3_NW, 1)
void conv_stem3d_kernel(const Stem3dParams p) {
  constexpr int CP = TC * 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* wl = smem;                                   // [21][CP][32] bf16
  char* pbuf = smem + CP * S3_STEPS * 64;            // [4][PR][Q] 16-byte entries

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int frow = lane & 15;
  const int g = lane >> 4;

  // weights: global [row][step][g] 16-byte chunks -> LDS [step][row][g]
  for (int c = tid; c < CP * S3_STEPS * 4; c += 64 * S3_NW) {
    const int row = c / (S3_STEPS * 4);
    const int rem = c - row * (S3_STEPS * 4);
    *(bf16x8*)(wl + ((((rem >> 2) * CP + row) << 6) | ((rem & 3) << 4))) =
        *(const bf16x8*)(p.w + (size_t)c * 8);
  }

  // Patch load unit u = (patch row r, column chunk cc); wave w takes units
  // w, w + 8, ...; the lane's padded column is pc = 64 cc + lane, input
  // column pc - 3. Box-independent parts: the LDS byte offset (-1: no such
  // unit / column), the byte offset inside an input row (-1: border), the
  // patch frame and the row within it.
  int lofs[S3_PL], xofs[S3_PL], pjt[S3_PL], pj[S3_PL];
#pragma unroll
  for (int i = 0; i < S3_PL; ++i) {
    const int u = wave + S3_NW * i;
    const int r = u / p.CW;
    const int pc = (u - r * p.CW) * 64 + lane;
    const bool live = u < p.units && pc < 2 * p.Q;
    lofs[i] = live ? (r * p.Q * 2 + pc) * 8 : -1;
    xofs[i] = (live && (unsigned)(pc - 3) < (unsigned)p.W) ? (pc - 3) * 16 : -1;
    pjt[i] = r / p.PR;
    pj[i] = r - pjt[i] * p.PR;
  }

  const __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.x, (short)0, p.x_bytes, 0x00020000);
  const EpCtx e = ep_make(p.y, p.y_stride, p.res, p.res_stride, p.M, p.Cout_p, p.relu != 0);

  ep_i32x2 pre[S3_PL];
  // the 8-byte loads of box b's patch; pixels outside the clip read 0
  auto issue_patch = [&](int b) {
    const int band = b % p.bands;
    b /= p.bands;
    const int tp = b % p.tboxes;
    const int n = b / p.tboxes;
#pragma unroll
    for (int i = 0; i < S3_PL; ++i) {
      const int t = tp * S3_TF - 1 + pjt[i];
      const int h = 2 * band * p.R - 3 + pj[i];
      uint32_t off = S3_INVALID;
      if (xofs[i] >= 0 && (unsigned)t < (unsigned)p.T && (unsigned)h < (unsigned)p.H)
        off = (uint32_t)(((n * p.T + t) * p.H + h) * p.W) * 16u + (uint32_t)xofs[i];
      pre[i] = __builtin_amdgcn_raw_buffer_load_b64(xr, off, 0, 0);
    }
  };

  const int nboxes = p.nboxes;
  const int stride = gridDim.x;
  int box = blockIdx.x;
  if (box < nboxes) issue_patch(box);
  __syncthreads();                                   // weights are in LDS

  for (; box < nboxes; box += stride) {
#pragma unroll
    for (int i = 0; i < S3_PL; ++i)
      if (lofs[i] >= 0) *(ep_i32x2*)(pbuf + lofs[i]) = pre[i];
    __syncthreads();
    if (box + stride < nboxes) issue_patch(box + stride);

    int b = box;
    const int band = b % p.bands;
    b /= p.bands;
    const int tp = b % p.tboxes;
    const int n = b / p.tboxes;
    const int t0 = tp * S3_TF;
    const int h0 = band * p.R;
    const int fpx = min(p.R, p.Ho - h0) * p.Wo;      // output pixels per box frame
    const int npx = min(S3_TF, p.T - t0) * fpx;      // valid output pixels (>= 1)
    // tiles of this wave that hold a valid pixel: a < nact
    const int ntiles = (npx + 15) >> 4;
    const int nact = ntiles > wave ? min(S3_HP, (ntiles - wave + S3_NW - 1) / S3_NW) : 0;

    int base[S3_HP];        // patch byte offset of (dt, dy) = (0, 0), entry wo + g
    long long mrow[S3_HP];  // output row of the lane's pixel
    bool ok[S3_HP];
#pragma unroll
    for (int a = 0; a < S3_HP; ++a) {
      const int i = (wave + S3_NW * a) * 16 + frow;  // pixel within the box
      ok[a] = i < npx;
      const int ic = min(i, npx - 1);
      const int ft = ic / fpx;
      const int r = ic - ft * fpx;
      const int hh = r / p.Wo;
      const int ww = r - hh * p.Wo;
      base[a] = (((ft * p.PR + 2 * hh) * p.Q) + ww + g) << 4;
      mrow[a] = ((long long)(n * p.T + t0 + ft) * p.Ho + (h0 + hh)) * p.Wo + ww;
    }

    f32x4 acc[S3_HP][TC];                            // starts at the (folded) bias
#pragma unroll
    for (int tc = 0; tc < TC; ++tc) {
      const f32x4 b4 = ep_bias4(p.bias, tc, g);
#pragma unroll
      for (int a = 0; a < S3_HP; ++a) acc[a][tc] = b4;
    }

    if (nact > 0) {
      for (int dt = 0; dt < 3; ++dt) {
#pragma unroll
        for (int dy = 0; dy < 7; ++dy) {
          const int s = dt * 7 + dy;
          const int shift = ((dt * p.PR + dy) * p.Q) << 4;
          bf16x8 wf[TC], af[S3_HP];
#pragma unroll
          for (int tc = 0; tc < TC; ++tc)
            wf[tc] = *(const bf16x8*)(wl + (((s * CP + tc * 16 + frow) << 6) | (g << 4)));
#pragma unroll
          for (int a = 0; a < S3_HP; ++a) af[a] = *(const bf16x8*)(pbuf + base[a] + shift);
#pragma unroll
          for (int a = 0; a < S3_HP; ++a) {
            if (a < nact) {
#pragma unroll
              for (int tc = 0; tc < TC; ++tc)
                acc[a][tc] =
                    __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[tc], af[a], acc[a][tc], 0, 0, 0);
            }
          }
        }
      }
    }
    __syncthreads();                                 // the patch is free again
#pragma unroll
    for (int a = 0; a < S3_HP; ++a)
      if (a < nact) ep_row<TC>(e, ok[a], mrow[a], 0, g, acc[a]);
  }
}

typedef void (*Stem3dKernel)(const Stem3dParams);
static const Stem3dKernel kStem3d[4] = {conv_stem3d_kernel<1>, conv_stem3d_kernel<2>,
                                        conv_stem3d_kernel<3>, conv_stem3d_kernel<4>};

static bool s3_cout_ok(int Cout_p) { return Cout_p >= 16 && Cout_p <= 64 && Cout_p % 16 == 0; }

static int s3_lds(int R, int W, int Cout_p) {
  const int Q = (W - 1) / 2 + 1 + 3;
  return Cout_p * S3_STEPS * 64 + (S3_TF + 2) * (2 * R + 5) * Q * 16;
}

extern "C" {

int rnb_stem3d_params_size() { return (int)sizeof(Stem3dParams); }

// Output rows of a box on T x H x W clips (0: the shape cannot run): the most
// rows whose pixels fit the waves' tiles, whose patch fits LDS next to the
// weights and whose load units fit the lanes' S3_PL register pairs.
int rnb_stem3d_box(int T, int H, int W, int Cout_p) {
  if (T < 1 || H < 1 || W < 1 || !s3_cout_ok(Cout_p)) return 0;
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int CW = (2 * (Wo + 3) + 63) / 64;
  int R = (16 * S3_HP * S3_NW) / (S3_TF * Wo);
  if (R > Ho) R = Ho;
  while (R >= 1 && (s3_lds(R, W, Cout_p) > S3_LDS_LIMIT ||
                    (S3_TF + 2) * (2 * R + 5) * CW > S3_NW * S3_PL))
    --R;
  return R < 1 ? 0 : R;
}

// LDS bytes a launch on this shape requests (0: the shape cannot run).
int rnb_stem3d_lds_bytes(int T, int H, int W, int Cout_p) {
  const int R = rnb_stem3d_box(T, H, W, Cout_p);
  return R == 0 ? 0 : s3_lds(R, W, Cout_p);
}

// blocks per CU of the Cout_p kernel with `lds` dynamic bytes; < 0: a HIP error
int rnb_stem3d_occupancy(int Cout_p, int lds) {
  if (!s3_cout_ok(Cout_p)) return -1;
  const void* k = (const void*)kStem3d[Cout_p / 16 - 1];
  rnb_ensure_max_lds(k);
  int nb = 0;
  const hipError_t e =
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k, 64 * S3_NW, (size_t)lds);
  return e == hipSuccess ? nb : -(int)e;
}

// Serves 3x7x7 / (1,2,2) / (1,3,3) convs over 8 stored channels only: an
// output size that is not that geometry's, or a shape without a box, is an
// error code and no launch. p.R .. p.x_bytes are filled in here.
int rnb_stem3d_launch(const Stem3dParams* pp, hipStream_t stream) {
  Stem3dParams p = *pp;
  if (p.N < 0 || p.T < 1 || p.H < 1 || p.W < 1) return -1;
  if (!s3_cout_ok(p.Cout_p)) return -2;
  if (p.Ho != (p.H - 1) / 2 + 1 || p.Wo != (p.W - 1) / 2 + 1) return -3;
  if (p.M <= 0) return 0;
  if ((long long)p.M != (long long)p.N * p.T * p.Ho * p.Wo) return -3;
  if ((long long)p.N * p.T * p.H * p.W * 16 > 0x7FFFFF00LL) return -5;
  p.R = rnb_stem3d_box(p.T, p.H, p.W, p.Cout_p);
  if (p.R == 0) return -4;
  p.bands = (p.Ho + p.R - 1) / p.R;
  p.tboxes = (p.T + S3_TF - 1) / S3_TF;
  p.Q = p.Wo + 3;
  p.PR = 2 * p.R + 5;
  p.CW = (2 * p.Q + 63) / 64;
  p.units = (S3_TF + 2) * p.PR * p.CW;
  if (p.units > S3_NW * S3_PL || S3_TF * p.R * p.Wo > 16 * S3_HP * S3_NW) return -4;
  const int lds = s3_lds(p.R, p.W, p.Cout_p);
  if (lds > S3_LDS_LIMIT) return -6;
  p.x_bytes = (uint32_t)((long long)p.N * p.T * p.H * p.W * 16);
  if (p.y_stride < p.Cout_p || (p.res && p.res_stride < p.Cout_p)) return -9;
  if ((long long)p.M * p.y_stride * 2 > 0xFFFFFF00LL ||
      (long long)p.M * (p.res ? p.res_stride : 0) * 2 > 0xFFFFFF00LL) return -11;
  const long long boxes = (long long)p.N * p.tboxes * p.bands;
  if (boxes > 0x7FFFFFFFLL) return -7;
  p.nboxes = (int)boxes;
  if (p.grid < 1) return -8;
  if (p.grid > p.nboxes) p.grid = p.nboxes;
  const Stem3dKernel k = kStem3d[p.Cout_p / 16 - 1];
  rnb_ensure_max_lds((const void*)k);
  hipLaunchKernelGGL(k, dim3((unsigned)p.grid), dim3(64 * S3_NW), lds, stream, p);
  return (int)hipGetLastError();
}

}  // extern "C"
