// Parity-staged 3x3x3 stride-2 pad-1 convolution in bf16 (the convs that open
// layer2, layer3 and layer4 of r3d_18) on CDNA4: the stride-2 sibling of
// conv_vol.hip.
//
// Why: the generic implicit-GEMM kernel (conv_igemm.hip) gathers 27 16-byte
// chunks per output pixel and 8 channels through LDS-DMA, the path that
// bounds it. At stride 2 an input value feeds 27 / 8 taps on average, so a
// block that stages the input PATCH of its output box once moves about 8
// input pixels per output pixel plus halo instead of 27.
//
// Box and patch. A block owns one clip's box of TFO = 1 output frame x Ro
// output rows x the full output width Wo, times a tile of 128 output
// channels. Per 32-channel input chunk it DMAs the (2 TFO + 1) x (2 Ro + 1)
// patch rows of 2 Wo + 1 padded columns into LDS once, as 64-byte entries (32
// bf16): the 16 pixels x 4 K-quarters of an MFMA B fragment then read 1 KB of
// consecutive LDS and no swizzle is needed. (128-byte entries would admit
// only 56-pixel boxes at Wo = 28: 3 x 5 x 58 entries are 111 KB; 64-byte ones
// admit 1 x 4 x 28 = 112 pixels in 3 x 9 x 58 entries = 100 KB.)
//
// Column parity. A patch row is stored de-interleaved: an even plane and an
// odd plane of Wo + 1 entries each (row stride RS = 2 (Wo + 1)). Output pixel
// wo under tap dw reads padded column 2 wo + dw = plane dw & 1, entry
// wo + (dw >> 1), so every tap is a unit-stride read across the 16 pixels of
// a fragment, as at stride 1. The LDS-DMA destination is lane-consecutive, so
// the permutation is applied on the source-offset side. dt and dh are whole
// patch-row offsets and need no de-interleave.
//
// Borders. Patch entries outside the clip's T x H x W get the invalid buffer
// offset and read zeros: the left, top and first-frame padding, the right and
// bottom padding of odd sizes, rows of a short last band, and the frames of
// neighbouring clips (clips are adjacent in memory). A wave skips the dt
// planes none of its pixels has a frame for (wave-uniform branch, barriers
// outside it): dt = 0 of the first output frame, dt = 2 of the last when T is
// odd, so two of three at T = 1.
//
// Weights: the layer's existing wmat, k = ((dt*3 + dh)*3 + dw) * Cin_p + c; a
// (tap, 32-channel chunk) slice is 64 contiguous bytes of every row, so no
// repacked copy is made. They stream by LDS-DMA, double-buffered, in stages
// of one (dt, dh) row of three taps (3 x 128 x 64 B = 24 KB): 9 barriers per
// chunk with 24 MFMAs per wave between them.
//
// Geometry: 8 waves = NPW 4 pixel waves x 2 channel halves. Pixel wave pw
// owns box pixels [16 HP pw, 16 HP (pw + 1)) (box pixel i = (frame, row,
// column) raster), channel half cw the 64 channels [64 cw, 64 cw + 64) of the
// tile: HP x 4 accumulators of v_mfma_f32_16x16x32_bf16, A = weights, B =
// patch entries, 4 + HP fragment reads per 4 HP MFMAs. The epilogue is
// conv_epilogue.h (bias folded into the accumulator, paired 16-byte stores).
//
// One variant (kVol2): HP = 2, 128-pixel boxes (28 x 28 outputs in boxes of 4
// rows: 1566 entries, 149 KB with the weight stages; 14 x 14 in boxes of 7
// rows; 7 x 7 frames whole), one block per CU. A 64-pixel variant (HP = 1)
// was measured and never beat both this one and the generic kernel
// (profiles/r3d_vol2_bf16.txt), so it is not instantiated.
#include <hip/hip_runtime.h>
#include "lds_attr.h"
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "conv_epilogue.h"

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define VOL2_INVALID 0xFFFFFFF0u
#define VOL2_TFO 1                       // output frames per box
#define VOL2_LDS_LIMIT (160 * 1024)
#define VOL2_C_TILE 128
#define VOL2_WBUF (3 * VOL2_C_TILE * 64) // one weight stage: 3 taps x 128 rows x 64 B

// Mirrored by rnb_amd/ops/native.py:Vol2Params (the launcher fills in
// n_ctiles .. x_bytes).
struct Vol2Params {
  const uint16_t* x;   // NDHWC input, Cin channels (multiple of 32)
  const uint16_t* w;   // [w_rows][K_pad], k = tap * Cin + c, tap = (dt*3 + dh)*3 + dw
  const float* bias;
  const uint16_t* res;
  uint16_t* y;
  int N, T, H, W, Cin;
  int To, Ho, Wo;
  int Cout_p, y_stride, res_stride;
  int K_pad, M, relu, w_rows;
  int n_ctiles;
  int Ro;              // output rows per box
  int bands;           // ceil(Ho / Ro) boxes per output frame group
  int tboxes;          // ceil(To / VOL2_TFO)
  int np;              // patch entries = (2 TFO + 1) * (2 Ro + 1) * 2 * (Wo + 1)
  uint32_t x_bytes;
};

// One block = one box (clip n, output frames [to0, to0 + TFO), output rows
// [ho0, ho0 + Ro)) x 128 output channels; 512 threads. LDS = one patch + 2
// weight stages. PI = patch DMA instructions per wave (8 * PI * 16 >= the
// variant's most patch entries).
template <int HP, int PI>
__global__ __launch_bounds__(512, 1)
void conv_vol2_kernel(const Vol2Params p) {
  constexpr int NW = 8, TC = 4;
  constexpr int W_INSTR = 3 * VOL2_C_TILE / 16;        // weight DMA instructions / stage
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pw = wave & 3, cw = wave >> 2;

  // consecutive work-groups of one XCD share a patch (channel tiles fastest)
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int ctile = wgid % p.n_ctiles;
  int box = wgid / p.n_ctiles;
  const int band = box % p.bands;
  box /= p.bands;
  const int tb = box % p.tboxes;
  const int n = box / p.tboxes;
  const int c0 = ctile * VOL2_C_TILE;
  const int to0 = tb * VOL2_TFO;
  const int ho0 = band * p.Ro;
  const int nrows = min(p.Ro, p.Ho - ho0);
  const int fpx = nrows * p.Wo;                        // output pixels per box frame
  const int npx = min(VOL2_TFO, p.To - to0) * fpx;     // valid output pixels
  const int PL = p.Wo + 1;                             // entries per parity plane
  const int RS = 2 * PL;                               // entries per patch row
  const int PR = 2 * p.Ro + 1;                         // patch rows per frame
  const int FS = PR * RS;                              // entries per patch frame

  const int lent = lane >> 2;                          // entry / weight row within a DMA
  const uint32_t lq = (uint32_t)(lane & 3) * 16u;      // K-quarter byte offset
  const int n_instr = (p.np + 15) >> 4;
  // patch entry q = ((jt * PR + j) * 2 + plane) * PL + e <-> input frame
  // 2 to0 - 1 + jt, row 2 ho0 - 1 + j, column 2 e + plane - 1 of clip n;
  // anything outside the clip's T x H x W is invalid
  uint32_t poff[PI];
#pragma unroll
  for (int i = 0; i < PI; ++i) {
    const int instr = wave + NW * i;
    const int q = instr * 16 + lent;
    uint32_t off = VOL2_INVALID;
    if (instr < n_instr && q < p.np) {
      const int jt = q / FS;
      const int r = q - jt * FS;
      const int j = r / RS;
      const int r2 = r - j * RS;
      const int plane = r2 >= PL ? 1 : 0;
      const int e = r2 - plane * PL;
      const int t = 2 * to0 - 1 + jt, h = 2 * ho0 - 1 + j, wc = 2 * e + plane - 1;
      if ((unsigned)t < (unsigned)p.T && (unsigned)h < (unsigned)p.H &&
          (unsigned)wc < (unsigned)p.W)
        off = (uint32_t)(((n * p.T + t) * p.H + h) * p.W + wc) * (uint32_t)(p.Cin * 2) + lq;
    }
    poff[i] = off;
  }

  const int frow = lane & 15;
  const int fq = lane >> 4;
  int base[HP];           // patch entry of tap (0, 0, 0) of the lane's pixel
  long long mrow[HP];     // output row of the lane's pixel
  bool ok[HP];
#pragma unroll
  for (int a = 0; a < HP; ++a) {
    const int i = pw * 16 * HP + a * 16 + frow;        // pixel within the box
    ok[a] = i < npx;
    const int ic = min(i, max(npx - 1, 0));
    const int ft = ic / fpx;
    const int r = ic - ft * fpx;
    const int hh = r / p.Wo;
    const int ww = r - hh * p.Wo;
    base[a] = 2 * ft * FS + 2 * hh * RS + ww;
    mrow[a] = ((long long)(n * p.To + to0 + ft) * p.Ho + (ho0 + hh)) * p.Wo + ww;
  }
  // output frames of this wave's valid pixels: ft in [ftmin, ftmax] (idle wave: none)
  const int i0 = pw * 16 * HP;
  const bool busy = i0 < npx;
  const int ftmin = busy ? i0 / fpx : 0;
  const int ftmax = busy ? min(i0 + 16 * HP - 1, npx - 1) / fpx : -1;

  const __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.x, (short)0, p.x_bytes, 0x00020000);
  const uint32_t w_bytes = (uint32_t)p.w_rows * (uint32_t)p.K_pad * 2u;
  const __amdgpu_buffer_rsrc_t wr =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.w, (short)0, w_bytes, 0x00020000);
  const uint32_t wrow_off = (uint32_t)(c0 + lent) * (uint32_t)p.K_pad * 2u + lq;

  char* pbuf = smem;
  char* wbase = smem + n_instr * 1024;

  auto issue_patch = [&](int chunk) {
    const uint32_t coff = (uint32_t)chunk * 64u;
#pragma unroll
    for (int i = 0; i < PI; ++i) {
      const int instr = wave + NW * i;
      if (instr < n_instr) {
        const uint32_t off = poff[i] == VOL2_INVALID ? VOL2_INVALID : poff[i] + coff;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            xr, (__attribute__((address_space(3))) void*)(pbuf + instr * 1024), 16, off, 0, 0,
            0);
      }
    }
  };
  // stage = the three dw taps of (chunk, dt * 3 + dh): instruction j covers
  // rows 16 (j % 8) .. + 15 of tap dw = j / 8
  auto issue_w = [&](int chunk, int dtdh, int buf) {
    for (int j = wave; j < W_INSTR; j += NW) {
      const int dw = j >> 3, rg = j & 7;
      const uint32_t kofs = (uint32_t)((dtdh * 3 + dw) * p.Cin + chunk * 32);
      const uint32_t off = wrow_off + ((uint32_t)(rg * 16) * (uint32_t)p.K_pad + kofs) * 2u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          wr, (__attribute__((address_space(3))) void*)(wbase + buf * VOL2_WBUF + j * 1024), 16,
          off, 0, 0, 0);
    }
  };

  const int gt0 = (c0 >> 4) + cw * TC;             // first 16-row weight tile of the wave
  f32x4 acc[HP][TC];                               // starts at the (folded) bias
#pragma unroll
  for (int b = 0; b < TC; ++b) {
    const f32x4 b4 = ep_bias4(p.bias, gt0 + b, fq);
#pragma unroll
    for (int a = 0; a < HP; ++a) acc[a][b] = b4;
  }

  const int nchunks = p.Cin >> 5;
  const int nstages = nchunks * 9;
  issue_w(0, 0, 0);
  int s = 0;
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    // the previous chunk's last stage ended with a barrier: the patch is free
    issue_patch(chunk);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int dt = 0; dt < 3; ++dt) {
      // does any pixel of the wave read a frame of the clip through this dt?
      const bool live =
          busy && 2 * (to0 + ftmax) + dt - 1 >= 0 && 2 * (to0 + ftmin) + dt - 1 < p.T;
      for (int dh = 0; dh < 3; ++dh, ++s) {
        if (s + 1 < nstages) {
          const int d1 = dt * 3 + dh + 1;
          issue_w(d1 == 9 ? chunk + 1 : chunk, d1 == 9 ? 0 : d1, (s + 1) & 1);
        }
        if (live) {
          const char* wb = wbase + (s & 1) * VOL2_WBUF + (cw * TC * 16 + frow) * 64 + fq * 16;
          const char* pb = pbuf + (dt * FS + dh * RS) * 64 + fq * 16;
#pragma unroll
          for (int dw = 0; dw < 3; ++dw) {
            const int shift = (dw & 1) * PL + (dw >> 1);
            bf16x8 af[HP], wf[TC];
#pragma unroll
            for (int tc = 0; tc < TC; ++tc)
              wf[tc] = *(const bf16x8*)(wb + (dw * VOL2_C_TILE + tc * 16) * 64);
#pragma unroll
            for (int a = 0; a < HP; ++a)
              af[a] = *(const bf16x8*)(pb + (base[a] + shift) * 64);
#pragma unroll
            for (int a = 0; a < HP; ++a)
#pragma unroll
              for (int tc = 0; tc < TC; ++tc)
                acc[a][tc] =
                    __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[tc], af[a], acc[a][tc], 0, 0, 0);
          }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
      }
    }
  }

  const EpCtx e = ep_make(p.y, p.y_stride, p.res, p.res_stride, p.M, p.Cout_p, p.relu != 0);
#pragma unroll
  for (int a = 0; a < HP; ++a) ep_row<TC>(e, ok[a], mrow[a], gt0, fq, acc[a]);
}

// Variants: box pixels (64 HP over the 4 pixel waves), most patch entries
// (8 waves * pi * 16 >= entries; the LDS limit less the weight stages holds
// 1792), kernel.
struct Vol2Variant {
  int max_px, max_np;
  void (*kernel)(const Vol2Params);
};
static const Vol2Variant kVol2[] = {
    {128, 1792, conv_vol2_kernel<2, 14>},
};
static const int kVol2Count = (int)(sizeof(kVol2) / sizeof(kVol2[0]));

static inline int vol2_np(int Ro, int Wo) {
  return (2 * VOL2_TFO + 1) * (2 * Ro + 1) * 2 * (Wo + 1);
}

extern "C" {

int rnb_vol2_params_size() { return (int)sizeof(Vol2Params); }
int rnb_vol2_num_variants() { return kVol2Count; }

// The box rule (that of rnb_vol_box, on the output): output rows of variant
// v's box on T x H x W input clips, 0 = the variant cannot run them. The most
// rows whose pixels fit the waves and whose patch fits the variant's LDS,
// then evened out over the output frame's boxes (14 rows at up to 9 per box:
// 7 + 7, not 9 + 5).
int rnb_vol2_box(int v, int T, int H, int W) {
  if (v < 0 || v >= kVol2Count) return 0;
  if (T < 1 || H < 1 || W < 1) return 0;
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  int R = kVol2[v].max_px / (VOL2_TFO * Wo);
  if (R > Ho) R = Ho;
  while (R >= 1 && vol2_np(R, Wo) > kVol2[v].max_np) --R;
  if (R < 1) return 0;
  const int nb = (Ho + R - 1) / R;
  return (Ho + nb - 1) / nb;
}

// LDS bytes a launch of variant v on this shape requests (-1: not supported).
int rnb_vol2_lds_bytes(int v, int T, int H, int W, int Cin) {
  const int R = rnb_vol2_box(v, T, H, W);
  if (R == 0 || Cin < 32 || Cin % 32 != 0) return -1;
  const int lds = ((vol2_np(R, (W + 1) / 2) + 15) >> 4) * 1024 + 2 * VOL2_WBUF;
  return lds <= VOL2_LDS_LIMIT ? lds : -1;
}

// blocks per CU of the variant's kernel with `lds` dynamic bytes; < 0: a HIP error
int rnb_vol2_occupancy(int v, int lds) {
  if (v < 0 || v >= kVol2Count) return -1;
  rnb_ensure_max_lds((const void*)kVol2[v].kernel);
  int nb = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &nb, (const void*)kVol2[v].kernel, 512, (size_t)lds);
  return e == hipSuccess ? nb : -(int)e;
}

int rnb_vol2_launch(const Vol2Params* pp, int v, hipStream_t stream) {
  if (v < 0 || v >= kVol2Count) return -10;
  Vol2Params p = *pp;
  const Vol2Variant& vv = kVol2[v];
  if (p.N < 0 || p.T < 1 || p.H < 1 || p.W < 1) return -1;
  if (p.Cin < 32 || p.Cin % 32 != 0 || p.K_pad < 27 * p.Cin || p.K_pad % 8 != 0 ||
      p.Cout_p < 4 || p.Cout_p % 4 != 0)
    return -2;
  if (p.To != (p.T + 1) / 2 || p.Ho != (p.H + 1) / 2 || p.Wo != (p.W + 1) / 2) return -3;
  if (p.M <= 0) return 0;
  if ((long long)p.M != (long long)p.N * p.To * p.Ho * p.Wo) return -3;
  const long long xb = (long long)p.N * p.T * p.H * p.W * p.Cin * 2;
  if (xb > 0x7FFFFF00LL) return -5;
  p.Ro = rnb_vol2_box(v, p.T, p.H, p.W);
  if (p.Ro == 0) return -4;
  p.bands = (p.Ho + p.Ro - 1) / p.Ro;
  p.tboxes = (p.To + VOL2_TFO - 1) / VOL2_TFO;
  p.np = vol2_np(p.Ro, p.Wo);
  if (p.np > vv.max_np || VOL2_TFO * p.Ro * p.Wo > vv.max_px) return -4;
  const int lds = rnb_vol2_lds_bytes(v, p.T, p.H, p.W, p.Cin);
  if (lds < 0 || lds > VOL2_LDS_LIMIT) return -6;
  p.x_bytes = (uint32_t)xb;
  p.n_ctiles = (p.Cout_p + VOL2_C_TILE - 1) / VOL2_C_TILE;
  if (p.n_ctiles * VOL2_C_TILE > p.w_rows) return -8;
  if ((long long)p.w_rows * p.K_pad * 2 > 0xFFFFFF00LL) return -8;
  if (p.y_stride < p.Cout_p || (p.res && p.res_stride < p.Cout_p)) return -9;
  if ((long long)p.M * p.y_stride * 2 > 0xFFFFFF00LL ||
      (long long)p.M * (p.res ? p.res_stride : 0) * 2 > 0xFFFFFF00LL) return -11;
  const long long blocks = (long long)p.N * p.tboxes * p.bands * p.n_ctiles;
  if (blocks > 0x7FFFFFFFLL) return -7;
  rnb_ensure_max_lds((const void*)vv.kernel);
  hipLaunchKernelGGL(vv.kernel, dim3((unsigned)blocks), dim3(512), lds, stream, p);
  return (int)hipGetLastError();
}

}  // extern "C"
