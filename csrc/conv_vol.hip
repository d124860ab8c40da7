// Volume-halo 3x3x3 stride-1 pad-1 convolution in bf16 (r3d_18's block convs)
// on CDNA4: the 3-D sibling of conv_halo.hip.
//
// Why: the generic implicit-GEMM kernel (conv_igemm.hip) gathers every input
// pixel once per tap through LDS-DMA, 27x for a 3x3x3 conv, and that DMA path
// bounds it. Here a block owns a BOX of one clip -- TF = 2 output frames x R
// output rows x the full width W -- times a tile of 128 output channels and,
// per 64-channel input chunk, DMAs the (TF+2) x (R+2) x (W+2) input PATCH the
// box touches exactly once. bf16 needs no hi / lo split, so the patch goes
// from HBM to LDS as it is. The 27 taps are 27 K-steps that read B fragments
// from the patch at entry offset (dt * (R+2) + dh) * (W+2) + dw; only the
// 128 x 64 weight slice of a tap and chunk streams (double-buffered LDS-DMA).
//
// Borders. The spatial border reads zeros through out-of-range buffer
// offsets. Clips are adjacent in memory, so frame -1 of clip n is the last
// frame of clip n-1 (and frame T the first of clip n+1): patch rows of frames
// outside [0, T) get the invalid offset too, per row, which also covers the
// box frame past T when T is odd. A wave skips the taps whose input frame
// lies outside the clip for all of its pixels (wave-uniform branch, barriers
// outside it): at T = 2 that is a third of the MFMAs.
//
// Weights: the layer's existing wmat, k = ((dt*3 + dh)*3 + dw) * Cin_p + c.
// With Cin_p % 64 == 0 a (tap, chunk) slice is 64 contiguous k of every row,
// so no repacked copy is needed.
//
// Geometry: wave w computes pixels [32w, 32w+32) of the box (two 16-pixel
// MFMA sub-tiles; box pixel i = (frame, row, column) raster, so a wave's
// output rows are contiguous in NDHWC) x all 128 channels (8 sub-tiles) with
// v_mfma_f32_16x16x32_bf16, A = weights, B = patch rows: 10 fragment reads
// per 16 MFMAs. LDS rows are 128 B (64 bf16 channels) with the chunk XOR
// swizzle (chunk ^ (row & 7)) applied on the DMA source side; the epilogue is
// conv_epilogue.h (bias folded into the accumulator, paired 16-byte stores).
//
// Variants (kVol): 0 = 7 waves, 224-pixel boxes, up to 928 patch entries
// (56 x 56 in boxes of 2 rows: 4 x 4 x 58 = 119 KB; 28 x 28 in boxes of 4:
// 720 entries; 14 x 14 in boxes of 7: 576), one block per CU; 1 = 4 waves,
// 128-pixel boxes, up to 384 entries (7 x 7 frames whole: 4 x 9 x 9 = 324
// entries, 73.5 KB with the weight stages), two blocks per CU; 2 = variant 0
// with a 64-channel tile (6 fragment reads per 8 MFMAs) for layer1's 64
// output channels, of which a 128-channel tile wastes half the MFMAs.
#include <hip/hip_runtime.h>
#include "lds_attr.h"
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "conv_epilogue.h"

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define VOL_INVALID 0xFFFFFFF0u
#define VOL_TF 2
#define VOL_LDS_LIMIT (160 * 1024)

// Mirrored by rnb_amd/ops/native.py:VolParams.
struct VolParams {
  const uint16_t* x;   // NDHWC input, Cin channels (multiple of 64)
  const uint16_t* w;   // [w_rows][K_pad], k = tap * Cin + c, tap = (dt*3 + dh)*3 + dw
  const float* bias;
  const uint16_t* res;
  uint16_t* y;
  int N, T, H, W, Cin;
  int Cout_p, y_stride, res_stride;
  int K_pad, M, relu, w_rows;
  int n_ctiles;
  int R;               // output rows per box
  int bands;           // ceil(H / R) boxes per frame pair
  int tpairs;          // ceil(T / 2)
  int np;              // patch entries = 4 * (R + 2) * (W + 2)
  uint32_t x_bytes;
};

// One block = one box (clip n, frames t0, t0+1, rows [h0, h0+R)) x TC * 16
// output channels; blockDim = 64 * NW waves, wave w owns box pixels
// [32w, 32w + 32). LDS = one patch + 2 weight stages. PI = patch DMA
// instructions per wave (NW * PI * 8 >= the variant's most patch entries).
template <int TC, int HP, int PI, int NW, int MINB>
__global__ __launch_bounds__(64 * NW, MINB)
void conv_vol_kernel(const VolParams p) {
  constexpr int C_TILE = TC * 16;
  constexpr int W_INSTR_TOTAL = C_TILE / 8;            // weight DMA instructions / step
  constexpr int WBUF = C_TILE * 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // consecutive work-groups of one XCD share a patch (channel tiles fastest)
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int ctile = wgid % p.n_ctiles;
  int box = wgid / p.n_ctiles;
  const int band = box % p.bands;
  box /= p.bands;
  const int tp = box % p.tpairs;
  const int n = box / p.tpairs;
  const int c0 = ctile * C_TILE;
  const int t0 = tp * VOL_TF;
  const int h0 = band * p.R;
  const int nrows = min(p.R, p.H - h0);
  const int fpx = nrows * p.W;                         // output pixels per box frame
  const int npx = min(VOL_TF, p.T - t0) * fpx;         // valid output pixels
  const int W2 = p.W + 2, R2 = p.R + 2;
  const int RW2 = R2 * W2;

  const int lrow = lane >> 3;
  const int kc = (lane & 7) ^ lrow;
  const int n_instr = (p.np + 7) >> 3;
  // patch entry q <-> input (t0 - 1 + q / RW2, h0 - 1 + (q % RW2) / W2,
  // q % W2 - 1) of clip n; anything outside the clip's T x H x W is invalid
  uint32_t poff[PI];
#pragma unroll
  for (int i = 0; i < PI; ++i) {
    const int instr = wave + NW * i;
    const int q = instr * 8 + lrow;
    uint32_t off = VOL_INVALID;
    if (instr < n_instr && q < p.np) {
      const int jt = q / RW2;
      const int r = q - jt * RW2;
      const int j = r / W2;
      const int col = r - j * W2;
      const int t = t0 - 1 + jt, h = h0 - 1 + j, wc = col - 1;
      if ((unsigned)t < (unsigned)p.T && (unsigned)h < (unsigned)p.H &&
          (unsigned)wc < (unsigned)p.W)
        off = (uint32_t)((((((n * p.T + t) * p.H + h) * p.W + wc) * p.Cin) + kc * 8) * 2);
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
    const int i = wave * 16 * HP + a * 16 + frow;      // pixel within the box
    ok[a] = i < npx;
    const int ic = min(i, max(npx - 1, 0));
    const int ft = ic / fpx;
    const int r = ic - ft * fpx;
    const int hh = r / p.W;
    const int ww = r - hh * p.W;
    base[a] = (ft * R2 + hh) * W2 + ww;
    mrow[a] = ((long long)(n * p.T + t0 + ft) * p.H + (h0 + hh)) * p.W + ww;
  }
  // frames of this wave's valid pixels: ft in [ftmin, ftmax] (idle wave: none)
  const int i0 = wave * 16 * HP;
  const bool busy = i0 < npx;
  const int ftmin = busy ? i0 / fpx : 0;
  const int ftmax = busy ? min(i0 + 16 * HP - 1, npx - 1) / fpx : -1;

  const __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.x, (short)0, p.x_bytes, 0x00020000);
  const uint32_t w_bytes = (uint32_t)p.w_rows * (uint32_t)p.K_pad * 2u;
  const __amdgpu_buffer_rsrc_t wr =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.w, (short)0, w_bytes, 0x00020000);
  const uint32_t wrow_off = ((uint32_t)c0 * (uint32_t)p.K_pad + (uint32_t)kc * 8u) * 2u;

  char* pbuf = smem;
  char* wbase = smem + n_instr * 1024;

  auto issue_patch = [&](int chunk) {
    const uint32_t coff = (uint32_t)chunk * 128u;
#pragma unroll
    for (int i = 0; i < PI; ++i) {
      const int instr = wave + NW * i;
      if (instr < n_instr) {
        const uint32_t off = poff[i] == VOL_INVALID ? VOL_INVALID : poff[i] + coff;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            xr, (__attribute__((address_space(3))) void*)(pbuf + instr * 1024), 16, off, 0, 0,
            0);
      }
    }
  };
  auto issue_w = [&](int chunk, int tap, int buf) {
    const uint32_t kofs = (uint32_t)(tap * p.Cin + chunk * 64);
    for (int instr = wave; instr < W_INSTR_TOTAL; instr += NW) {
      const uint32_t off =
          wrow_off + ((uint32_t)(instr * 8 + lrow) * (uint32_t)p.K_pad + kofs) * 2u;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          wr, (__attribute__((address_space(3))) void*)(wbase + buf * WBUF + instr * 1024), 16,
          off, 0, 0, 0);
    }
  };

  f32x4 acc[HP][TC];                               // starts at the (folded) bias
#pragma unroll
  for (int b = 0; b < TC; ++b) {
    const f32x4 b4 = ep_bias4(p.bias, (c0 >> 4) + b, fq);
#pragma unroll
    for (int a = 0; a < HP; ++a) acc[a][b] = b4;
  }

  const int nchunks = p.Cin >> 6;
  const int nsteps = nchunks * 27;
  issue_w(0, 0, 0);
  int s = 0;
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    // the previous chunk's last step ended with a barrier: the patch is free
    issue_patch(chunk);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int dt = 0; dt < 3; ++dt) {
      // does any pixel of the wave read a frame of the clip through this dt?
      const bool live = busy && t0 + ftmax + dt - 1 >= 0 && t0 + ftmin + dt - 1 < p.T;
      for (int dhw = 0; dhw < 9; ++dhw, ++s) {
        if (s + 1 < nsteps) {
          const int tap1 = dt * 9 + dhw + 1;
          issue_w(tap1 == 27 ? chunk + 1 : chunk, tap1 == 27 ? 0 : tap1, (s + 1) & 1);
        }
        if (live) {
          const char* wb = wbase + (s & 1) * WBUF;
          const int dh = dhw / 3, dw = dhw - dh * 3;
          const int shift = (dt * R2 + dh) * W2 + dw;
#pragma unroll
          for (int kk = 0; kk < 2; ++kk) {
            const int ch = kk * 4 + fq;
            bf16x8 af[HP], wf[TC];
#pragma unroll
            for (int tc = 0; tc < TC; ++tc) {
              const int row = tc * 16 + frow;
              wf[tc] = *(const bf16x8*)(wb + row * 128 + ((ch ^ (row & 7)) << 4));
            }
#pragma unroll
            for (int a = 0; a < HP; ++a) {
              const int row = base[a] + shift;
              af[a] = *(const bf16x8*)(pbuf + row * 128 + ((ch ^ (row & 7)) << 4));
            }
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
  for (int a = 0; a < HP; ++a) ep_row<TC>(e, ok[a], mrow[a], c0 >> 4, fq, acc[a]);
}

// Variants: waves, box pixels (32 per wave), most patch entries, patch DMA
// instructions per wave (waves * pi * 8 >= entries), channel tile, kernel.
struct VolVariant {
  int waves, max_px, max_np, c_tile;
  void (*kernel)(const VolParams);
};
static const VolVariant kVol[] = {
    {7, 224, 928, 128, conv_vol_kernel<8, 2, 17, 7, 1>},
    {4, 128, 384, 128, conv_vol_kernel<8, 2, 12, 4, 2>},
    {7, 224, 928, 64, conv_vol_kernel<4, 2, 17, 7, 1>},
};
static const int kVolCount = (int)(sizeof(kVol) / sizeof(kVol[0]));

extern "C" {

int rnb_vol_params_size() { return (int)sizeof(VolParams); }
int rnb_vol_num_variants() { return kVolCount; }

// The box rule (that of rnb_conv_h3v_box): output rows of variant v's box on
// T x H x W clips, 0 = the variant cannot run them. The most rows whose
// pixels fit the waves and whose patch fits the variant's LDS, then evened
// out over the frame's boxes (14 rows at up to 8 per box: 7 + 7, not 8 + 6).
int rnb_vol_box(int v, int T, int H, int W) {
  if (v < 0 || v >= kVolCount) return 0;
  if (T < 2 || H < 1 || W < 1) return 0;
  int R = kVol[v].max_px / (VOL_TF * W);
  if (R > H) R = H;
  while (R >= 1 && (VOL_TF + 2) * (R + 2) * (W + 2) > kVol[v].max_np) --R;
  if (R < 1) return 0;
  const int nb = (H + R - 1) / R;
  return (H + nb - 1) / nb;
}

// LDS bytes a launch of variant v on this shape requests (-1: not supported).
int rnb_vol_lds_bytes(int v, int T, int H, int W, int Cin) {
  const int R = rnb_vol_box(v, T, H, W);
  if (R == 0 || Cin < 64 || Cin % 64 != 0) return -1;
  const int np = (VOL_TF + 2) * (R + 2) * (W + 2);
  return ((np + 7) >> 3) * 1024 + 2 * kVol[v].c_tile * 128;
}

// blocks per CU of the variant's kernel with `lds` dynamic bytes; < 0: a HIP error
int rnb_vol_occupancy(int v, int lds) {
  if (v < 0 || v >= kVolCount) return -1;
  rnb_ensure_max_lds((const void*)kVol[v].kernel);
  int nb = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &nb, (const void*)kVol[v].kernel, 64 * kVol[v].waves, (size_t)lds);
  return e == hipSuccess ? nb : -(int)e;
}

int rnb_vol_launch(const VolParams* pp, int v, hipStream_t stream) {
  if (v < 0 || v >= kVolCount) return -10;
  VolParams p = *pp;
  const VolVariant& vv = kVol[v];
  if (p.N < 0 || p.T < 2 || p.H < 1 || p.W < 1) return -1;
  if (p.Cin < 64 || p.Cin % 64 != 0 || p.K_pad != 27 * p.Cin || p.Cout_p < 4 ||
      p.Cout_p % 4 != 0)
    return -2;
  if (p.M <= 0) return 0;
  if ((long long)p.M != (long long)p.N * p.T * p.H * p.W) return -3;
  if ((long long)p.M * p.Cin * 2 > 0x7FFFFF00LL) return -5;
  p.R = rnb_vol_box(v, p.T, p.H, p.W);
  if (p.R == 0) return -4;
  p.bands = (p.H + p.R - 1) / p.R;
  p.tpairs = (p.T + VOL_TF - 1) / VOL_TF;
  p.np = (VOL_TF + 2) * (p.R + 2) * (p.W + 2);
  if (p.np > vv.max_np || VOL_TF * p.R * p.W > vv.max_px) return -4;
  const int lds = rnb_vol_lds_bytes(v, p.T, p.H, p.W, p.Cin);
  if (lds < 0 || lds > VOL_LDS_LIMIT) return -6;
  p.x_bytes = (uint32_t)((long long)p.M * p.Cin * 2);
  p.n_ctiles = (p.Cout_p + vv.c_tile - 1) / vv.c_tile;
  if (p.n_ctiles * vv.c_tile > p.w_rows) return -8;
  if ((long long)p.w_rows * p.K_pad * 2 > 0xFFFFFF00LL) return -8;
  if (p.y_stride < p.Cout_p || (p.res && p.res_stride < p.Cout_p)) return -9;
  if ((long long)p.M * p.y_stride * 2 > 0xFFFFFF00LL ||
      (long long)p.M * (p.res ? p.res_stride : 0) * 2 > 0xFFFFFF00LL) return -11;
  const long long blocks = (long long)p.N * p.tpairs * p.bands * p.n_ctiles;
  if (blocks > 0x7FFFFFFFLL) return -7;
  rnb_ensure_max_lds((const void*)vv.kernel);
  hipLaunchKernelGGL(vv.kernel, dim3((unsigned)blocks), dim3(64 * vv.waves), lds, stream, p);
  return (int)hipGetLastError();
}

}  // extern "C"
