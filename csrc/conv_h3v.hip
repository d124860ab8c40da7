// Volume-band h3 conv ("h3v"): the stride-1 3x3x3 convs (pad 1) of the
// torchvision r3d_18 tree, fp32 products on the fp16 matrix cores as in
// conv_h3.hip (fp16 hi / lo split, three v_mfma_f32_16x16x32_f16 per 32
// channels, h3_common.h).
//
// Work split. A block owns a box of one clip: TF = 2 output frames x R output
// rows x the full width W, times C_TILE output channels. Its 4 waves (one per
// SIMD) form a 2 x 2 grid: wave (wp, wc) holds output frame t0 + wp of the box
// (TP pixel tiles of 16, TP * 16 >= R * W) and channel half wc (TC channel
// tiles), so a tap costs a wave TP activation and TC weight fragment reads
// for 3 TP TC MFMAs, and a wave's rows are one contiguous range of the NDHWC
// output: the shared epilogue (x6d_epilogue) runs per wave on its frame.
//
// Staging. Per 32-channel chunk the (TF + 2) x (R + 2) x (W + 2) input patch
// is loaded once and split once into ready-made MFMA B operands in the
// row-band layout (conv_h3r_kernel): 128 B per entry, [H0 H1] / [L0 L1] slots
// per channel quad, permuted by x6r_swz; entries outside the clip stay zero.
// The 27 taps are 27 GEMM steps on shifted entries, entry offset
// (dt (R + 2) + dh) (W + 2) + dw, with the weights streamed per group of G
// taps by LDS-DMA, double-buffered (weight step s = tap * Cin_p / 32 + chunk:
// the h3 direct kernel's K order). Against the gather-table kernel, which
// loads and splits every input value 27 times, a 56 x 56 box stages 4.1
// entries per output pixel.
//
// Taps whose input frame lies outside the clip (the first frame's dt = 0, the
// last frame's dt = 2, every tap of a box frame past T) multiply zeros: a wave
// skips them (a wave-uniform branch; the barriers stay outside it). At T = 2
// that is a third of the MFMAs.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "x6d_common.h"

#include "h3_common.h"

extern "C" int* rnb_h3_range_flag();

#define H3V_TF 2

template <int TP, int TC, int HALO_PX, int G, int MINB, bool ST>
__global__ __launch_bounds__(256, MINB)
void conv_h3v_kernel(const ConvF32Params p, const X6DStats st) {
  constexpr int NW = 4, WC = 2;
  constexpr int C_TILE = WC * TC * 16;
  constexpr int HALO_BYTES = HALO_PX * 128;
  constexpr int W_BYTES = C_TILE * 128;              // one tap's weights of a chunk
  constexpr int W_TOTAL = C_TILE / 8;                // 1 KB = 8 weight rows per DMA
  constexpr int W_INSTR = W_TOTAL / NW;
  constexpr int NT = 64 * NW;
  constexpr int ITEMS = (HALO_PX * 4 + NT - 1) / NT; // (entry, quad) items per lane
  constexpr int LDS_BYTES = HALO_BYTES + 2 * G * W_BYTES;
  static_assert(W_TOTAL % NW == 0, "weight DMA split");
  __shared__ __attribute__((aligned(16))) char lds[LDS_BYTES];
  char* const wbuf = lds + HALO_BYTES;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wp = wave >> 1, wc = wave & 1;
  const int frow = lane & 15, fq = lane >> 4;
  const int T = p.T, H = p.H, W = p.W, W2 = p.W + 2;
  const int R = p.ngroups, PR = R + 2;               // host: rows per box, bands per frame
  const int nbands = p.n_ptiles, nboxt = (T + H3V_TF - 1) / H3V_TF;

  // XCD-aware bijective block remap (conv_x6_kernel); channel tiles of a box
  // are neighbours, so its patch is read from L2 after the first
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int q8 = nwg >> 3, r8 = nwg & 7, xcd = bid & 7;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
  const int ctile = wgid % p.n_ctiles;
  int rest = wgid / p.n_ctiles;
  const int band = rest % nbands;
  rest /= nbands;
  const int tb = rest % nboxt, n = rest / nboxt;
  const int t0 = tb * H3V_TF, r0 = band * R;
  const int rows = min(R, H - r0);
  const int c0 = ctile * C_TILE;
  const int nck = p.Cin_p / 32;

  const x6d_u32x4 wr = x6d_rsrc(p.w, (uint32_t)(p.K_pad / 32) * (uint32_t)p.w_rows * 128u);
  auto issue_w = [&](int s, int buf) {
    const uint32_t wbase = ((uint32_t)s * (uint32_t)p.w_rows + (uint32_t)c0) * 128u;
#pragma unroll
    for (int j = 0; j < W_INSTR; ++j) {
      const int instr = wave + NW * j;
      x6d_dma16(wr, wbase + (uint32_t)(instr * 1024 + lane * 16),
                wbuf + buf * W_BYTES + instr * 1024);
    }
  };

  // patch staging: item i = 4 e + quad of entry e = (pt PR + ph) W2 + pw, the
  // input at frame t0 - 1 + pt, row r0 - 1 + ph, column pw - 1; the lane's
  // quad is threadIdx.x & 3 for every item
  const __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.x, (short)0, p.x_bytes, 0x00020000);
  const int fpx = PR * W2, npx = (H3V_TF + 2) * fpx;
  const int qd = threadIdx.x & 3;
  uint32_t src[ITEMS];
  int dst[ITEMS];
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const int e = (threadIdx.x + i * NT) >> 2;
    const int pt = e / fpx, re = e - pt * fpx;
    const int ph = re / W2, pw = re - ph * W2;
    const int t = t0 - 1 + pt, y = r0 - 1 + ph, x = pw - 1;
    const bool ok = e < npx && t >= 0 && t < T && y >= 0 && y < H && x >= 0 && x < W;
    src[i] = ok ? (uint32_t)(((((n * T + t) * H + y) * W + x) * p.Cin_p + qd * 4) * 4)
                : X6D_INVALID;
    dst[i] = e < npx ? e * 128 : -1;
  }
  const float in_scale = st.in_scale;
  constexpr int SB = 5;                              // items' loads in flight
  auto stage = [&](int chunk) {
#pragma unroll
    for (int i0 = 0; i0 < ITEMS; i0 += SB) {
      x6f32x4 v0[SB], v1[SB];
#pragma unroll
      for (int k = 0; k < SB; ++k) {
        const int i = min(i0 + k, ITEMS - 1);
        const uint32_t o = src[i] == X6D_INVALID ? X6D_INVALID : src[i] + (uint32_t)(chunk * 128);
        v0[k] = __builtin_amdgcn_raw_buffer_load_b128(xr, o, 0, 0);
        v1[k] = __builtin_amdgcn_raw_buffer_load_b128(xr, o == X6D_INVALID ? o : o + 64u, 0, 0);
      }
#pragma unroll
      for (int k = 0; k < SB; ++k) {
        const int i = i0 + k;
        if (i >= ITEMS || dst[i] < 0) continue;
        const int e = dst[i] >> 7;
        uint32_t h[4], l[4];
        h3_split4(v0[k] * in_scale, h, l);
        h3_split4(v1[k] * in_scale, h + 2, l + 2);
        char* base = lds + dst[i];
        *(wu32x4*)(base + (x6r_swz(2 * qd, e) << 4)) = (wu32x4){h[0], h[1], h[2], h[3]};
        *(wu32x4*)(base + (x6r_swz(2 * qd + 1, e) << 4)) = (wu32x4){l[0], l[1], l[2], l[3]};
      }
    }
  };

  // this lane's output pixel of tile tp -> patch entry at tap (0, 0, 0)
  // (slots past the box read entry 0 and are never stored)
  int pq[TP];
#pragma unroll
  for (int tp = 0; tp < TP; ++tp) {
    const int pp = tp * 16 + frow;
    const int py = pp / W;
    pq[tp] = pp < R * W ? (wp * PR + py) * W2 + (pp - py * W) : 0;
  }

  x6f32x4 acc[TP][TC];
#pragma unroll
  for (int b = 0; b < TC; ++b) {
    const int c = c0 + (wc * TC + b) * 16 + 4 * fq;
    const float4 b4 = *(const float4*)(p.bias + c);
    const x6f32x4 bv = (x6f32x4){b4.x, b4.y, b4.z, b4.w} * st.acc_scale;
#pragma unroll
    for (int a = 0; a < TP; ++a) acc[a][b] = bv;
  }
  const int w_hh = x6_chunk(2 * fq, frow) << 4, w_ll = x6_chunk(2 * fq + 1, frow) << 4;
  const int fo = t0 + wp;                            // this wave's output frame

  // steps in (chunk, tap) order in sync groups of G taps: one wait + barrier
  // per group (conv_h3r_kernel)
  constexpr int NG = (27 + G - 1) / G;
  auto issue_group = [&](int c, int g, int half) {
    for (int j = 0; j < G && g * G + j < 27; ++j) issue_w((g * G + j) * nck + c, half * G + j);
  };
  issue_group(0, 0, 0);
  int half = 0;
  for (int c = 0; c < nck; ++c) {
    stage(c);
    x6d_wait_vm<0>();
    x6d_barrier();
#pragma unroll 1
    for (int g = 0; g < NG; ++g) {
      if (g + 1 < NG) issue_group(c, g + 1, half ^ 1);
      else if (c + 1 < nck) issue_group(c + 1, 0, half ^ 1);
#pragma unroll
      for (int j = 0; j < G; ++j) {
        const int t = g * G + j;
        const int dt = t / 9, r9 = t - 9 * dt;
        const int dh = r9 / 3, dw = r9 - 3 * dh;
        // the tap's input frame is a frame of the clip (wave-uniform)
        if (t < 27 && fo < T && (unsigned)(fo + dt - 1) < (unsigned)T) {
          const int toff = (dt * PR + dh) * W2 + dw;
          H3B bf[TP];
#pragma unroll
          for (int tp = 0; tp < TP; ++tp) {
            const int q = pq[tp] + toff;
            const char* base = lds + q * 128;
            bf[tp].h = *(const wu32x4*)(base + (x6r_swz(2 * fq, q) << 4));
            bf[tp].l = *(const wu32x4*)(base + (x6r_swz(2 * fq + 1, q) << 4));
          }
          const char* wb = wbuf + (half * G + j) * W_BYTES;
#pragma unroll
          for (int tc = 0; tc < TC; ++tc) {
            const char* wrow = wb + ((wc * TC + tc) * 16 + frow) * 128;
            const wu32x4 ah = *(const wu32x4*)(wrow + w_hh);
            const wu32x4 al = *(const wu32x4*)(wrow + w_ll);
#pragma unroll
            for (int tp = 0; tp < TP; ++tp) acc[tp][tc] = h3_mma(al, bf[tp].h, acc[tp][tc]);
#pragma unroll
            for (int tp = 0; tp < TP; ++tp) acc[tp][tc] = h3_mma(ah, bf[tp].l, acc[tp][tc]);
#pragma unroll
            for (int tp = 0; tp < TP; ++tp) acc[tp][tc] = h3_mma(ah, bf[tp].h, acc[tp][tc]);
          }
        }
      }
      x6d_wait_vm<0>();             // the next group's weights landed (this wave) ...
      x6d_barrier();                // ... in every wave; this group's LDS reads are done
      half ^= 1;
    }
  }

  // the wave's rows: R x W pixels of frame fo, contiguous in the output. A box
  // frame past the clip has no valid row; its range is clamped into the clip
  // so that every wave of the block sees the same video (ST)
  const int fc = min(fo, T - 1);
  const int p0 = ((n * T + fc) * H + r0) * W;
  const int m_end = fo < T ? p0 + rows * W : p0;
  x6d_epilogue<TP, TC, NW, C_TILE, ST>(p, st, acc, p0, m_end, p0 + TP * 16, c0, 0, wc, lane, lds,
                                       LDS_BYTES, st.out_scale);
}

// Variants: 4 waves as 2 frames x 2 channel halves, TP pixel tiles per frame
// x TC channel tiles per wave, HALO patch entries, G taps per barrier.
struct ConvH3VConfig {
  int tp, c_tile, halo;
  void (*kernel[2])(const ConvF32Params, const X6DStats);    // [st]
};
#define H3VCFG(TP, TC, HALO, G, MINB)                                               \
  {TP, 2 * TC * 16, HALO,                                                           \
   {conv_h3v_kernel<TP, TC, HALO, G, MINB, false>, conv_h3v_kernel<TP, TC, HALO, G, MINB, true>}}
static const ConvH3VConfig kH3VConfigs[] = {
    // 0: 2 x 112 px x 64 channels, 928 entries (56 x 56 frames in boxes of 2
    // rows: 4 x 4 x 58), 148 KB: layer1, the patch staged once in total
    H3VCFG(7, 2, 928, 2, 1),
    // 1: 2 x 112 px x 128 channels, 720 entries (28 x 28 in boxes of 4 rows,
    // 14 x 14 in boxes of 7), 154 KB
    H3VCFG(7, 4, 720, 2, 1),
    // 2: 2 x 64 px x 128 channels, 384 entries (7 x 7 frames whole: 4 x 9 x 9;
    // 14 x 14 in boxes of 4 rows), one tap per barrier, 80 KB: two blocks per CU
    H3VCFG(4, 4, 384, 1, 2),
};

extern "C" {

int rnb_conv_h3v_num_variants() { return (int)(sizeof(kH3VConfigs) / sizeof(kH3VConfigs[0])); }

// The box rule: output frames (*tf) and rows of a variant's box on T x H x W
// clips; 0 = the variant cannot run them. The rows are the most whose pixels
// fit the wave's tiles and whose patch fits the LDS, then evened out over the
// frame's boxes (14 rows at up to 8 per box: 7 + 7, not 8 + 6).
int rnb_conv_h3v_box(int variant, int T, int H, int W, int* tf) {
  if (variant < 0 || variant >= rnb_conv_h3v_num_variants()) return 0;
  const ConvH3VConfig& cfg = kH3VConfigs[variant];
  if (tf) *tf = H3V_TF;
  if (T < 2 || H < 1 || W < 1) return 0;
  int R = cfg.tp * 16 / W;
  if (R > H) R = H;
  while (R >= 1 && (H3V_TF + 2) * (R + 2) * (W + 2) > cfg.halo) --R;
  if (R < 1) return 0;
  const int nb = (H + R - 1) / R;
  return (H + nb - 1) / nb;
}

// output pixels per block
int rnb_conv_h3v_pixels(int variant) {
  if (variant < 0 || variant >= rnb_conv_h3v_num_variants()) return 0;
  return H3V_TF * kH3VConfigs[variant].tp * 16;
}

// blocks of a launch (0: the variant cannot run the shape)
long long rnb_conv_h3v_blocks(int variant, int N, int T, int H, int W, int Cout_p) {
  const int R = rnb_conv_h3v_box(variant, T, H, W, nullptr);
  if (R == 0) return 0;
  const int ct = kH3VConfigs[variant].c_tile;
  return (long long)N * ((T + H3V_TF - 1) / H3V_TF) * ((H + R - 1) / R) * ((Cout_p + ct - 1) / ct);
}

// blocks per CU of the variant's kernel; < 0: a HIP error
int rnb_conv_h3v_occupancy(int variant) {
  if (variant < 0 || variant >= rnb_conv_h3v_num_variants()) return -1;
  int nb = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &nb, (const void*)kH3VConfigs[variant].kernel[0], 256, 0);
  return e == hipSuccess ? nb : -(int)e;
}

int rnb_conv_h3v_launch(const ConvF32Params* pp, int variant, hipStream_t stream, double* sums,
                        const int* clip_seg, int stats_c, float in_scale, float out_scale) {
  if (variant < 0 || variant >= rnb_conv_h3v_num_variants()) return -1;
  ConvF32Params p = *pp;
  const ConvH3VConfig& cfg = kH3VConfigs[variant];
  if (p.KT != 3 || p.KH != 3 || p.KW != 3 || p.PT != 1 || p.PH != 1 || p.PW != 1) return -2;
  if (p.ST != 1 || p.SH != 1 || p.SW != 1 || p.Cin_p % 32 != 0 || p.Cout_p % 4 != 0) return -2;
  if (p.To != p.T || p.Ho != p.H || p.Wo != p.W) return -2;
  if (p.K_pad < 27 * p.Cin_p || p.K_pad % 32 != 0) return -3;
  if (p.M <= 0) return 0;
  if (p.M != p.N * p.T * p.H * p.W) return -3;
  if (p.y_stride < p.Cout_p || p.y_stride % 4 != 0 || (p.res && (p.res_stride < p.Cout_p ||
                                                               p.res_stride % 4 != 0)))
    return -4;
  const long long xb = (long long)p.N * p.T * p.H * p.W * p.Cin_p * 4;
  if (xb > 0x7FFFFF00LL || (long long)p.M * p.y_stride * 4 > 0x7FFFFF00LL) return -5;
  if (p.res && (long long)p.M * p.res_stride * 4 > 0x7FFFFF00LL) return -6;
  const int R = rnb_conv_h3v_box(variant, p.T, p.H, p.W, nullptr);
  if (R == 0) return -13;
  if ((long long)(p.K_pad / 32) * p.w_rows * 128 > 0x7FFFFF00LL) return -11;
  if (!(in_scale > 0.f) || !(out_scale > 0.f)) return -15;
  p.x_bytes = (uint32_t)xb;
  f32_magic_div((uint32_t)p.Wo, &p.mWo, &p.sWo);
  f32_magic_div((uint32_t)p.Ho, &p.mHo, &p.sHo);
  f32_magic_div((uint32_t)p.To, &p.mTo, &p.sTo);
  p.ngroups = R;                               // rows per box (read by the kernel)
  p.n_ptiles = (p.H + R - 1) / R;              // boxes per frame
  p.n_ctiles = (p.Cout_p + cfg.c_tile - 1) / cfg.c_tile;
  if (p.n_ctiles * cfg.c_tile > p.w_rows) return -8;
  const long long blocks = rnb_conv_h3v_blocks(variant, p.N, p.T, p.H, p.W, p.Cout_p);
  if (blocks > 0x7FFFFFFF) return -7;
  if (sums && (!clip_seg || stats_c < p.Cout_p)) return -12;
  X6DStats st;
  st.sums = sums;
  st.clip_seg = clip_seg;
  st.stats_c = stats_c;
  st.ksplit = 1;
  st.ws = nullptr;
  st.in_scale = in_scale;
  st.out_scale = out_scale;
  st.acc_scale = 1.f / out_scale;
  st.in_ss = nullptr;
  st.in_seg = nullptr;
  st.oflag = rnb_h3_range_flag();
  hipLaunchKernelGGL(cfg.kernel[sums ? 1 : 0], dim3((unsigned)blocks), dim3(256), 0, stream, p,
                     st);
  return (int)hipGetLastError();
}

}  // extern "C"
