// Frame-stacked, parity-staged 1x3x3 stride-(1,2,2) pad-(0,1,1) convolution in
// bf16 on CDNA4: the conv that opens layer2, layer3 and layer4 of mc3_18 and
// the spatial stride-2 conv of the downsampling blocks of R(2+1)D. The flat
// sibling of conv_vol2.hip.
//
// Why: the generic implicit-GEMM kernel (conv_igemm.hip) gathers nine 16-byte
// chunks per output pixel and 8 channels through LDS-DMA. At stride 2 an input
// value feeds 9 / 4 taps on average, so a block that stages the input PATCH of
// its output box once moves about 4 input pixels per output pixel plus halo.
//
// Box. No tap crosses a frame, so the N * T frames of a launch are one flat
// list and a box may span clips. A block owns F consecutive frames x Ro output
// rows x the full output width Wo (at most 256 pixels), times a tile of 128
// output channels. conv_vol2's box was one output frame (112 pixels at 28 x
// 28) because every further frame costs two more patch frames; here a frame
// costs exactly its own rows, so F is chosen by rnb_sp2_box to fill the box:
// 2 frames x 4 rows of a 28-wide output (224 pixels), one 14 x 14 frame (196),
// 4 frames of 7 x 7 (196). The last frame group of a launch is partial.
//
// Patch. Per 32-channel input chunk the F x (2 Ro + 1) patch rows are DMA'd
// into LDS as 64-byte entries (32 bf16), each row de-interleaved into an even
// and an odd plane of Wo + 1 padded columns (row stride RS = 2 (Wo + 1)); the
// permutation sits on the DMA's source offsets, the destination is
// lane-consecutive. Output pixel wo under tap dw reads plane dw & 1, entry
// wo + (dw >> 1), so the 16 pixels x 4 K-quarters of an MFMA B fragment are
// 1 KB of consecutive LDS under every tap and no swizzle is needed. Entries
// outside a frame's H x W (the left and top padding, the right and bottom
// padding of odd sizes, rows of a short last band, frames past the launch's
// last) get the invalid buffer offset and read zeros. A patch frame holds
// rows of its own frame only, so no tap ever reads another frame.
//
// Pipeline. Two patch buffers: chunk c + 1's patch is issued in nine pieces
// (at most one DMA instruction per wave and tap) under chunk c's nine taps.
// Weights come from the layer's wmat as it is (k = (dh * 3 + dw) * Cin_p + c:
// a (tap, chunk) slice is 64 contiguous bytes of every row) in stages of ONE
// tap (128 rows x 64 B = 8 KB, one DMA instruction per wave) through three
// buffers, two stages ahead. A stage ends with s_waitcnt vmcnt(1 + piece): the
// weight stage and the patch piece issued during it stay in flight, so every
// load has two stages (32 MFMAs per wave) to land; only tap 8 waits for all.
// Stages of three taps (24 KB x 2), as in conv_vol2, would leave 56 KB per
// patch buffer and boxes of 196 / 196 / 147 pixels; one-tap stages (8 KB x 3)
// leave 68 KB and admit the boxes above.
//
// Geometry: 8 waves = 4 pixel waves x 2 channel halves. The box's 16-pixel
// tiles are dealt round-robin to the pixel waves (tile j to wave j & 3), so a
// 196-pixel box is 4 + 3 + 3 + 3 tiles instead of 4 + 4 + 4 + 1; a wave skips
// the tiles it has not got (wave-uniform). Channel half cw owns the 64
// channels [64 cw, 64 cw + 64) of the tile: up to 4 x 4 accumulators of
// v_mfma_f32_16x16x32_bf16, A = weights, B = patch entries, 8 fragment reads
// per 16 MFMAs. The epilogue is conv_epilogue.h.
#include <hip/hip_runtime.h>
#include "lds_attr.h"
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "conv_epilogue.h"

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

#define SP2_INVALID 0xFFFFFFF0u
#define SP2_LDS_LIMIT (160 * 1024)
#define SP2_C_TILE 128
#define SP2_WBUF (SP2_C_TILE * 64)       // one weight stage: 1 tap x 128 rows x 64 B
#define SP2_NWBUF 3
#define SP2_MAX_PX 256                   // 16 tiles of 16 pixels
#define SP2_PI 9                         // patch DMA instructions per wave and chunk (one per tap)
// most patch entries: 2 buffers of ceil(np / 16) KB + 3 weight stages <= the LDS limit
#define SP2_MAX_NP (((SP2_LDS_LIMIT - SP2_NWBUF * SP2_WBUF) / 2048) * 16)

// Mirrored by rnb_amd/ops/native.py:Sp2Params (the launcher fills in
// n_ctiles .. x_bytes).
struct Sp2Params {
  const uint16_t* x;   // NDHWC input, Cin channels (multiple of 32)
  const uint16_t* w;   // [w_rows][K_pad], k = (dh*3 + dw) * Cin + c
  const float* bias;
  const uint16_t* res;
  uint16_t* y;
  int N, T, H, W, Cin;
  int Ho, Wo;
  int Cout_p, y_stride, res_stride;
  int K_pad, M, relu, w_rows;
  int n_ctiles;
  int F;               // frames per box
  int Ro;              // output rows per box
  int bands;           // ceil(Ho / Ro)
  int fgroups;         // ceil(N * T / F)
  int np;              // patch entries = F * (2 Ro + 1) * 2 * (Wo + 1)
  uint32_t x_bytes;
};

// One block = one box (frames [f0, f0 + F) of the flat list, output rows
// [ho0, ho0 + Ro)) x 128 output channels; 512 threads. LDS = 2 patch buffers +
// 3 weight stages.
__global__ __launch_bounds__(512, 1)
void conv_sp2_kernel(const Sp2Params p) {
  constexpr int NW = 8, TC = 4, HP = SP2_MAX_PX / 64, PI = SP2_PI;
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
  const int box = wgid / p.n_ctiles;
  const int band = box % p.bands;
  const int fg = box / p.bands;
  const int c0 = ctile * SP2_C_TILE;
  const int NF = p.N * p.T;
  const int f0 = fg * p.F;
  const int ho0 = band * p.Ro;
  const int nrows = min(p.Ro, p.Ho - ho0);
  const int fpx = nrows * p.Wo;                        // output pixels per box frame
  const int npx = min(p.F, NF - f0) * fpx;             // valid output pixels
  const int PL = p.Wo + 1;                             // entries per parity plane
  const int RS = 2 * PL;                               // entries per patch row
  const int PR = 2 * p.Ro + 1;                         // patch rows per frame
  const int FS = PR * RS;                              // entries per patch frame

  const int lent = lane >> 2;                          // entry / weight row within a DMA
  const uint32_t lq = (uint32_t)(lane & 3) * 16u;      // K-quarter byte offset
  const int n_instr = (p.np + 15) >> 4;
  // patch entry q = ((jf * PR + j) * 2 + plane) * PL + e <-> frame f0 + jf of
  // the flat list, row 2 ho0 - 1 + j, column 2 e + plane - 1; anything outside
  // the frame's H x W or past the last frame is invalid
  uint32_t poff[PI];
#pragma unroll
  for (int i = 0; i < PI; ++i) {
    const int instr = wave + NW * i;
    const int q = instr * 16 + lent;
    uint32_t off = SP2_INVALID;
    if (instr < n_instr && q < p.np) {
      const int jf = q / FS;
      const int r = q - jf * FS;
      const int j = r / RS;
      const int r2 = r - j * RS;
      const int plane = r2 >= PL ? 1 : 0;
      const int e = r2 - plane * PL;
      const int f = f0 + jf, h = 2 * ho0 - 1 + j, wc = 2 * e + plane - 1;
      if (f < NF && (unsigned)h < (unsigned)p.H && (unsigned)wc < (unsigned)p.W)
        off = (uint32_t)((f * p.H + h) * p.W + wc) * (uint32_t)(p.Cin * 2) + lq;
    }
    poff[i] = off;
  }

  const int frow = lane & 15;
  const int fq = lane >> 4;
  // tiles of this pixel wave: j = pw + 4 a, a < na
  const int ntiles = (npx + 15) >> 4;
  const int na = (ntiles - pw + 3) >> 2;
  int base[HP];           // patch entry of tap (0, 0) of the lane's pixel
  long long mrow[HP];     // output row of the lane's pixel
  bool ok[HP];
#pragma unroll
  for (int a = 0; a < HP; ++a) {
    const int i = (pw + 4 * a) * 16 + frow;            // pixel within the box
    ok[a] = i < npx;
    const int ic = min(i, npx - 1);
    const int ft = ic / fpx;
    const int r = ic - ft * fpx;
    const int hh = r / p.Wo;
    const int ww = r - hh * p.Wo;
    base[a] = ft * FS + 2 * hh * RS + ww;
    mrow[a] = ((long long)(f0 + ft) * p.Ho + (ho0 + hh)) * p.Wo + ww;
  }

  const __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.x, (short)0, p.x_bytes, 0x00020000);
  const uint32_t w_bytes = (uint32_t)p.w_rows * (uint32_t)p.K_pad * 2u;
  const __amdgpu_buffer_rsrc_t wr =
      __builtin_amdgcn_make_buffer_rsrc((void*)p.w, (short)0, w_bytes, 0x00020000);
  // this wave's 16 rows of a weight stage
  const uint32_t wrow_off = (uint32_t)(c0 + wave * 16 + lent) * (uint32_t)p.K_pad * 2u + lq;

  const int pbytes = n_instr * 1024;                   // one patch buffer
  char* wbase = smem + 2 * pbytes;

  // piece i of chunk's patch (this wave's instruction wave + 8 i) into buffer chunk & 1
  auto issue_patch = [&](int chunk, int i) {
    const uint32_t off = poff[i] == SP2_INVALID ? SP2_INVALID : poff[i] + (uint32_t)chunk * 64u;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        xr,
        (__attribute__((address_space(3))) void*)(smem + (chunk & 1) * pbytes +
                                                  (wave + NW * i) * 1024),
        16, off, 0, 0, 0);
  };
  // stage s = (chunk, tap): rows 16 wave .. + 15 of the tile into buffer s % 3
  auto issue_w = [&](int chunk, int tap, int buf) {
    const uint32_t kofs = (uint32_t)(tap * p.Cin + chunk * 32);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        wr, (__attribute__((address_space(3))) void*)(wbase + buf * SP2_WBUF + wave * 1024), 16,
        wrow_off + kofs * 2u, 0, 0, 0);
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
#pragma unroll
  for (int i = 0; i < PI; ++i)
    if (wave + NW * i < n_instr) issue_patch(0, i);
  issue_w(0, 0, 0);
  issue_w(0, 1, 1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int s = 0;                                       // stage = chunk * 9 + tap
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    const char* pbuf = smem + (chunk & 1) * pbytes + fq * 16;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap, ++s) {
      // weight buffer of stage s: s % 3 = tap % 3 (9 stages per chunk). Two
      // stages ahead: its buffer was read in stage s - 1, which ended in a barrier
      const int wb = tap % 3;
      if (s + 2 < nstages) {
        const int t2 = tap + 2;
        issue_w(t2 >= 9 ? chunk + 1 : chunk, t2 >= 9 ? t2 - 9 : t2, (tap + 2) % 3);
      }
      // the next chunk's patch: its buffer was read in chunk - 1
      const bool piece = chunk + 1 < nchunks && wave + NW * tap < n_instr;
      if (piece) issue_patch(chunk + 1, tap);
      {
        const int dh = tap / 3, dw = tap - 3 * dh;
        const int shift = dh * RS + (dw & 1) * PL + (dw >> 1);
        const char* wbp = wbase + wb * SP2_WBUF + (cw * TC * 16 + frow) * 64 + fq * 16;
        bf16x8 wf[TC];
#pragma unroll
        for (int tc = 0; tc < TC; ++tc) wf[tc] = *(const bf16x8*)(wbp + tc * 16 * 64);
#pragma unroll
        for (int a = 0; a < HP; ++a) {
          if (a < na) {
            const bf16x8 af = *(const bf16x8*)(pbuf + (base[a] + shift) * 64);
#pragma unroll
            for (int tc = 0; tc < TC; ++tc)
              acc[a][tc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[tc], af, acc[a][tc], 0, 0, 0);
          }
        }
      }
      // in flight past the barrier: this stage's weight load (for s + 2) and
      // patch piece; stage s + 1's weights, issued before them, have landed.
      // After tap 8 the next chunk's whole patch must have.
      if (tap == 8 || s + 2 >= nstages)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      else if (piece)
        asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else
        asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
      // the bare barrier: __syncthreads() would wait for every load in flight.
      // This stage's fragment reads must have left LDS (a wave without tiles
      // consumes none of them).
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
  }

  const EpCtx e = ep_make(p.y, p.y_stride, p.res, p.res_stride, p.M, p.Cout_p, p.relu != 0);
#pragma unroll
  for (int a = 0; a < HP; ++a) ep_row<TC>(e, ok[a], mrow[a], gt0, fq, acc[a]);
}

static inline int sp2_np(int F, int Ro, int Wo) { return F * (2 * Ro + 1) * 2 * (Wo + 1); }

extern "C" {

int rnb_sp2_params_size() { return (int)sizeof(Sp2Params); }
int rnb_sp2_num_variants() { return 1; }

// The box rule: frames F and output rows Ro of variant v's box on frames of
// H x W (T frames per clip; the flat list does not depend on it), returned as
// F * 65536 + Ro, 0 = the variant cannot run them. Ro runs over the even
// splits of the Ho output rows (ceil(Ho / nb)), F over what fits 256 pixels
// and the patch budget; the winner has the most output pixels per box on
// average (F * Ho * Wo / nb), then the fewest patch entries. 28 x 28 outputs:
// 2 x 4 rows (224 pixels, 1044 entries); 14 x 14: one frame (196, 870); 7 x 7:
// 4 frames (196, 960; a fifth would pass the patch budget of 1088 entries).
int rnb_sp2_box(int v, int T, int H, int W) {
  if (v != 0 || T < 1 || H < 1 || W < 1) return 0;
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  long long best_px = 0;
  int best_np = 0, best = 0;
  for (int nb = 1; nb <= Ho; ++nb) {
    const int R = (Ho + nb - 1) / nb;
    if ((Ho + R - 1) / R != nb) continue;            // the same R as a smaller nb
    if (R * Wo > SP2_MAX_PX || sp2_np(1, R, Wo) > SP2_MAX_NP) continue;
    int F = SP2_MAX_PX / (R * Wo);
    if (F > SP2_MAX_NP / sp2_np(1, R, Wo)) F = SP2_MAX_NP / sp2_np(1, R, Wo);
    if (F > 32767) F = 32767;
    const long long px = (long long)F * Ho * Wo * 1024 / nb;   // average per box, x 1024
    const int np = sp2_np(F, R, Wo);
    if (px > best_px || (px == best_px && np < best_np)) {
      best_px = px;
      best_np = np;
      best = F * 65536 + R;
    }
  }
  return best;
}

// LDS bytes a launch of variant v on this shape requests (-1: not supported).
int rnb_sp2_lds_bytes(int v, int T, int H, int W, int Cin) {
  const int box = rnb_sp2_box(v, T, H, W);
  if (box == 0 || Cin < 32 || Cin % 32 != 0) return -1;
  const int np = sp2_np(box >> 16, box & 0xFFFF, (W + 1) / 2);
  const int lds = 2 * ((np + 15) >> 4) * 1024 + SP2_NWBUF * SP2_WBUF;
  return lds <= SP2_LDS_LIMIT ? lds : -1;
}

// blocks per CU of the kernel with `lds` dynamic bytes; < 0: a HIP error
int rnb_sp2_occupancy(int v, int lds) {
  if (v != 0) return -1;
  rnb_ensure_max_lds((const void*)conv_sp2_kernel);
  int nb = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &nb, (const void*)conv_sp2_kernel, 512, (size_t)lds);
  return e == hipSuccess ? nb : -(int)e;
}

int rnb_sp2_launch(const Sp2Params* pp, int v, hipStream_t stream) {
  if (v != 0) return -10;
  Sp2Params p = *pp;
  if (p.N < 0 || p.T < 1 || p.H < 1 || p.W < 1) return -1;
  if (p.Cin < 32 || p.Cin % 32 != 0 || p.K_pad < 9 * p.Cin || p.K_pad % 8 != 0 ||
      p.Cout_p < 4 || p.Cout_p % 4 != 0)
    return -2;
  if (p.Ho != (p.H + 1) / 2 || p.Wo != (p.W + 1) / 2) return -3;
  if (p.M <= 0) return 0;
  if ((long long)p.M != (long long)p.N * p.T * p.Ho * p.Wo) return -3;
  const long long xb = (long long)p.N * p.T * p.H * p.W * p.Cin * 2;
  if (xb > 0x7FFFFF00LL) return -5;
  const int box = rnb_sp2_box(v, p.T, p.H, p.W);
  if (box == 0) return -4;
  p.F = box >> 16;
  p.Ro = box & 0xFFFF;
  p.bands = (p.Ho + p.Ro - 1) / p.Ro;
  p.fgroups = (int)(((long long)p.N * p.T + p.F - 1) / p.F);
  p.np = sp2_np(p.F, p.Ro, p.Wo);
  if (p.np > SP2_MAX_NP || p.np > 8 * SP2_PI * 16 || p.F * p.Ro * p.Wo > SP2_MAX_PX) return -4;
  const int lds = rnb_sp2_lds_bytes(v, p.T, p.H, p.W, p.Cin);
  if (lds < 0 || lds > SP2_LDS_LIMIT) return -6;
  p.x_bytes = (uint32_t)xb;
  p.n_ctiles = (p.Cout_p + SP2_C_TILE - 1) / SP2_C_TILE;
  if (p.n_ctiles * SP2_C_TILE > p.w_rows) return -8;
  if ((long long)p.w_rows * p.K_pad * 2 > 0xFFFFFF00LL) return -8;
  if (p.y_stride < p.Cout_p || (p.res && p.res_stride < p.Cout_p)) return -9;
  if ((long long)p.M * p.y_stride * 2 > 0xFFFFFF00LL ||
      (long long)p.M * (p.res ? p.res_stride : 0) * 2 > 0xFFFFFF00LL) return -11;
  const long long blocks = (long long)p.fgroups * p.bands * p.n_ctiles;
  if (blocks > 0x7FFFFFFFLL) return -7;
  rnb_ensure_max_lds((const void*)conv_sp2_kernel);
  hipLaunchKernelGGL(conv_sp2_kernel, dim3((unsigned)blocks), dim3(512), lds, stream, p);
  return (int)hipGetLastError();
}

}  // extern "C"
