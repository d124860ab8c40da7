// GPU half of the MJPEG decode backend: dequantise + 8x8 inverse DCT of the
// frame records the host entropy decoder (jpeg_entropy.cpp) produced.
//
//  * rnb_jpeg_idct   nframes records (uint16 qt[3][64], then int16 quantised
//                    coefficients, 64 per block in natural order: Y blocks
//                    row-major over the padded 2*mh x 2*mw grid, then Cb, then
//                    Cr; see jpeg_entropy.cpp) -> 8-bit planar I420 frames at
//                    the padded size: Y [16*mh][16*mw], Cb and Cr
//                    [8*mh][8*mw], 384*mw*mh bytes per frame. Per sample:
//                    coefficient x table entry, separable 8-point IDCT in
//                    fp32, + 128, round to nearest, clamp to [0, 255].
//  * rnb_jpeg_idct_s the same for any of the three chroma layouts (sampling 0:
//                    4:2:0 as above, 1: 4:2:2, 2: 4:4:4; luma factors Hs x Vs =
//                    2x2, 2x1, 1x1): a record holds B = Hs Vs + 2 blocks per MCU,
//                    the Y blocks row-major over the padded (Vs mh) x (Hs mw)
//                    grid, then Cb, then Cr (384 + 128 B mw mh bytes); the frame
//                    is Y [8 Vs mh][8 Hs mw], Cb and Cr [8 mh][8 mw], 64 B mw mh
//                    bytes.
//  * rnb_jpeg_idct_r the same at 1 / reduce of the size (reduce 1, 2, 4, 8;
//                    N = 8 / reduce samples per block and axis), each sample
//                    the reduce x reduce box mean of the unrounded full-size
//                    samples (libjpeg's scale_denom): frames of Y
//                    [N Vs mh][N Hs mw], Cb and Cr [N mh][N mw], N^2 B mw mh
//                    bytes. reduce = 1 is rnb_jpeg_idct_s.
//
// Every address is a function of (frame, block, line) and the geometry the
// launcher validated, never of a coefficient: corrupt coefficients give wrong
// pixels, not wrong addresses. Every byte of the surface's nframes frames is
// written, the padding rows and columns included.
#include <hip/hip_runtime.h>
#include <stdint.h>

// kJpegBasis[x][u] = c(u) / 2 * cos((2x + 1) u pi / 16), c(0) = 1/sqrt(2)
__device__ __attribute__((aligned(16))) const float kJpegBasis[8][8] = {
    {0.35355339f, 0.49039264f, 0.46193977f, 0.41573481f, 0.35355339f, 0.27778512f, 0.19134172f, 0.09754516f},
    {0.35355339f, 0.41573481f, 0.19134172f, -0.09754516f, -0.35355339f, -0.49039264f, -0.46193977f, -0.27778512f},
    {0.35355339f, 0.27778512f, -0.19134172f, -0.49039264f, -0.35355339f, 0.09754516f, 0.46193977f, 0.41573481f},
    {0.35355339f, 0.09754516f, -0.46193977f, -0.27778512f, 0.35355339f, 0.41573481f, -0.19134172f, -0.49039264f},
    {0.35355339f, -0.09754516f, -0.46193977f, 0.27778512f, 0.35355339f, -0.41573481f, -0.19134172f, 0.49039264f},
    {0.35355339f, -0.27778512f, -0.19134172f, 0.49039264f, -0.35355339f, -0.09754516f, 0.46193977f, -0.41573481f},
    {0.35355339f, -0.41573481f, 0.19134172f, 0.09754516f, -0.35355339f, 0.49039264f, -0.46193977f, 0.27778512f},
    {0.35355339f, -0.49039264f, 0.46193977f, -0.41573481f, 0.35355339f, -0.27778512f, 0.19134172f, -0.09754516f},
};

#define JPEG_BLOCKS_PER_WG 32      // 8 threads per 8x8 block, 256 threads
// LDS image of one block's half-transformed values: 8 rows of 8 floats, rows
// 12 floats apart and blocks 100 floats apart, so that the 16-byte writes of a
// block's 8 lanes and the (broadcast) 16-byte reads of a wave's 8 blocks fall
// on distinct 4-bank slots
#define JPEG_ROW_STRIDE 12
#define JPEG_BLK_STRIDE 100

struct JpegIdctArgs {
  long long record_bytes;
  long long total_blocks;          // nframes * B * mw * mh
  int mw, mh;
};

static __device__ __forceinline__ uint32_t jpeg_sample(float s) {
  // + 128, round to nearest (ties to even), clamp
  return (uint32_t)min(max(__float2int_rn(s + 128.f), 0), 255);
}

// One thread per 8-sample line, 8 threads per block. Thread j first holds
// coefficient row j (one aligned 16-byte load, plus the 16 bytes of its
// component's table row), dequantises it and transforms it along the row in
// registers; the 8x8 intermediate goes through LDS; thread x then transforms
// along the columns for output row x and ends with 8 adjacent samples, written
// with one 8-byte store. Blocks that are neighbours in x are neighbours in the
// record, so a wave's stores form 64-byte runs per row. HS, VS: the luma
// sampling factors; block -> (component, plane position) follows from them and
// (mw, mh) alone.
template <int HS, int VS>
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const uint8_t* __restrict__ rec,
                                                        uint8_t* __restrict__ surf,
                                                        JpegIdctArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[JPEG_BLOCKS_PER_WG * JPEG_BLK_STRIDE];
  const int t = (int)threadIdx.x;
  const int line = t & 7, lb = t >> 3;
  const long long gb = (long long)blockIdx.x * JPEG_BLOCKS_PER_WG + lb;
  const bool live = gb < a.total_blocks;
  const int n = a.mw * a.mh;                     // MCUs per frame
  constexpr int NY = HS * VS;                    // Y blocks per MCU
  const int per_frame = (NY + 2) * n;
  const long long frame = live ? gb / per_frame : 0;
  const int b = live ? (int)(gb - frame * per_frame) : 0;
  const int comp = b < NY * n ? 0 : (b < (NY + 1) * n ? 1 : 2);
  float* tile = lds + lb * JPEG_BLK_STRIDE;
  if (live) {
    const uint8_t* r = rec + frame * a.record_bytes;
    const uint4 cw = *(const uint4*)(r + 384 + (long long)b * 128 + line * 16);
    const uint4 qw = *(const uint4*)(r + comp * 128 + line * 16);
    const uint32_t cs[4] = {cw.x, cw.y, cw.z, cw.w}, qs[4] = {qw.x, qw.y, qw.z, qw.w};
    float f[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {                // |coef * q| < 2^24: exact in fp32
      f[2 * i] = (float)(int)(int16_t)(cs[i] & 0xFFFFu) * (float)(qs[i] & 0xFFFFu);
      f[2 * i + 1] = (float)(int)(int16_t)(cs[i] >> 16) * (float)(qs[i] >> 16);
    }
    float h[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) {
      float s = 0.f;
#pragma unroll
      for (int v = 0; v < 8; ++v) s += f[v] * kJpegBasis[y][v];
      h[y] = s;
    }
    float4* row = (float4*)(tile + line * JPEG_ROW_STRIDE);
    row[0] = make_float4(h[0], h[1], h[2], h[3]);
    row[1] = make_float4(h[4], h[5], h[6], h[7]);
  }
  __syncthreads();
  if (!live) return;
  const float4 b0 = *(const float4*)&kJpegBasis[line][0];
  const float4 b1 = *(const float4*)&kJpegBasis[line][4];
  const float bu[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float4 lo = *(const float4*)(tile + u * JPEG_ROW_STRIDE);
    const float4 hi = *(const float4*)(tile + u * JPEG_ROW_STRIDE + 4);
    s[0] += bu[u] * lo.x; s[1] += bu[u] * lo.y; s[2] += bu[u] * lo.z; s[3] += bu[u] * lo.w;
    s[4] += bu[u] * hi.x; s[5] += bu[u] * hi.y; s[6] += bu[u] * hi.z; s[7] += bu[u] * hi.w;
  }
  const uint32_t w0 = jpeg_sample(s[0]) | (jpeg_sample(s[1]) << 8) | (jpeg_sample(s[2]) << 16) |
                      (jpeg_sample(s[3]) << 24);
  const uint32_t w1 = jpeg_sample(s[4]) | (jpeg_sample(s[5]) << 8) | (jpeg_sample(s[6]) << 16) |
                      (jpeg_sample(s[7]) << 24);
  // block -> plane position (all from the geometry)
  int pb = b, cols = HS * a.mw;
  long long plane = 0;
  if (comp) {
    pb = b - (NY - 1 + comp) * n;
    cols = a.mw;
    plane = (long long)(64 * (NY - 1) + 64 * comp) * n;    // 4:2:0: 256 n (Cb), 320 n (Cr)
  }
  const int by = pb / cols, bx = pb - by * cols;
  uint8_t* dst = surf + frame * (64LL * (NY + 2) * n) + plane +
                 ((long long)by * 8 + line) * (8 * cols) + bx * 8;
  *(uint2*)dst = make_uint2(w0, w1);
}

// Reduced-size decode (reduce = s in {2, 4, 8}, N = 8 / s samples per block
// and axis): the reduced sample is the s x s box mean of the unrounded,
// unclamped full-size samples, i.e. the same separable transform with the
// box-averaged basis Bs[i][u] = 1/s sum_{x in [s i, s i + s)} kJpegBasis[x][u]
// (fp32 constants derived in fp64). Columns of Bs that are zero (u = 4 for
// s = 2; u = 2, 4, 6 for s = 4) are skipped: their coefficient rows are never
// loaded. The frame is Y [N Vs mh][N Hs mw], Cb, Cr [N mh][N mw], N^2 B mw mh
// bytes, every byte written once.
__device__ __attribute__((aligned(16))) const float kJpegBasisHalf[4][8] = {
    {0.353553385f, 0.453063726f, 0.326640755f, 0.159094825f, 0.f, -0.106303759f, -0.135299027f, -0.0901199803f},
    {0.353553385f, 0.187665135f, -0.326640755f, -0.384088874f, 0.f, 0.256639987f, 0.135299027f, -0.0373289175f},
    {0.353553385f, -0.187665135f, -0.326640755f, 0.384088874f, 0.f, -0.256639987f, 0.135299027f, 0.0373289175f},
    {0.353553385f, -0.453063726f, 0.326640755f, -0.159094825f, 0.f, 0.106303759f, -0.135299027f, 0.0901199803f},
};
__device__ __attribute__((aligned(16))) const float kJpegBasisQuarter[2][8] = {
    {0.353553385f, 0.320364445f, 0.f, -0.112497024f, 0.f, 0.0751681104f, 0.f, -0.0637244508f},
    {0.353553385f, -0.320364445f, 0.f, 0.112497024f, 0.f, -0.0751681104f, 0.f, 0.0637244508f},
};

template <int N>
static __device__ __forceinline__ const float* jpeg_bs_row(int i) {
  return N == 4 ? kJpegBasisHalf[i] : kJpegBasisQuarter[i];
}

// column u of Bs is zero
template <int N>
static __device__ __forceinline__ constexpr bool jpeg_bs_zero(int u) {
  return N == 4 ? u == 4 : (u == 2 || u == 4 || u == 6);
}

// N = 4 or 2. Pass 1 as in jpeg_idct_kernel (8 lanes per block, lane u holds
// coefficient row u, dequantises it and leaves its N row outputs in LDS; the
// lanes of zero columns of Bs do nothing); pass 2 on the lanes line < N, each
// output row `line` of the block: N adjacent samples, one N-byte store.
template <int HS, int VS, int N>
__global__ __launch_bounds__(256) void jpeg_idct_reduced_kernel(const uint8_t* __restrict__ rec,
                                                                uint8_t* __restrict__ surf,
                                                                JpegIdctArgs a) {
  static_assert(N == 4 || N == 2, "N = 4 or 2");
  __shared__ __attribute__((aligned(16))) float lds[JPEG_BLOCKS_PER_WG * JPEG_BLK_STRIDE];
  const int t = (int)threadIdx.x;
  const int line = t & 7, lb = t >> 3;
  const long long gb = (long long)blockIdx.x * JPEG_BLOCKS_PER_WG + lb;
  const bool live = gb < a.total_blocks;
  const int n = a.mw * a.mh;                     // MCUs per frame
  constexpr int NY = HS * VS;                    // Y blocks per MCU
  const int per_frame = (NY + 2) * n;
  const long long frame = live ? gb / per_frame : 0;
  const int b = live ? (int)(gb - frame * per_frame) : 0;
  const int comp = b < NY * n ? 0 : (b < (NY + 1) * n ? 1 : 2);
  float* tile = lds + lb * JPEG_BLK_STRIDE;
  if (live && !jpeg_bs_zero<N>(line)) {
    const uint8_t* r = rec + frame * a.record_bytes;
    const uint4 cw = *(const uint4*)(r + 384 + (long long)b * 128 + line * 16);
    const uint4 qw = *(const uint4*)(r + comp * 128 + line * 16);
    const uint32_t cs[4] = {cw.x, cw.y, cw.z, cw.w}, qs[4] = {qw.x, qw.y, qw.z, qw.w};
    float f[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {                // |coef * q| < 2^24: exact in fp32
      f[2 * i] = (float)(int)(int16_t)(cs[i] & 0xFFFFu) * (float)(qs[i] & 0xFFFFu);
      f[2 * i + 1] = (float)(int)(int16_t)(cs[i] >> 16) * (float)(qs[i] >> 16);
    }
    float h[N];
#pragma unroll
    for (int y = 0; y < N; ++y) {
      float s = 0.f;
#pragma unroll
      for (int v = 0; v < 8; ++v)
        if (!jpeg_bs_zero<N>(v)) s += f[v] * jpeg_bs_row<N>(y)[v];
      h[y] = s;
    }
    if constexpr (N == 4)
      *(float4*)(tile + line * JPEG_ROW_STRIDE) = make_float4(h[0], h[1], h[2], h[3]);
    else
      *(float2*)(tile + line * JPEG_ROW_STRIDE) = make_float2(h[0], h[1]);
  }
  __syncthreads();
  if (!live || line >= N) return;
  const float4 b0 = *(const float4*)(jpeg_bs_row<N>(line));
  const float4 b1 = *(const float4*)(jpeg_bs_row<N>(line) + 4);
  const float bu[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
  float s[N];
#pragma unroll
  for (int j = 0; j < N; ++j) s[j] = 0.f;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    if (jpeg_bs_zero<N>(u)) continue;
    if constexpr (N == 4) {
      const float4 lo = *(const float4*)(tile + u * JPEG_ROW_STRIDE);
      s[0] += bu[u] * lo.x; s[1] += bu[u] * lo.y; s[2] += bu[u] * lo.z; s[3] += bu[u] * lo.w;
    } else {
      const float2 lo = *(const float2*)(tile + u * JPEG_ROW_STRIDE);
      s[0] += bu[u] * lo.x; s[1] += bu[u] * lo.y;
    }
  }
  // block -> plane position (all from the geometry)
  int pb = b, cols = HS * a.mw;
  long long plane = 0;
  if (comp) {
    pb = b - (NY - 1 + comp) * n;
    cols = a.mw;
    plane = (long long)(N * N * (NY - 1 + comp)) * n;
  }
  const int by = pb / cols, bx = pb - by * cols;
  uint8_t* dst = surf + frame * ((long long)(N * N * (NY + 2)) * n) + plane +
                 ((long long)by * N + line) * (N * cols) + bx * N;
  if constexpr (N == 4)
    *(uint32_t*)dst = jpeg_sample(s[0]) | (jpeg_sample(s[1]) << 8) | (jpeg_sample(s[2]) << 16) |
                      (jpeg_sample(s[3]) << 24);
  else
    *(uint16_t*)dst = (uint16_t)(jpeg_sample(s[0]) | (jpeg_sample(s[1]) << 8));
}

// N = 1 (reduce = 8): one thread per block, sample = F[0][0] / 8 + 128. The
// blocks of a plane are row-major over its grid, the planes follow each other
// as the components do in the record, so block b of a frame is byte b of it.
template <int NB>
__global__ __launch_bounds__(256) void jpeg_idct_dc_kernel(const uint8_t* __restrict__ rec,
                                                           uint8_t* __restrict__ surf,
                                                           JpegIdctArgs a) {
  const long long gb = (long long)blockIdx.x * 256 + (int)threadIdx.x;
  if (gb >= a.total_blocks) return;
  const int n = a.mw * a.mh;
  const int per_frame = NB * n;
  const long long frame = gb / per_frame;
  const int b = (int)(gb - frame * per_frame);
  const int comp = b < (NB - 2) * n ? 0 : (b < (NB - 1) * n ? 1 : 2);
  const uint8_t* r = rec + frame * a.record_bytes;
  const float f = (float)(int)*(const int16_t*)(r + 384 + (long long)b * 128) *
                  (float)*(const uint16_t*)(r + comp * 128);
  surf[frame * per_frame + b] = (uint8_t)jpeg_sample(f * 0.125f);
}

// sampling: 0 4:2:0, 1 4:2:2, 2 4:4:4; reduce: 1, 2, 4, 8 (-2 otherwise)
static int jpeg_idct_launch(const void* rec, long long rec_len, long long record_bytes,
                            int nframes, int mw, int mh, void* surf, long long surf_len,
                            int sampling, int reduce, hipStream_t stream) {
  if (reduce != 1 && reduce != 2 && reduce != 4 && reduce != 8) return -2;
  if (nframes == 0) return 0;
  if (nframes < 0 || mw < 1 || mh < 1 || mw > 4096 || mh > 4096) return -2;
  if (sampling < 0 || sampling > 2) return -2;
  const long long nb = sampling == 0 ? 6 : sampling == 1 ? 4 : 3;    // blocks per MCU
  const long long n = (long long)mw * mh;
  const long long N = 8 / reduce;                 // samples per block and axis = store width
  if (((uintptr_t)rec & 15u) != 0 || ((uintptr_t)surf & (uintptr_t)(N - 1)) != 0 ||
      record_bytes % 16 != 0)
    return -2;
  if (record_bytes < 384 + 128 * nb * n) return -4;
  if (rec_len < 0 || surf_len < 0 || record_bytes > rec_len / nframes ||
      N * N * nb * n > surf_len / nframes)
    return -4;
  const long long total = nb * n * nframes;
  const long long per_wg = N == 1 ? 256 : JPEG_BLOCKS_PER_WG;
  const long long groups = (total + per_wg - 1) / per_wg;
  if (groups > 0x7FFFFFFFLL) return -2;
  JpegIdctArgs a;
  a.record_bytes = record_bytes;
  a.total_blocks = total;
  a.mw = mw;
  a.mh = mh;
  auto kernel = sampling == 0 ? jpeg_idct_kernel<2, 2>
                              : sampling == 1 ? jpeg_idct_kernel<2, 1> : jpeg_idct_kernel<1, 1>;
  if (N == 4)
    kernel = sampling == 0 ? jpeg_idct_reduced_kernel<2, 2, 4>
                           : sampling == 1 ? jpeg_idct_reduced_kernel<2, 1, 4>
                                           : jpeg_idct_reduced_kernel<1, 1, 4>;
  else if (N == 2)
    kernel = sampling == 0 ? jpeg_idct_reduced_kernel<2, 2, 2>
                           : sampling == 1 ? jpeg_idct_reduced_kernel<2, 1, 2>
                                           : jpeg_idct_reduced_kernel<1, 1, 2>;
  else if (N == 1)
    kernel = sampling == 0 ? jpeg_idct_dc_kernel<6>
                           : sampling == 1 ? jpeg_idct_dc_kernel<4> : jpeg_idct_dc_kernel<3>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(256), 0, stream, (const uint8_t*)rec,
                     (uint8_t*)surf, a);
  return (int)hipGetLastError();
}

extern "C" {

// rec: nframes records record_bytes apart (rec_len bytes in all); surf:
// surf_len bytes, receives nframes frames of 384*mw*mh bytes. -2: bad shape or
// alignment; -4: a record or a frame would reach outside its buffer (nothing
// is launched).
int rnb_jpeg_idct(const void* rec, long long rec_len, long long record_bytes, int nframes,
                  int mw, int mh, void* surf, long long surf_len, hipStream_t stream) {
  return jpeg_idct_launch(rec, rec_len, record_bytes, nframes, mw, mh, surf, surf_len, 0, 1, stream);
}

// The same for 4:2:0 / 4:2:2 / 4:4:4 records (sampling 0 / 1 / 2): records of
// >= 384 + 128 B mw mh bytes, frames of 64 B mw mh bytes, B = 6 / 4 / 3.
int rnb_jpeg_idct_s(const void* rec, long long rec_len, long long record_bytes, int nframes,
                    int mw, int mh, void* surf, long long surf_len, int sampling,
                    hipStream_t stream) {
  return jpeg_idct_launch(rec, rec_len, record_bytes, nframes, mw, mh, surf, surf_len, sampling,
                          1, stream);
}

// The same at 1 / reduce of the size (reduce 1, 2, 4, 8; N = 8 / reduce): frames
// of N^2 B mw mh bytes, Y [N Vs mh][N Hs mw], Cb, Cr [N mh][N mw]; reduce = 1
// is rnb_jpeg_idct_s. surf must be aligned to N bytes. -2 also for another
// reduce; -4 when N^2 B mw mh > surf_len / nframes.
int rnb_jpeg_idct_r(const void* rec, long long rec_len, long long record_bytes, int nframes,
                    int mw, int mh, void* surf, long long surf_len, int sampling, int reduce,
                    hipStream_t stream) {
  return jpeg_idct_launch(rec, rec_len, record_bytes, nframes, mw, mh, surf, surf_len, sampling,
                          reduce, stream);
}

}  // extern "C"
