// Per-video class scores for gfx950: softmax per row, row sum / mean per video,
// top-k with a fixed tie rule. The last step of the multi-clip, multi-view
// evaluation protocol; the GPU form of ops/video.py's video_scores mirror.
//
//  * rnb_video_scores   [rows][ncls] logits + [nvid+1] row offsets ->
//                       [nvid][ncls] scores, [nvid][k] top values / indices
//
// One workgroup of 256 threads (four waves) per video. Thread t owns classes
// t, t+256, ... and keeps one fp32 accumulator per class in registers, added
// to in row order: the order of video_reduce_kernel, so the logit sums agree
// with it bit for bit whatever the launch geometry. With softmax on, the rows
// are taken in chunks of SC_CHUNK: the waves first leave (max, sum of exp) of
// every row of the chunk in LDS, each row read once into one wave's registers,
// then every thread adds exp(x - max) / sum of its classes over the chunk's
// rows. LDS use is fixed; the row count is unbounded. No atomics, no host
// sync, no allocation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define SC_THREADS 256
#define SC_WAVES (SC_THREADS / 64)
#define SC_CHUNK 16
#define SC_MAX_CLS 4096
#define SC_MAX_K 16

// error codes of rnb_video_scores (ops/native.py names the argument)
#define SC_ERR_NCLS (-21)
#define SC_ERR_K (-22)
#define SC_ERR_PTR (-23)

__device__ __forceinline__ float sc_wave_max(float v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  return v;
}

__device__ __forceinline__ float sc_wave_sum(float v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// larger value first, lower index on equal values
__device__ __forceinline__ bool sc_better(float av, int ai, float bv, int bi) {
  return av > bv || (av == bv && ai < bi);
}

// NJ = classes per thread (ncls <= NJ * 256); acc[] is indexed by unrolled
// constants only, so it stays in registers
template <int NJ>
__global__ __launch_bounds__(SC_THREADS) void video_scores_kernel(
    const float* __restrict__ logits, const int* __restrict__ offsets,
    float* __restrict__ scores, float* __restrict__ top_val, int* __restrict__ top_idx,
    int ncls, int k, int softmax, int mean) {
  constexpr int NV = NJ * SC_THREADS / 64;   // classes per lane when a wave holds a row
  constexpr int RU = NJ <= 2 ? 4 : 1;        // rows a wave holds at once
  __shared__ float rmax[SC_CHUNK];
  __shared__ float rsum[SC_CHUNK];
  __shared__ float wv[2][SC_WAVES];
  __shared__ int wi[2][SC_WAVES];
  const int v = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int c0 = offsets[v], c1 = offsets[v + 1];

  float acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = 0.f;

  if (softmax) {
    for (int b0 = c0; b0 < c1; b0 += SC_CHUNK) {
      const int nr = min(SC_CHUNK, c1 - b0);
      // a wave reads RU rows at once, each once, into registers (lane l holds
      // classes l, l+64, ...): the loads of all of them are in flight together
      for (int r0 = wave * RU; r0 < nr; r0 += SC_WAVES * RU) {
        float xv[RU][NV];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
          const float* row = logits + (size_t)(b0 + min(r0 + u, nr - 1)) * ncls;
#pragma unroll
          for (int i = 0; i < NV; ++i) {
            const int o = lane + i * 64;
            xv[u][i] = o < ncls ? row[o] : -INFINITY;
          }
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
          float m = -INFINITY;
#pragma unroll
          for (int i = 0; i < NV; ++i) m = fmaxf(m, xv[u][i]);
          m = sc_wave_max(m);
          float s = 0.f;
#pragma unroll
          for (int i = 0; i < NV; ++i)
            if (lane + i * 64 < ncls) s += expf(xv[u][i] - m);
          s = sc_wave_sum(s);
          if (lane == 0 && r0 + u < nr) { rmax[r0 + u] = m; rsum[r0 + u] = s; }
        }
      }
      __syncthreads();
#pragma unroll 4
      for (int r = 0; r < nr; ++r) {
        const float* row = logits + (size_t)(b0 + r) * ncls;
        const float m = rmax[r], s = rsum[r];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int o = t + j * SC_THREADS;
          if (o < ncls) acc[j] += expf(row[o] - m) / s;
        }
      }
      __syncthreads();          // rmax / rsum are rewritten by the next chunk
    }
  } else {
#pragma unroll 4
    for (int c = c0; c < c1; ++c) {
      const float* row = logits + (size_t)c * ncls;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const int o = t + j * SC_THREADS;
        if (o < ncls) acc[j] += row[o];
      }
    }
  }

  if (mean && c1 > c0) {
    const float n = (float)(c1 - c0);
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = acc[j] / n;
  }
  if (scores) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int o = t + j * SC_THREADS;
      if (o < ncls) scores[(size_t)v * ncls + o] = acc[j];
    }
  }
  if (c1 <= c0) {               // empty video (uniform over the block)
    if (t < k) { top_val[(size_t)v * k + t] = 0.f; top_idx[(size_t)v * k + t] = -1; }
    return;
  }

  // k rounds of block arg-max over the classes not yet taken
  uint32_t taken = 0;
  for (int round = 0; round < k; ++round) {
    float best = -INFINITY;
    int besti = 0x7FFFFFFF;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int o = t + j * SC_THREADS;
      if (o < ncls && !(taken & (1u << j)) && sc_better(acc[j], o, best, besti)) {
        best = acc[j];
        besti = o;
      }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const float ov = __shfl_xor(best, d, 64);
      const int oi = __shfl_xor(besti, d, 64);
      if (sc_better(ov, oi, best, besti)) { best = ov; besti = oi; }
    }
    const int buf = round & 1;  // two buffers: one barrier per round is enough
    if (lane == 0) { wv[buf][wave] = best; wi[buf][wave] = besti; }
    __syncthreads();
    best = wv[buf][0];
    besti = wi[buf][0];
#pragma unroll
    for (int w = 1; w < SC_WAVES; ++w)
      if (sc_better(wv[buf][w], wi[buf][w], best, besti)) { best = wv[buf][w]; besti = wi[buf][w]; }
    // nothing comparable left (NaN scores only): no index
    const bool none = besti == 0x7FFFFFFF;
    if (t == 0) {
      top_val[(size_t)v * k + round] = none ? 0.f : best;
      top_idx[(size_t)v * k + round] = none ? -1 : besti;
    }
    if (!none && (besti & (SC_THREADS - 1)) == t) taken |= 1u << (besti / SC_THREADS);
  }
}

extern "C" {

// logits: [rows][ncls]; offsets: [nvid+1]; scores: [nvid][ncls] or null;
// top_val / top_idx: [nvid][k]. softmax: rows -> softmax first; mean: divide
// the row sum by the row count. Returns 0, a negative SC_ERR_* code (nothing
// launched) or a hipError.
int rnb_video_scores(const float* logits, const int* offsets, float* scores, float* top_val,
                     int* top_idx, int nvid, int ncls, int k, int softmax, int mean,
                     hipStream_t stream) {
  if (ncls < 1 || ncls > SC_MAX_CLS) return SC_ERR_NCLS;
  if (k < 1 || k > SC_MAX_K || k > ncls) return SC_ERR_K;
  if (nvid <= 0) return 0;
  // logits may be null: a tensor of no rows (every video empty) has no storage
  if (!offsets || !top_val || !top_idx) return SC_ERR_PTR;
  const dim3 grid(nvid), block(SC_THREADS);
  if (ncls <= 2 * SC_THREADS)
    hipLaunchKernelGGL(video_scores_kernel<2>, grid, block, 0, stream, logits, offsets, scores,
                       top_val, top_idx, ncls, k, softmax, mean);
  else
    hipLaunchKernelGGL(video_scores_kernel<SC_MAX_CLS / SC_THREADS>, grid, block, 0, stream,
                       logits, offsets, scores, top_val, top_idx, ncls, k, softmax, mean);
  return (int)hipGetLastError();
}

}  // extern "C"
