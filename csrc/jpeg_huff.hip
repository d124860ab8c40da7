// Huffman decode of MJPEG scans on the GPU: packed scan records
// (rnb_jpeg_pack_scans; layout in jpeg_huff.h) -> the frame records that
// jpeg_idct_kernel (jpeg_ops.hip) reads.
//
//  * rnb_jpeg_huff   one workgroup of 64 lanes per frame. The workgroup checks
//                    the record's header, builds the six canonical tables in
//                    LDS (lane k builds table k with the host's build_huff) and
//                    copies qt; lane i then decodes restart intervals i,
//                    i + 64, ... with decode_record_interval, the loop the
//                    host decoder runs (jpeg_huff.h), straight into the frame
//                    record. A restart interval byte-aligns the stream and
//                    resets the DC predictors, so intervals are independent;
//                    a stream without DRI is one interval, i.e. one lane, per
//                    frame.
//  * rnb_jpeg_huff_subseq  the same records and status from one workgroup of
//                    256 lanes per frame, which decodes a frame of ONE interval
//                    by synchronised subsequences (jpeg_huff_subseq_kernel
//                    below; the passes are in jpeg_huff.h) and every other
//                    frame as above.
//  * rnb_jpeg_huff_s / rnb_jpeg_huff_subseq_s  the same for 4:2:0, 4:2:2 and
//                    4:4:4 records (sampling 0 / 1 / 2): the kernels are
//                    instantiated per MCU geometry (jpeg_huff.h: Geo), which
//                    comes from the launcher's argument; a scan record whose
//                    sampling word is another one is refused (E_SCANREC).
//
// Addresses and trip counts: every block address is a function of (interval,
// MCU, block) and the launcher's geometry (mcu_block); every byte read is
// checked against the lane's span, the span against scan_len, and scan_len and
// the span table against the record's extent (scan_record_check), which the
// kernel checks against the buffer. A block takes at most 64 symbols, an MCU
// B <= 6 blocks, an interval mcus_per_interval MCUs. Corrupt data gives a code in
// status[frame] and zeroed blocks, never another address or a long loop.
//
// Every block of every frame record is written (zeroed, then filled), and
// status[frame] is 0 or the code of the lowest-numbered failing interval
// (E_SCANREC / E_HUFFMAN when the record or a table is refused as a whole: all
// blocks are zero then): a minimum over (interval, code) keys, so it does not
// depend on the order the lanes finish in.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_huff.h"

using namespace jpeg_huff;

#define JPEG_HUFF_LANES 64

struct JpegHuffArgs {
  long long scans_len;
  long long record_bytes;
  int mw, mh;
};

template <int SAMPLING>
static __device__ __forceinline__ Geo kernel_geo() {
  constexpr int hs = SAMPLING == SAMPLING_444 ? 1 : 2, vs = SAMPLING == SAMPLING_420 ? 2 : 1;
  Geo g = {hs, vs, hs * vs + 2};
  return g;
}

template <int SAMPLING>
__global__ __launch_bounds__(JPEG_HUFF_LANES) void jpeg_huff_kernel(
    const uint8_t* __restrict__ scans, const long long* __restrict__ scan_offs,
    uint8_t* __restrict__ records, int* __restrict__ status, JpegHuffArgs a) {
  __shared__ Huff tabs[6];
  __shared__ int table_rc;
  __shared__ unsigned first_bad;       // min over (interval << 5) | -code
  const int t = (int)threadIdx.x;
  const long long frame = blockIdx.x;
  const long long nmcu = (long long)a.mw * a.mh;
  const Geo geo = kernel_geo<SAMPLING>();
  uint8_t* dst = records + frame * a.record_bytes;
  int16_t* coef = (int16_t*)(dst + 384);
  // the record's extent, from the device copy of the offset table: checked
  // again here, the launcher saw the host copy
  const long long o0 = scan_offs[frame], o1 = scan_offs[frame + 1];
  const bool inside = o0 >= 0 && (o0 & 15) == 0 && o1 <= a.scans_len && o1 - o0 >= SR_SPANS + 8;
  const uint8_t* rec = scans + (inside ? o0 : 0);
  ScanHeader h = {0u, 0u, 0u};
  const int head_rc = inside ? scan_record_check(rec, o1 - o0, nmcu, h, SAMPLING) : (int)E_SCANREC;
  if (t == 0) {
    table_rc = E_OK;
    first_bad = 0xFFFFFFFFu;
  }
  __syncthreads();
  if (t < 24)                           // qt: 384 bytes, 16 per lane
    ((uint4*)dst)[t] = inside ? ((const uint4*)rec)[t] : make_uint4(0u, 0u, 0u, 0u);
  if (head_rc == E_OK && t < 6) {
    const uint8_t* tb = rec + SR_HUFF + SR_TABLE * t;
    int total = 0;
    for (int l = 0; l < 16; ++l) total += tb[l];
    tabs[t].set = 0;
    const int rc = build_huff(tb, tb + 16, total, tabs[t]);
    if (rc) table_rc = rc;              // E_HUFFMAN is the only code build_huff gives
  }
  __syncthreads();
  const int frame_rc = head_rc ? head_rc : table_rc;
  if (frame_rc) {
    for (long long i = t; i < 8 * geo.nb * nmcu; i += JPEG_HUFF_LANES)     // 128 B nmcu bytes
      ((uint4*)coef)[i] = make_uint4(0u, 0u, 0u, 0u);
    if (t == 0) status[frame] = frame_rc;
    return;
  }
  Tables tb;
  for (int c = 0; c < 3; ++c) {
    tb.dc[c] = &tabs[2 * c];
    tb.ac[c] = &tabs[2 * c + 1];
  }
  bool failed = false;
  for (long long i = t; i < (long long)h.n_intervals; i += JPEG_HUFF_LANES) {
    const int rc = decode_record_interval(rec, h, i, tb, a.mw, nmcu, coef, geo);
    if (rc && !failed) {              // a lane's intervals ascend: its first failure is its lowest
      failed = true;
      atomicMin(&first_bad, ((unsigned)i << 5) | (unsigned)(-rc));
    }
  }
  __syncthreads();
  if (t == 0) status[frame] = first_bad == 0xFFFFFFFFu ? 0 : -(int)(first_bad & 31u);
}

// One workgroup of JPEG_SUBSEQ_LANES lanes per frame. Header check, tables,
// qt and the refusals as in jpeg_huff_kernel. A frame that subseq_plan accepts
// (one interval, more than one subsequence) is decoded by synchronised
// subsequences with the passes of jpeg_huff.h: lane t owns subsequences t,
// t + LANES, ... (at most SUBSEQ_CAP / LANES of them, one bit each in `dirty`),
// the per-subsequence state lives in LDS, and every barrier is reached by the
// whole workgroup: n_sub and the "an entry changed" flag are read from LDS
// behind a barrier, so the round loop's trip count is uniform. Every other
// frame goes lane per interval through decode_record_interval, as before.
// Bounds: a subsequence is scanned in at most 8 S iterations, at most
// n_sub - 1 rounds run, the write pass stops at block B nmcu or its first
// error; every block address comes from mcu_block with a block index below
// B nmcu, every byte read lies inside the span.
template <int LANES, int SAMPLING>
__global__ __launch_bounds__(LANES) void jpeg_huff_subseq_kernel(
    const uint8_t* __restrict__ scans, const long long* __restrict__ scan_offs,
    uint8_t* __restrict__ records, int* __restrict__ status, int* __restrict__ rounds,
    JpegHuffArgs a, int subseq_bytes) {
  static_assert(SUBSEQ_CAP / LANES <= 32, "one dirty bit per owned subsequence");
  __shared__ Huff tabs[6];
  __shared__ int table_rc;
  __shared__ unsigned first_bad;              // min over (interval or subsequence << 5) | -code
  __shared__ unsigned span_end;               // the first marker inside the span
  __shared__ int changed[2];
  __shared__ long long bad_block;
  __shared__ uint32_t s_bits[SUBSEQ_CAP + 1]; // data bytes, then the boundary's bit position
  __shared__ uint16_t s_entry[SUBSEQ_CAP], s_exit[SUBSEQ_CAP];
  __shared__ uint32_t s_blocks[SUBSEQ_CAP];   // blocks completed, then the entry's block index
  __shared__ int s_dc[3][SUBSEQ_CAP];         // DC difference sums, then the entry's predictors
  const int t = (int)threadIdx.x;
  const long long frame = blockIdx.x;
  const long long nmcu = (long long)a.mw * a.mh;
  const Geo geo = kernel_geo<SAMPLING>();
  uint8_t* dst = records + frame * a.record_bytes;
  int16_t* coef = (int16_t*)(dst + 384);
  const long long o0 = scan_offs[frame], o1 = scan_offs[frame + 1];
  const bool inside = o0 >= 0 && (o0 & 15) == 0 && o1 <= a.scans_len && o1 - o0 >= SR_SPANS + 8;
  const uint8_t* rec = scans + (inside ? o0 : 0);
  ScanHeader h = {0u, 0u, 0u};
  const int head_rc = inside ? scan_record_check(rec, o1 - o0, nmcu, h, SAMPLING) : (int)E_SCANREC;
  SubseqPlan pl;
  const bool split = head_rc == E_OK && subseq_plan(rec, h, subseq_bytes, pl);
  if (t == 0) {
    table_rc = E_OK;
    first_bad = 0xFFFFFFFFu;
    span_end = split ? (unsigned)pl.end : 0u;
    changed[0] = changed[1] = 0;
    bad_block = geo.nb * nmcu;
  }
  __syncthreads();
  if (t < 24)                           // qt: 384 bytes, 16 per lane
    ((uint4*)dst)[t] = inside ? ((const uint4*)rec)[t] : make_uint4(0u, 0u, 0u, 0u);
  if (head_rc == E_OK && t < 6) {
    const uint8_t* tb = rec + SR_HUFF + SR_TABLE * t;
    int total = 0;
    for (int l = 0; l < 16; ++l) total += tb[l];
    tabs[t].set = 0;
    const int rc = build_huff(tb, tb + 16, total, tabs[t]);
    if (rc) table_rc = rc;
  }
  __syncthreads();
  const int frame_rc = head_rc ? head_rc : table_rc;
  if (frame_rc || split) {              // refused: all zero; split: zero, then only non-zeros
    for (long long i = t; i < 8 * geo.nb * nmcu; i += LANES)
      ((uint4*)coef)[i] = make_uint4(0u, 0u, 0u, 0u);
  }
  if (frame_rc) {
    if (t == 0) {
      status[frame] = frame_rc;
      rounds[frame] = 0;
    }
    return;
  }
  if (!split) {
    Tables tb;
    for (int c = 0; c < 3; ++c) {
      tb.dc[c] = &tabs[2 * c];
      tb.ac[c] = &tabs[2 * c + 1];
    }
    bool failed = false;
    for (long long i = t; i < (long long)h.n_intervals; i += LANES) {
      const int rc = decode_record_interval(rec, h, i, tb, a.mw, nmcu, coef, geo);
      if (rc && !failed) {
        failed = true;
        atomicMin(&first_bad, ((unsigned)i << 5) | (unsigned)(-rc));
      }
    }
    __syncthreads();
    if (t == 0) {
      status[frame] = first_bad == 0xFFFFFFFFu ? 0 : -(int)(first_bad & 31u);
      rounds[frame] = 0;
    }
    return;
  }
  const uint8_t* scan = rec + SR_SPANS + 8;
  // pre-pass: data bytes per subsequence; the first marker ends the span
  for (int i = t; i < pl.n_sub; i += LANES) {
    const long long b0 = pl.begin + i * pl.S;
    uint32_t cnt;
    const long long at = subseq_count(scan, pl.begin, pl.end, b0,
                                      b0 + pl.S < pl.end ? b0 + pl.S : pl.end, cnt);
    s_bits[i] = cnt;
    if (at < pl.end) atomicMin(&span_end, (unsigned)at);
  }
  __syncthreads();
  const long long end = span_end;
  const int n_sub = end > pl.begin ? (int)((end - pl.begin + pl.S - 1) / pl.S) : 1;
  // guess pass
  for (int i = t; i < n_sub; i += LANES) {
    SubseqExit x;
    subseq_scan(scan, subseq_start(scan, pl.begin, pl.begin + i * pl.S), end, (int)(8u * s_bits[i]),
                tabs, 0u, x, geo);
    s_entry[i] = 0;
    s_exit[i] = (uint16_t)x.state;
    s_blocks[i] = x.blocks;
    s_dc[0][i] = x.dc0; s_dc[1][i] = x.dc1; s_dc[2][i] = x.dc2;
  }
  __syncthreads();
  // synchronisation rounds
  int nrounds = 0;
  for (int r = 0; r < n_sub - 1; ++r) {
    unsigned dirty = 0;
    int q = 0;
    for (int i = t; i < n_sub; i += LANES, ++q) {
      if (i > 0 && s_exit[i - 1] != s_entry[i]) {
        s_entry[i] = s_exit[i - 1];
        dirty |= 1u << q;
      }
    }
    if (dirty) changed[r & 1] = 1;
    __syncthreads();
    const int any = changed[r & 1];
    if (t == 0) changed[(r + 1) & 1] = 0;
    if (!any) break;                    // uniform: read from LDS behind the barrier
    ++nrounds;
    q = 0;
    for (int i = t; i < n_sub; i += LANES, ++q) {
      if (dirty >> q & 1u) {
        SubseqExit x;
        subseq_scan(scan, subseq_start(scan, pl.begin, pl.begin + i * pl.S), end,
                    (int)(8u * s_bits[i]), tabs, s_entry[i], x, geo);
        s_exit[i] = (uint16_t)x.state;
        s_blocks[i] = x.blocks;
        s_dc[0][i] = x.dc0; s_dc[1][i] = x.dc1; s_dc[2][i] = x.dc2;
      }
    }
    __syncthreads();
  }
  // exclusive prefix sums, one array per lane: bit positions, block indices, predictors
  if (t == 0) {
    uint32_t at = 0;
    for (int i = 0; i < n_sub; ++i) {
      const uint32_t nb = 8u * s_bits[i];
      s_bits[i] = at;
      at += nb;
    }
    s_bits[n_sub] = at;
  } else if (t == 1) {
    uint32_t g = 0;
    for (int i = 0; i < n_sub; ++i) {
      const uint32_t nb = s_blocks[i];
      s_blocks[i] = g;
      g += nb;
    }
  } else if (t < 5) {
    long long d = 0;
    for (int i = 0; i < n_sub; ++i) {
      const int v = s_dc[t - 2][i];
      s_dc[t - 2][i] = subseq_clamp_pred(d);
      d += v;
    }
  }
  __syncthreads();
  // write pass; the lowest subsequence that fails holds the serial decoder's first error
  int my_sub = -1;
  long long my_bad = 0;
  for (int i = t; i < n_sub; i += LANES) {
    const long long g = s_blocks[i];
    if (g >= geo.nb * nmcu) break;
    const int rc = subseq_write(scan, subseq_start(scan, pl.begin, pl.begin + i * pl.S), end,
                                (int)(s_bits[i + 1] - s_bits[i]), i == n_sub - 1,
                                (long long)s_bits[n_sub] - s_bits[i], tabs, s_entry[i], g,
                                s_dc[0][i], s_dc[1][i], s_dc[2][i], a.mw, nmcu, coef, my_bad,
                                geo);
    if (rc) {
      my_sub = i;
      atomicMin(&first_bad, ((unsigned)i << 5) | (unsigned)(-rc));
      break;
    }
  }
  __syncthreads();
  const unsigned bad = first_bad;
  if (bad != 0xFFFFFFFFu && (int)(bad >> 5) == my_sub) bad_block = my_bad;
  __syncthreads();
  for (long long g = bad_block + t; g < geo.nb * nmcu; g += LANES)
    zero_block(mcu_block(coef, g / geo.nb, (int)(g % geo.nb), a.mw, nmcu, geo));
  if (t == 0) {
    status[frame] = bad == 0xFFFFFFFFu ? 0 : -(int)(bad & 31u);
    rounds[frame] = nrounds;
  }
}

#define JPEG_SUBSEQ_LANES 256

// the launchers' checks: 1: nothing to do; 0: launch; -2 / -4 as documented below
static int jpeg_huff_checks(const void* scans, long long scans_len,
                            const long long* scan_offs_host, const void* scan_offs_dev,
                            int nframes, int mw, int mh, void* records, long long rec_len,
                            long long record_bytes, void* status, int sampling) {
  Geo geo;
  if (!geo_of(sampling, geo)) return -2;
  if (nframes == 0) return 1;
  if (nframes < 0 || mw < 1 || mh < 1 || mw > 4096 || mh > 4096) return -2;
  if (!scans || !scan_offs_host || !scan_offs_dev || !records || !status) return -2;
  const long long n = (long long)mw * mh;
  if (((uintptr_t)scans & 15u) != 0 || ((uintptr_t)records & 15u) != 0 ||
      ((uintptr_t)scan_offs_dev & 7u) != 0 || ((uintptr_t)status & 3u) != 0 ||
      record_bytes % 16 != 0)
    return -2;
  if (record_bytes < 384 + 128 * geo.nb * n) return -4;
  if (rec_len < 0 || scans_len < 0 || record_bytes > rec_len / nframes) return -4;
  if (scan_offs_host[0] < 0 || scan_offs_host[nframes] > scans_len) return -4;
  for (int i = 0; i < nframes; ++i) {
    if (scan_offs_host[i] % 16 != 0) return -2;
    if (scan_offs_host[i + 1] - scan_offs_host[i] < SR_SPANS + 8) return -4;
  }
  return 0;
}

static int jpeg_huff_launch(const void* scans, long long scans_len,
                            const long long* scan_offs_host, const void* scan_offs_dev,
                            int nframes, int mw, int mh, void* records, long long rec_len,
                            long long record_bytes, void* status, int sampling,
                            hipStream_t stream) {
  const int rc = jpeg_huff_checks(scans, scans_len, scan_offs_host, scan_offs_dev, nframes, mw, mh,
                                  records, rec_len, record_bytes, status, sampling);
  if (rc) return rc > 0 ? 0 : rc;
  JpegHuffArgs a;
  a.scans_len = scans_len;
  a.record_bytes = record_bytes;
  a.mw = mw;
  a.mh = mh;
  auto kernel = sampling == SAMPLING_420 ? jpeg_huff_kernel<SAMPLING_420>
                : sampling == SAMPLING_422 ? jpeg_huff_kernel<SAMPLING_422>
                                           : jpeg_huff_kernel<SAMPLING_444>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nframes), dim3(JPEG_HUFF_LANES), 0, stream,
                     (const uint8_t*)scans, (const long long*)scan_offs_dev, (uint8_t*)records,
                     (int*)status, a);
  return (int)hipGetLastError();
}

static int jpeg_huff_subseq_launch(const void* scans, long long scans_len,
                                   const long long* scan_offs_host, const void* scan_offs_dev,
                                   int nframes, int mw, int mh, void* records, long long rec_len,
                                   long long record_bytes, void* status, int subseq_bytes,
                                   void* rounds, int sampling, hipStream_t stream) {
  const int rc = jpeg_huff_checks(scans, scans_len, scan_offs_host, scan_offs_dev, nframes, mw, mh,
                                  records, rec_len, record_bytes, status, sampling);
  if (rc < 0) return rc;
  if (!subseq_bytes_ok(subseq_bytes)) return -2;
  if (rc > 0) return 0;
  if (!rounds || ((uintptr_t)rounds & 3u) != 0) return -2;
  JpegHuffArgs a;
  a.scans_len = scans_len;
  a.record_bytes = record_bytes;
  a.mw = mw;
  a.mh = mh;
  auto kernel = sampling == SAMPLING_420
                    ? jpeg_huff_subseq_kernel<JPEG_SUBSEQ_LANES, SAMPLING_420>
                    : sampling == SAMPLING_422
                          ? jpeg_huff_subseq_kernel<JPEG_SUBSEQ_LANES, SAMPLING_422>
                          : jpeg_huff_subseq_kernel<JPEG_SUBSEQ_LANES, SAMPLING_444>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nframes), dim3(JPEG_SUBSEQ_LANES), 0, stream,
                     (const uint8_t*)scans, (const long long*)scan_offs_dev, (uint8_t*)records,
                     (int*)status, (int*)rounds, a, subseq_bytes);
  return (int)hipGetLastError();
}

extern "C" {

// scans: scans_len bytes of scan records on the device; scan_offs_host /
// scan_offs_dev: the same nframes + 1 byte offsets into scans (record i is
// [offs[i], offs[i + 1])), on the host for the checks below and on the device
// for the kernel, which checks its copy again. records: rec_len bytes,
// receives nframes frame records record_bytes apart; status: nframes ints.
// -2: bad shape, pointer or alignment; -4: a scan record, the room for its
// span table or a frame record would reach outside its buffer. Nothing is
// launched then.
int rnb_jpeg_huff(const void* scans, long long scans_len, const long long* scan_offs_host,
                  const void* scan_offs_dev, int nframes, int mw, int mh, void* records,
                  long long rec_len, long long record_bytes, void* status, hipStream_t stream) {
  return jpeg_huff_launch(scans, scans_len, scan_offs_host, scan_offs_dev, nframes, mw, mh,
                          records, rec_len, record_bytes, status, SAMPLING_420, stream);
}

// The same for records of `sampling` (0 4:2:0, 1 4:2:2, 2 4:4:4; -2 otherwise):
// (mw, mh) count its MCUs and a frame record is >= 384 + 128 B mw mh bytes.
int rnb_jpeg_huff_s(const void* scans, long long scans_len, const long long* scan_offs_host,
                    const void* scan_offs_dev, int nframes, int mw, int mh, void* records,
                    long long rec_len, long long record_bytes, void* status, int sampling,
                    hipStream_t stream) {
  return jpeg_huff_launch(scans, scans_len, scan_offs_host, scan_offs_dev, nframes, mw, mh,
                          records, rec_len, record_bytes, status, sampling, stream);
}

// As rnb_jpeg_huff, with frames of one interval decoded by synchronised
// subsequences of subseq_bytes raw scan bytes (a multiple of 16 in 16..4096;
// jpeg_huff_subseq_kernel). rounds: nframes ints on the device, receive the
// synchronisation rounds each frame took (0 for a frame decoded lane per
// interval). Records and status are rnb_jpeg_huff's byte for byte. -2 also for
// a bad subseq_bytes or rounds pointer; nothing is launched then.
int rnb_jpeg_huff_subseq(const void* scans, long long scans_len, const long long* scan_offs_host,
                         const void* scan_offs_dev, int nframes, int mw, int mh, void* records,
                         long long rec_len, long long record_bytes, void* status,
                         int subseq_bytes, void* rounds, hipStream_t stream) {
  return jpeg_huff_subseq_launch(scans, scans_len, scan_offs_host, scan_offs_dev, nframes, mw, mh,
                                 records, rec_len, record_bytes, status, subseq_bytes, rounds,
                                 SAMPLING_420, stream);
}

// The same for records of `sampling`, as rnb_jpeg_huff_s.
int rnb_jpeg_huff_subseq_s(const void* scans, long long scans_len,
                           const long long* scan_offs_host, const void* scan_offs_dev,
                           int nframes, int mw, int mh, void* records, long long rec_len,
                           long long record_bytes, void* status, int subseq_bytes, void* rounds,
                           int sampling, hipStream_t stream) {
  return jpeg_huff_subseq_launch(scans, scans_len, scan_offs_host, scan_offs_dev, nframes, mw, mh,
                                 records, rec_len, record_bytes, status, subseq_bytes, rounds,
                                 sampling, stream);
}

}  // extern "C"
