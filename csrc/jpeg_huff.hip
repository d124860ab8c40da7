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
//
// Addresses and trip counts: every block address is a function of (interval,
// MCU, block) and the launcher's geometry (mcu_block); every byte read is
// checked against the lane's span, the span against scan_len, and scan_len and
// the span table against the record's extent (scan_record_check), which the
// kernel checks against the buffer. A block takes at most 64 symbols, an MCU 6
// blocks, an interval mcus_per_interval MCUs. Corrupt data gives a code in
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

__global__ __launch_bounds__(JPEG_HUFF_LANES) void jpeg_huff_kernel(
    const uint8_t* __restrict__ scans, const long long* __restrict__ scan_offs,
    uint8_t* __restrict__ records, int* __restrict__ status, JpegHuffArgs a) {
  __shared__ Huff tabs[6];
  __shared__ int table_rc;
  __shared__ unsigned first_bad;       // min over (interval << 5) | -code
  const int t = (int)threadIdx.x;
  const long long frame = blockIdx.x;
  const long long nmcu = (long long)a.mw * a.mh;
  uint8_t* dst = records + frame * a.record_bytes;
  int16_t* coef = (int16_t*)(dst + 384);
  // the record's extent, from the device copy of the offset table: checked
  // again here, the launcher saw the host copy
  const long long o0 = scan_offs[frame], o1 = scan_offs[frame + 1];
  const bool inside = o0 >= 0 && (o0 & 15) == 0 && o1 <= a.scans_len && o1 - o0 >= SR_SPANS + 8;
  const uint8_t* rec = scans + (inside ? o0 : 0);
  ScanHeader h = {0u, 0u, 0u};
  const int head_rc = inside ? scan_record_check(rec, o1 - o0, nmcu, h) : (int)E_SCANREC;
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
    for (long long i = t; i < 48 * nmcu; i += JPEG_HUFF_LANES)     // 768 nmcu bytes
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
    const int rc = decode_record_interval(rec, h, i, tb, a.mw, nmcu, coef);
    if (rc && !failed) {                // a lane's intervals ascend: its first failure is its lowest
      failed = true;
      atomicMin(&first_bad, ((unsigned)i << 5) | (unsigned)(-rc));
    }
  }
  __syncthreads();
  if (t == 0) status[frame] = first_bad == 0xFFFFFFFFu ? 0 : -(int)(first_bad & 31u);
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
  if (nframes == 0) return 0;
  if (nframes < 0 || mw < 1 || mh < 1 || mw > 4096 || mh > 4096) return -2;
  if (!scans || !scan_offs_host || !scan_offs_dev || !records || !status) return -2;
  const long long n = (long long)mw * mh;
  if (((uintptr_t)scans & 15u) != 0 || ((uintptr_t)records & 15u) != 0 ||
      ((uintptr_t)scan_offs_dev & 7u) != 0 || ((uintptr_t)status & 3u) != 0 ||
      record_bytes % 16 != 0)
    return -2;
  if (record_bytes < 384 + 768 * n) return -4;
  if (rec_len < 0 || scans_len < 0 || record_bytes > rec_len / nframes) return -4;
  if (scan_offs_host[0] < 0 || scan_offs_host[nframes] > scans_len) return -4;
  for (int i = 0; i < nframes; ++i) {
    if (scan_offs_host[i] % 16 != 0) return -2;
    if (scan_offs_host[i + 1] - scan_offs_host[i] < SR_SPANS + 8) return -4;
  }
  JpegHuffArgs a;
  a.scans_len = scans_len;
  a.record_bytes = record_bytes;
  a.mw = mw;
  a.mh = mh;
  hipLaunchKernelGGL(jpeg_huff_kernel, dim3((unsigned)nframes), dim3(JPEG_HUFF_LANES), 0, stream,
                     (const uint8_t*)scans, (const long long*)scan_offs_dev, (uint8_t*)records,
                     (int*)status, a);
  return (int)hipGetLastError();
}

}  // extern "C"
