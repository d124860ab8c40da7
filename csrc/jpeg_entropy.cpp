// Host entropy decoder for Motion-JPEG streams (librnb_jpeg.so).
//
// The serial, bit-level half of the MJPEG decode backend: it walks a stream of
// concatenated JPEG frames and Huffman-decodes sampled frames into "frame
// records" of quantised coefficients, which the GPU (jpeg_idct_kernel in
// jpeg_ops.hip) dequantises and transforms. Plain C++17 behind a C ABI: no HIP,
// no PyTorch, loads on a machine without a GPU. The decode loop itself lives in
// jpeg_huff.h, shared with the GPU kernel (jpeg_huff.hip); for that kernel this
// file also packs scans into scan records (rnb_jpeg_pack_scans) and mirrors the
// kernel on the host (rnb_jpeg_decode_scans_host).
//
// Read: baseline sequential Huffman (SOF0), 8-bit samples, three components
// sampled 2x2 / 1x1 / 1x1 (4:2:0), 2x1 / 1x1 / 1x1 (4:2:2) or 1x1 / 1x1 / 1x1
// (4:4:4) in one interleaved scan, all frames of a stream alike, up to 4 + 4 Huffman
// tables and 4 8-bit quantisation tables redefined per frame, restart
// intervals, any size >= 1x1. Everything else is refused with its own code
// (rnb_jpeg_error_name).
//
// Frame record (the upload format), record_bytes >= 384 + 128 * B * mw * mh
// with luma factors Hs x Vs (jpeg_huff.h: Geo), B = Hs Vs + 2,
// mw = ceil(W / (8 Hs)), mh = ceil(H / (8 Vs)); 4:2:0: 384 + 768 * mw * mh:
//   uint16 qt[3][64]   the quantisation table of Y, Cb, Cr, natural order
//   int16  blocks[][64] QUANTISED coefficients in natural order: the Y blocks
//                      row-major over the padded Vs*mh x Hs*mw grid, then the
//                      mh x mw Cb blocks, then the Cr blocks
//
// The entry points without a sampling argument are the 4:2:0 forms: they refuse
// a 4:2:2 or 4:4:4 frame with E_SAMPLING. The *_s forms take or report the
// sampling (0 4:2:0, 1 4:2:2, 2 4:4:4); there a frame whose sampling is not the
// stream's gets E_SAMPLING_CHANGE.
//
// The input is untrusted: every read is checked against the frame's length
// and every write lands inside the record by construction (block indices come
// from the validated geometry, coefficient indices are checked against 63).
// A DC predictor that leaves the int16 range is an error (dc_range), not a
// saturation: no baseline encoder produces one.
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "jpeg_huff.h"

using namespace jpeg_huff;   // codes, tables, bit reader, decode_block / decode_interval

namespace {

struct Frame {
  int w = 0, h = 0;
  int sampling = SAMPLING_420;
  int tq[3], td[3], ta[3];
  int restart = 0;
  bool qset[4] = {false, false, false, false};
  uint16_t qt[4][64];
  Huff dc[4], ac[4];           // built with TABLES_BUILD
  bool rawset[2][4];           // [class][id]: the DHT segment as it stands, for the packer
  uint8_t raw[2][4][SR_TABLE]; // 16 counts + values, zero padded
  long long scan_begin = 0;   // first entropy-coded byte
  long long scan_end = 0;     // the FF of the marker that ends the scan
  long long frame_end = 0;    // one past EOI
  Frame() {
    for (int i = 0; i < 4; ++i) {
      dc[i].set = ac[i].set = 0;
      rawset[0][i] = rawset[1][i] = false;
    }
  }
};

// what parse_frame does with a DHT segment: nothing (the index), build the
// decode tables (the host decoder), or keep the segment's bytes (the packer,
// which does no Huffman work); the scan's tables must exist in the latter two
enum { TABLES_NONE = 0, TABLES_BUILD = 1, TABLES_RAW = 2 };

inline int rd16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Parse one frame that starts at p[0] (SOI); n bytes are readable. Walks the
// marker segments by their lengths and the scan up to EOI.
int parse_frame(const uint8_t* p, long long n, Frame& f, int tables) {
  if (n < 4) return n < 2 || (p[0] == 0xFF && p[1] == 0xD8) ? E_TRUNCATED : E_SOI;
  if (p[0] != 0xFF || p[1] != 0xD8) return E_SOI;
  long long pos = 2;
  bool have_sof = false, have_sos = false;
  int comp_id[3] = {0, 0, 0};
  for (;;) {
    if (pos + 2 > n) return have_sos ? E_EOI : E_TRUNCATED;
    if (p[pos] != 0xFF) return E_MARKER;
    int m = p[pos + 1];
    if (m == 0xFF) { pos += 1; continue; }             // fill byte
    pos += 2;
    if (m == 0xD9) {                                   // EOI
      if (!have_sos) return E_MARKER;
      f.frame_end = pos;
      return E_OK;
    }
    if (m == 0xD8 || m == 0x00 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) return E_MARKER;
    if (pos + 2 > n) return E_TRUNCATED;
    const int len = rd16(p + pos);
    if (len < 2) return E_MARKER;
    if (pos + len > n) return E_TRUNCATED;
    const uint8_t* s = p + pos + 2;
    const int body = len - 2;
    if (m == 0xC0) {                                   // SOF0
      if (have_sof) return E_MARKER;
      if (body < 6) return E_MARKER;
      if (s[0] != 8) return E_PRECISION;
      f.h = rd16(s + 1);
      f.w = rd16(s + 3);
      if (f.w == 0 || f.h == 0) return E_SIZE;
      if (s[5] != 3) return E_COMPONENTS;
      if (body != 6 + 3 * 3) return E_MARKER;
      for (int c = 0; c < 3; ++c) {
        comp_id[c] = s[6 + 3 * c];
        const int hv = s[7 + 3 * c];
        if (c == 0) {
          if (hv != 0x22 && hv != 0x21 && hv != 0x11) return E_SAMPLING;
          f.sampling = hv == 0x22 ? SAMPLING_420 : hv == 0x21 ? SAMPLING_422 : SAMPLING_444;
        } else if (hv != 0x11) {
          return E_SAMPLING;
        }
        f.tq[c] = s[8 + 3 * c];
        if (f.tq[c] > 3) return E_MARKER;
      }
      have_sof = true;
    } else if (m == 0xC4) {                            // DHT
      int o = 0;
      while (o < body) {
        if (o + 17 > body) return E_MARKER;
        const int tc = s[o] >> 4, th = s[o] & 15;
        if (tc > 1 || th > 3) return E_MARKER;
        uint8_t bits[17];
        int total = 0;
        bits[0] = 0;
        for (int l = 1; l <= 16; ++l) total += (bits[l] = s[o + l]);
        if (total > 256 || o + 17 + total > body) return E_MARKER;
        if (tables == TABLES_BUILD) {
          const int rc = build_huff(bits + 1, s + o + 17, total, tc ? f.ac[th] : f.dc[th]);
          if (rc) return rc;
        } else if (tables == TABLES_RAW) {
          uint8_t* r = f.raw[tc][th];
          memset(r, 0, SR_TABLE);
          memcpy(r, bits + 1, 16);
          memcpy(r + 16, s + o + 17, (size_t)total);
          f.rawset[tc][th] = true;
        }
        o += 17 + total;
      }
    } else if (m == 0xDB) {                            // DQT
      int o = 0;
      while (o < body) {
        const int pq = s[o] >> 4, tq = s[o] & 15;
        if (pq == 1) return E_QT16;
        if (pq > 1 || tq > 3) return E_MARKER;
        if (o + 65 > body) return E_MARKER;
        for (int k = 0; k < 64; ++k) f.qt[tq][kZigzag[k]] = s[o + 1 + k];
        f.qset[tq] = true;
        o += 65;
      }
    } else if (m == 0xDD) {                            // DRI
      if (body != 2) return E_MARKER;
      f.restart = rd16(s);
    } else if (m == 0xCC) {                            // DAC
      return E_ARITHMETIC;
    } else if (m >= 0xC1 && m <= 0xCF && m != 0xC8) {  // every other SOF
      return (m >= 0xC9) ? E_ARITHMETIC : E_SOF;
    } else if (m == 0xDA) {                            // SOS
      if (!have_sof) return E_MARKER;
      if (have_sos) return E_MULTISCAN;
      if (body < 1) return E_MARKER;
      if (s[0] != 3) return E_MULTISCAN;
      if (body != 1 + 2 * 3 + 3) return E_MARKER;
      for (int c = 0; c < 3; ++c) {
        if (s[1 + 2 * c] != comp_id[c]) return E_MARKER;
        f.td[c] = s[2 + 2 * c] >> 4;
        f.ta[c] = s[2 + 2 * c] & 15;
        if (f.td[c] > 3 || f.ta[c] > 3) return E_MARKER;
        if (!f.qset[f.tq[c]]) return E_TABLE;
        if (tables == TABLES_BUILD && (!f.dc[f.td[c]].set || !f.ac[f.ta[c]].set)) return E_TABLE;
        if (tables == TABLES_RAW && (!f.rawset[0][f.td[c]] || !f.rawset[1][f.ta[c]]))
          return E_TABLE;
      }
      if (s[7] != 0 || s[8] != 63 || s[9] != 0) return E_MULTISCAN;   // spectral selection
      have_sos = true;
      pos += len;
      f.scan_begin = pos;
      // entropy-coded data: up to the next marker that is not FF00 / RSTn
      for (;;) {
        const uint8_t* q = (const uint8_t*)memchr(p + pos, 0xFF, (size_t)(n - pos));
        if (!q) return E_EOI;
        pos = q - p;
        if (pos + 1 >= n) return E_EOI;
        const int b = p[pos + 1];
        if (b == 0x00 || (b >= 0xD0 && b <= 0xD7)) { pos += 2; continue; }
        if (b == 0xFF) { pos += 1; continue; }
        f.scan_end = pos;
        break;                                         // a marker: handled by the outer loop
      }
      continue;
    }
    // APPn, COM and anything else with a length: skipped
    pos += len;
  }
}

// MCU grid of a w x h frame
inline void mcu_grid(int w, int h, const Geo& g, long long& mw, long long& mh) {
  mw = (w + 8 * g.hs - 1) / (8 * g.hs);
  mh = (h + 8 * g.vs - 1) / (8 * g.vs);
}

// what a frame of another (readable) sampling than `want` gets: the 4:2:0 entry
// points (legacy) keep refusing it as before
inline int sampling_mismatch(bool legacy) { return legacy ? E_SAMPLING : E_SAMPLING_CHANGE; }

// one frame -> one record; rec has room for 384 + 128 * B * mw * mh bytes.
// sampling: the one the frame must have.
int decode_frame(const uint8_t* p, long long n, int want_w, int want_h, uint8_t* rec,
                 long long record_bytes, int* dims, int sampling, bool legacy) {
  std::vector<Frame> holder(1);            // ~14 KB of tables: off the thread's stack
  Frame& f = holder[0];
  int rc = parse_frame(p, n, f, TABLES_BUILD);
  if (rc) return rc;
  if (dims) { dims[0] = f.w; dims[1] = f.h; }
  if (f.sampling != sampling) return sampling_mismatch(legacy);
  if (want_w > 0 && (f.w != want_w || f.h != want_h)) return E_SIZE_CHANGE;
  Geo g = geo_420();
  if (!geo_of(sampling, g)) return E_ARG;
  long long mw, mh;
  mcu_grid(f.w, f.h, g, mw, mh);
  if (384 + 128 * g.nb * mw * mh > record_bytes) return E_RECORD;
  uint16_t* qt = (uint16_t*)rec;
  for (int c = 0; c < 3; ++c) memcpy(qt + 64 * c, f.qt[f.tq[c]], 128);
  int16_t* coef = (int16_t*)(rec + 384);      // every block is visited and zeroed first
  Tables t;
  for (int c = 0; c < 3; ++c) {
    t.dc[c] = &f.dc[f.td[c]];
    t.ac[c] = &f.ac[f.ta[c]];
  }
  const long long nmcu = mw * mh;
  const long long per = f.restart ? f.restart : nmcu;
  long long pos = f.scan_begin;
  int next_rst = 0;
  for (long long m0 = 0; m0 < nmcu; m0 += per) {
    Bits b;
    rc = decode_interval(b, p, pos, n, t, m0, nmcu - m0 < per ? nmcu - m0 : per, mw, nmcu, coef,
                         false, g);
    if (rc) return rc;
    if (m0 + per >= nmcu) break;
    // the marker follows the byte the interval ended in
    if (!interval_ended(b)) return E_RESTART;
    if (b.pos + 1 >= b.end || p[b.pos] != 0xFF || p[b.pos + 1] != 0xD0 + next_rst)
      return E_RESTART;
    pos = b.pos + 2;
    next_rst = (next_rst + 1) & 7;
  }
  return E_OK;
}

long long mjpeg_index(const uint8_t* data, long long len, long long* offs, long long* lens,
                      long long cap, int* info, bool legacy) {
  if (!data || len < 0 || cap < 0 || (cap > 0 && (!offs || !lens)) || !info) return E_ARG;
  info[0] = info[1] = info[2] = info[3] = 0;
  if (!legacy) info[4] = 0;
  int sampling = SAMPLING_420;
  std::vector<Frame> holder(1);
  long long pos = 0, count = 0;
  while (pos < len) {
    holder[0] = Frame();
    Frame& f = holder[0];
    info[2] = (int)count;
    const int rc = parse_frame(data + pos, len - pos, f, TABLES_NONE);
    if (rc) return rc;
    if (legacy && f.sampling != SAMPLING_420) return E_SAMPLING;
    if (count == 0) {
      info[0] = f.w; info[1] = f.h; info[3] = f.restart;
      sampling = f.sampling;
      if (!legacy) info[4] = sampling;
    } else if (f.sampling != sampling) {
      return E_SAMPLING_CHANGE;
    } else if (f.w != info[0] || f.h != info[1]) {
      return E_SIZE_CHANGE;
    }
    if (count < cap) { offs[count] = pos; lens[count] = f.frame_end; }
    ++count;
    pos += f.frame_end;
  }
  return count;
}

}  // namespace

extern "C" {

const char* rnb_jpeg_error_name(int code) {
  switch (code) {
    case E_OK: return "ok";
    case E_ARG: return "argument";
    case E_TRUNCATED: return "truncated";
    case E_SOI: return "SOI";
    case E_SOF: return "SOF";
    case E_ARITHMETIC: return "arithmetic";
    case E_PRECISION: return "precision";
    case E_QT16: return "DQT precision";
    case E_COMPONENTS: return "components";
    case E_SAMPLING: return "sampling";
    case E_MULTISCAN: return "scans";
    case E_SIZE_CHANGE: return "size";
    case E_HUFFMAN: return "huffman";
    case E_RUN: return "run";
    case E_RESTART: return "RST";
    case E_MARKER: return "marker";
    case E_EOI: return "EOI";
    case E_TABLE: return "table";
    case E_RECORD: return "record";
    case E_DC_RANGE: return "dc_range";
    case E_SIZE: return "dimensions";
    case E_SCANREC: return "scan record";
    case E_SAMPLING_CHANGE: return "sampling change";
    default: return "unknown";
  }
}

// Index a concatenated JPEG stream. Writes up to `cap` frame offsets / lengths
// and returns the number of frames found (call with cap = 0 to count), or a
// negative code. info[0..3] = width, height, index of the frame the error is
// in, restart interval of the first frame. Every frame's header is parsed and
// its size compared with the first frame's.
long long rnb_mjpeg_index(const uint8_t* data, long long len, long long* offs, long long* lens,
                          long long cap, int* info) {
  return mjpeg_index(data, len, offs, lens, cap, info, true);
}

// The same for 4:2:0, 4:2:2 and 4:4:4 streams: info has a fifth word, the
// sampling of the first frame (0 / 1 / 2), which every frame must share
// (E_SAMPLING_CHANGE otherwise).
long long rnb_mjpeg_index_s(const uint8_t* data, long long len, long long* offs, long long* lens,
                            long long cap, int* info) {
  return mjpeg_index(data, len, offs, lens, cap, info, false);
}

// Entropy-decode nframes frames (data + frame_offs[i], frame_lens[i] bytes)
// into records of record_bytes each at out + i * record_bytes, on up to
// `threads` (<= 16) threads. All frames must have the first one's size.
// Returns 0, or the code of the lowest-numbered frame that failed.
static int decode_frames(const uint8_t* data, long long len, const long long* frame_offs,
                         const long long* frame_lens, int nframes, uint8_t* out,
                         long long record_bytes, int threads, int sampling, bool legacy) {
  Geo geo;
  if (!geo_of(sampling, geo)) return E_ARG;
  if (nframes == 0) return E_OK;
  if (!data || !frame_offs || !frame_lens || !out || len < 0 || nframes < 0 || threads < 1 ||
      record_bytes < 384)
    return E_ARG;
  for (int i = 0; i < nframes; ++i)
    if (frame_offs[i] < 0 || frame_lens[i] < 0 || frame_offs[i] > len ||
        frame_lens[i] > len - frame_offs[i])
      return E_ARG;
  int dims[2] = {0, 0};
  std::vector<int> codes((size_t)nframes, 0);
  codes[0] = decode_frame(data + frame_offs[0], frame_lens[0], 0, 0, out, record_bytes, dims,
                          sampling, legacy);
  if (codes[0]) return codes[0];
  if (threads > 16) threads = 16;
  if (threads > nframes - 1) threads = nframes - 1;
  std::atomic<int> next(1);
  auto work = [&]() {
    for (;;) {
      const int i = next.fetch_add(1);
      if (i >= nframes) return;
      codes[(size_t)i] = decode_frame(data + frame_offs[i], frame_lens[i], dims[0], dims[1],
                                      out + (long long)i * record_bytes, record_bytes, nullptr,
                                      sampling, legacy);
    }
  };
  if (threads <= 1) {
    work();
  } else {
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t) pool.emplace_back(work);
    for (auto& t : pool) t.join();
  }
  for (int i = 0; i < nframes; ++i)
    if (codes[(size_t)i]) return codes[(size_t)i];
  return E_OK;
}

int rnb_jpeg_decode_frames(const uint8_t* data, long long len, const long long* frame_offs,
                           const long long* frame_lens, int nframes, uint8_t* out,
                           long long record_bytes, int threads) {
  return decode_frames(data, len, frame_offs, frame_lens, nframes, out, record_bytes, threads,
                       SAMPLING_420, true);
}

// The same for frames of `sampling` (0 4:2:0, 1 4:2:2, 2 4:4:4; E_ARG otherwise),
// which is the stream's, from rnb_mjpeg_index_s: records of 384 + 128 B mw mh
// bytes. A frame of another sampling: E_SAMPLING_CHANGE.
int rnb_jpeg_decode_frames_s(const uint8_t* data, long long len, const long long* frame_offs,
                             const long long* frame_lens, int nframes, uint8_t* out,
                             long long record_bytes, int threads, int sampling) {
  return decode_frames(data, len, frame_offs, frame_lens, nframes, out, record_bytes, threads,
                       sampling, false);
}

// Pack the scans of nframes frames into scan records (layout: jpeg_huff.h) for
// the interval decoders, back to back in out[0 .. out_cap). Per frame:
// parse_frame with its refusals, then one walk over the scan for RSTn markers,
// which must number D0, D1, ... cyclically and be exactly ceil(nmcu / DRI) - 1
// (E_RESTART otherwise). No Huffman work. scan_offs receives nframes + 1 byte
// offsets into out (record i is [scan_offs[i], scan_offs[i + 1]), 16-byte
// aligned). want_w / want_h: the size every frame must have (0: the first
// frame's). info[0..2] = width, height, index of the frame a refusal is in.
// Returns the number of bytes written, or a negative code (E_RECORD: out_cap
// is too small).
static long long pack_scans(const uint8_t* data, long long len, const long long* frame_offs,
                            const long long* frame_lens, int nframes, uint8_t* out,
                            long long out_cap, long long* scan_offs, int want_w, int want_h,
                            int* info, int sampling, bool legacy) {
  Geo geo;
  if (!geo_of(sampling, geo)) return E_ARG;
  if (!data || !frame_offs || !frame_lens || !out || !scan_offs || !info || len < 0 ||
      nframes < 0 || out_cap < 0 || want_w < 0 || want_h < 0 || ((uintptr_t)out & 15u) != 0)
    return E_ARG;
  info[0] = want_w; info[1] = want_h; info[2] = 0;
  for (int i = 0; i < nframes; ++i)
    if (frame_offs[i] < 0 || frame_lens[i] < 0 || frame_offs[i] > len ||
        frame_lens[i] > len - frame_offs[i])
      return E_ARG;
  std::vector<Frame> holder(1);
  long long at = 0;
  scan_offs[0] = 0;
  for (int i = 0; i < nframes; ++i) {
    info[2] = i;
    holder[0] = Frame();
    Frame& f = holder[0];
    const uint8_t* p = data + frame_offs[i];
    const int rc = parse_frame(p, frame_lens[i], f, TABLES_RAW);
    if (rc) return rc;
    if (f.sampling != sampling) return sampling_mismatch(legacy);
    if (info[0] == 0) { info[0] = f.w; info[1] = f.h; }
    if (f.w != info[0] || f.h != info[1]) return E_SIZE_CHANGE;
    long long mw, mh;
    mcu_grid(f.w, f.h, geo, mw, mh);
    const long long nmcu = mw * mh;
    const long long per = f.restart && f.restart < nmcu ? f.restart : nmcu;
    const long long n_int = (nmcu + per - 1) / per;
    const long long scan_len = f.scan_end - f.scan_begin;
    if (scan_len < 0 || scan_len > 0x7FFFFFFFLL) return E_ARG;
    const long long size = (SR_SPANS + 8 * n_int + scan_len + 15) & ~15LL;
    if (size > out_cap - at) return E_RECORD;
    uint8_t* rec = out + at;
    for (int c = 0; c < 3; ++c) {
      memcpy(rec + 128 * c, f.qt[f.tq[c]], 128);
      memcpy(rec + SR_HUFF + SR_TABLE * (2 * c), f.raw[0][f.td[c]], SR_TABLE);
      memcpy(rec + SR_HUFF + SR_TABLE * (2 * c + 1), f.raw[1][f.ta[c]], SR_TABLE);
    }
    const uint32_t head[4] = {(uint32_t)n_int, (uint32_t)per, (uint32_t)scan_len,
                              (uint32_t)sampling};
    memcpy(rec + SR_HEADER, head, 16);
    uint8_t* spans = rec + SR_SPANS;
    const uint8_t* scan = p + f.scan_begin;
    // the bytes in front of a marker that are FF are fill bytes, not data
    auto put_span = [&](long long k, long long begin, long long end) {
      while (end > begin && scan[end - 1] == 0xFF) --end;
      const uint32_t be[2] = {(uint32_t)begin, (uint32_t)end};
      memcpy(spans + 8 * k, be, 8);
    };
    long long pos = 0, start = 0, k = 0;
    while (pos < scan_len) {
      const uint8_t* q = (const uint8_t*)memchr(scan + pos, 0xFF, (size_t)(scan_len - pos));
      if (!q) break;
      pos = q - scan;
      const int b = scan[pos + 1];          // the scan ends in front of a marker: readable
      if (b >= 0xD0 && b <= 0xD7) {
        if (b - 0xD0 != (int)(k & 7) || k + 1 >= n_int) return E_RESTART;
        put_span(k, start, pos);
        ++k;
        pos += 2;
        start = pos;
      } else {
        pos += b == 0x00 ? 2 : 1;           // stuffing / a fill byte
      }
    }
    if (k != n_int - 1) return E_RESTART;
    put_span(k, start, scan_len);
    uint8_t* body = spans + 8 * n_int;
    memcpy(body, scan, (size_t)scan_len);
    memset(body + scan_len, 0, (size_t)(size - (SR_SPANS + 8 * n_int + scan_len)));
    at += size;
    scan_offs[i + 1] = at;
  }
  return at;
}

long long rnb_jpeg_pack_scans(const uint8_t* data, long long len, const long long* frame_offs,
                              const long long* frame_lens, int nframes, uint8_t* out,
                              long long out_cap, long long* scan_offs, int want_w, int want_h,
                              int* info) {
  return pack_scans(data, len, frame_offs, frame_lens, nframes, out, out_cap, scan_offs, want_w,
                    want_h, info, SAMPLING_420, true);
}

// The same for frames of `sampling` (0 / 1 / 2, the stream's; E_ARG otherwise):
// the record's fourth header word carries it. A frame of another sampling:
// E_SAMPLING_CHANGE.
long long rnb_jpeg_pack_scans_s(const uint8_t* data, long long len, const long long* frame_offs,
                                const long long* frame_lens, int nframes, uint8_t* out,
                                long long out_cap, long long* scan_offs, int want_w, int want_h,
                                int* info, int sampling) {
  return pack_scans(data, len, frame_offs, frame_lens, nframes, out, out_cap, scan_offs, want_w,
                    want_h, info, sampling, false);
}

// The GPU interval decoder's host mirror: nframes scan records (record i at
// scans[scan_offs[i] .. scan_offs[i + 1])) into frame records record_bytes
// apart in out, with what jpeg_huff_kernel does in the same order: the tables
// are built from the record, qt is copied, every interval is decoded with
// decode_record_interval, and status[i] is 0 or the code of the frame's
// lowest-numbered failing interval (E_SCANREC / E_HUFFMAN for a record or a
// table that is refused as a whole: all blocks zero then). Every block of
// every record is written. Returns 0, or E_ARG when a buffer, an offset or an
// alignment is refused (nothing is written then).
static int decode_scans_host(const uint8_t* scans, long long scans_len,
                             const long long* scan_offs, int nframes, int mw, int mh,
                             uint8_t* out, long long out_len, long long record_bytes,
                             int* status, int sampling) {
  Geo geo;
  if (!geo_of(sampling, geo)) return E_ARG;
  const long long coef_bytes = 128LL * geo.nb;          // per MCU
  if (nframes == 0) return E_OK;
  if (!scans || !scan_offs || !out || !status || nframes < 0 || mw < 1 || mh < 1 || mw > 4096 ||
      mh > 4096 || scans_len < 0 || out_len < 0)
    return E_ARG;
  const long long nmcu = (long long)mw * mh;
  if (((uintptr_t)out & 15u) != 0 || record_bytes % 16 != 0 ||
      record_bytes < 384 + coef_bytes * nmcu ||
      record_bytes > out_len / nframes)
    return E_ARG;
  if (scan_offs[0] < 0 || scan_offs[nframes] > scans_len) return E_ARG;
  for (int i = 0; i < nframes; ++i)
    if (scan_offs[i] % 16 != 0 || scan_offs[i + 1] - scan_offs[i] < SR_SPANS + 8) return E_ARG;
  std::vector<Huff> tabs(6);
  for (int i = 0; i < nframes; ++i) {
    const uint8_t* rec = scans + scan_offs[i];
    uint8_t* dst = out + (long long)i * record_bytes;
    int16_t* coef = (int16_t*)(dst + 384);
    ScanHeader h;
    int rc = scan_record_check(rec, scan_offs[i + 1] - scan_offs[i], nmcu, h, sampling);
    memcpy(dst, rec, 384);
    Tables t;
    for (int k = 0; k < 6 && !rc; ++k) {
      const uint8_t* tb = rec + SR_HUFF + SR_TABLE * k;
      int total = 0;
      for (int l = 0; l < 16; ++l) total += tb[l];
      tabs[(size_t)k].set = 0;
      rc = build_huff(tb, tb + 16, total, tabs[(size_t)k]);
    }
    for (int c = 0; c < 3; ++c) {
      t.dc[c] = &tabs[(size_t)(2 * c)];
      t.ac[c] = &tabs[(size_t)(2 * c + 1)];
    }
    if (rc) {
      memset(coef, 0, (size_t)(coef_bytes * nmcu));
      status[i] = rc;
      continue;
    }
    status[i] = E_OK;
    for (long long v = 0; v < (long long)h.n_intervals; ++v) {
      rc = decode_record_interval(rec, h, v, t, mw, nmcu, coef, geo);
      if (rc && !status[i]) status[i] = rc;
    }
  }
  return E_OK;
}

int rnb_jpeg_decode_scans_host(const uint8_t* scans, long long scans_len,
                               const long long* scan_offs, int nframes, int mw, int mh,
                               uint8_t* out, long long out_len, long long record_bytes,
                               int* status) {
  return decode_scans_host(scans, scans_len, scan_offs, nframes, mw, mh, out, out_len,
                           record_bytes, status, SAMPLING_420);
}

// The same with the geometry of `sampling` (0 / 1 / 2; E_ARG otherwise): (mw,
// mh) count its MCUs, records are >= 384 + 128 B mw mh bytes, and a scan record
// whose sampling word is another gets E_SCANREC.
int rnb_jpeg_decode_scans_host_s(const uint8_t* scans, long long scans_len,
                                 const long long* scan_offs, int nframes, int mw, int mh,
                                 uint8_t* out, long long out_len, long long record_bytes,
                                 int* status, int sampling) {
  return decode_scans_host(scans, scans_len, scan_offs, nframes, mw, mh, out, out_len,
                           record_bytes, status, sampling);
}

// The host emulation of jpeg_huff_subseq_kernel: as rnb_jpeg_decode_scans_host,
// but a frame whose scan is one interval of more than one subsequence of
// subseq_bytes (a multiple of 16 in 16..4096; see subseq_plan) is decoded by
// synchronised subsequences, with the header functions the kernel runs, pass
// by pass, as loops over the subsequences. Records and status equal
// rnb_jpeg_decode_scans_host's byte for byte; rounds[i] receives the number of
// synchronisation rounds frame i took (0 for every other frame).
static int decode_scans_subseq_host(const uint8_t* scans, long long scans_len,
                                    const long long* scan_offs, int nframes, int mw, int mh,
                                    uint8_t* out, long long out_len, long long record_bytes,
                                    int* status, int subseq_bytes, int* rounds, int sampling) {
  Geo geo;
  if (!geo_of(sampling, geo)) return E_ARG;
  const long long coef_bytes = 128LL * geo.nb;          // per MCU
  if (!rounds || !subseq_bytes_ok(subseq_bytes)) return E_ARG;
  if (nframes == 0) return E_OK;
  if (!scans || !scan_offs || !out || !status || nframes < 0 || mw < 1 || mh < 1 || mw > 4096 ||
      mh > 4096 || scans_len < 0 || out_len < 0)
    return E_ARG;
  const long long nmcu = (long long)mw * mh;
  if (((uintptr_t)out & 15u) != 0 || record_bytes % 16 != 0 ||
      record_bytes < 384 + coef_bytes * nmcu ||
      record_bytes > out_len / nframes)
    return E_ARG;
  if (scan_offs[0] < 0 || scan_offs[nframes] > scans_len) return E_ARG;
  for (int i = 0; i < nframes; ++i)
    if (scan_offs[i] % 16 != 0 || scan_offs[i + 1] - scan_offs[i] < SR_SPANS + 8) return E_ARG;
  std::vector<Huff> tabs(6);
  std::vector<uint32_t> bits, entry, blocks;
  std::vector<SubseqExit> exits;
  std::vector<int> pred;
  std::vector<char> dirty;
  for (int i = 0; i < nframes; ++i) {
    const uint8_t* rec = scans + scan_offs[i];
    uint8_t* dst = out + (long long)i * record_bytes;
    int16_t* coef = (int16_t*)(dst + 384);
    ScanHeader h;
    int rc = scan_record_check(rec, scan_offs[i + 1] - scan_offs[i], nmcu, h, sampling);
    memcpy(dst, rec, 384);
    rounds[i] = 0;
    for (int k = 0; k < 6 && !rc; ++k) {
      const uint8_t* tb = rec + SR_HUFF + SR_TABLE * k;
      int total = 0;
      for (int l = 0; l < 16; ++l) total += tb[l];
      tabs[(size_t)k].set = 0;
      rc = build_huff(tb, tb + 16, total, tabs[(size_t)k]);
    }
    if (rc) {
      memset(coef, 0, (size_t)(coef_bytes * nmcu));
      status[i] = rc;
      continue;
    }
    status[i] = E_OK;
    SubseqPlan pl;
    if (!subseq_plan(rec, h, subseq_bytes, pl)) {
      Tables t;
      for (int c = 0; c < 3; ++c) {
        t.dc[c] = &tabs[(size_t)(2 * c)];
        t.ac[c] = &tabs[(size_t)(2 * c + 1)];
      }
      for (long long v = 0; v < (long long)h.n_intervals; ++v) {
        rc = decode_record_interval(rec, h, v, t, mw, nmcu, coef, geo);
        if (rc && !status[i]) status[i] = rc;
      }
      continue;
    }
    const uint8_t* scan = rec + SR_SPANS + 8;
    memset(coef, 0, (size_t)(coef_bytes * nmcu));
    // pre-pass: data bytes per subsequence; the first marker ends the span
    bits.assign((size_t)pl.n_sub + 1, 0u);
    long long end = pl.end;
    for (int s = 0; s < pl.n_sub; ++s) {
      const long long b0 = pl.begin + s * pl.S;
      const long long at = subseq_count(scan, pl.begin, pl.end, b0,
                                        b0 + pl.S < pl.end ? b0 + pl.S : pl.end, bits[(size_t)s]);
      if (at < end) end = at;
    }
    const int n_sub = end > pl.begin ? (int)((end - pl.begin + pl.S - 1) / pl.S) : 1;
    auto start = [&](int s) { return subseq_start(scan, pl.begin, pl.begin + s * pl.S); };
    // guess pass
    entry.assign((size_t)n_sub, 0u);
    exits.resize((size_t)n_sub);
    for (int s = 0; s < n_sub; ++s)
      subseq_scan(scan, start(s), end, (int)(8 * bits[(size_t)s]), tabs.data(), 0u,
                  exits[(size_t)s], geo);
    // synchronisation rounds
    dirty.assign((size_t)n_sub, 0);
    for (int r = 0; r < n_sub - 1; ++r) {
      bool changed = false;
      for (int s = 1; s < n_sub; ++s) {
        dirty[(size_t)s] = exits[(size_t)s - 1].state != entry[(size_t)s];
        if (dirty[(size_t)s]) {
          entry[(size_t)s] = exits[(size_t)s - 1].state;
          changed = true;
        }
      }
      if (!changed) break;
      ++rounds[i];
      for (int s = 1; s < n_sub; ++s)
        if (dirty[(size_t)s])
          subseq_scan(scan, start(s), end, (int)(8 * bits[(size_t)s]), tabs.data(),
                      entry[(size_t)s], exits[(size_t)s], geo);
    }
    // prefix sums: boundary bit positions, block indices, predictors
    blocks.assign((size_t)n_sub, 0u);
    pred.assign(3 * (size_t)n_sub, 0);
    {
      uint32_t at = 0;
      unsigned long long g = 0;
      long long d0 = 0, d1 = 0, d2 = 0;
      for (int s = 0; s < n_sub; ++s) {
        const uint32_t nb = 8 * bits[(size_t)s];
        bits[(size_t)s] = at;
        at += nb;
        blocks[(size_t)s] = (uint32_t)g;
        g += exits[(size_t)s].blocks;
        pred[3 * (size_t)s] = subseq_clamp_pred(d0);
        pred[3 * (size_t)s + 1] = subseq_clamp_pred(d1);
        pred[3 * (size_t)s + 2] = subseq_clamp_pred(d2);
        d0 += exits[(size_t)s].dc0;
        d1 += exits[(size_t)s].dc1;
        d2 += exits[(size_t)s].dc2;
        if (s + 1 < n_sub && ((entry[(size_t)s + 1] >> 6) & 7) != g % geo.nb)
          return E_ARG;
      }
      bits[(size_t)n_sub] = at;
    }
    // write pass; the lowest subsequence that fails holds the first error
    const long long total = geo.nb * nmcu;
    long long bad_block = total;
    for (int s = 0; s < n_sub; ++s) {
      if ((long long)blocks[(size_t)s] >= total) break;
      rc = subseq_write(scan, start(s), end, (int)(bits[(size_t)s + 1] - bits[(size_t)s]),
                        s == n_sub - 1, (long long)bits[(size_t)n_sub] - bits[(size_t)s],
                        tabs.data(), entry[(size_t)s], blocks[(size_t)s], pred[3 * (size_t)s],
                        pred[3 * (size_t)s + 1], pred[3 * (size_t)s + 2], mw, nmcu, coef,
                        bad_block, geo);
      if (rc) {
        status[i] = rc;
        break;
      }
    }
    for (long long g = bad_block; g < total; ++g)
      zero_block(mcu_block(coef, g / geo.nb, (int)(g % geo.nb), mw, nmcu, geo));
  }
  return E_OK;
}

int rnb_jpeg_decode_scans_subseq_host(const uint8_t* scans, long long scans_len,
                                      const long long* scan_offs, int nframes, int mw, int mh,
                                      uint8_t* out, long long out_len, long long record_bytes,
                                      int* status, int subseq_bytes, int* rounds) {
  return decode_scans_subseq_host(scans, scans_len, scan_offs, nframes, mw, mh, out, out_len,
                                  record_bytes, status, subseq_bytes, rounds, SAMPLING_420);
}

// The same with the geometry of `sampling`, as rnb_jpeg_decode_scans_host_s.
int rnb_jpeg_decode_scans_subseq_host_s(const uint8_t* scans, long long scans_len,
                                        const long long* scan_offs, int nframes, int mw, int mh,
                                        uint8_t* out, long long out_len, long long record_bytes,
                                        int* status, int subseq_bytes, int* rounds,
                                        int sampling) {
  return decode_scans_subseq_host(scans, scans_len, scan_offs, nframes, mw, mh, out, out_len,
                                  record_bytes, status, subseq_bytes, rounds, sampling);
}

}  // extern "C"
