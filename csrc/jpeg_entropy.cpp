// Host entropy decoder for Motion-JPEG streams (librnb_jpeg.so).
//
// The serial, bit-level half of the MJPEG decode backend: it walks a stream of
// concatenated JPEG frames and Huffman-decodes sampled frames into "frame
// records" of quantised coefficients, which the GPU (jpeg_idct_kernel in
// jpeg_ops.hip) dequantises and transforms. Plain C++17 behind a C ABI: no HIP,
// no PyTorch, loads on a machine without a GPU.
//
// Read: baseline sequential Huffman (SOF0), 8-bit samples, three components
// sampled 2x2 / 1x1 / 1x1 (4:2:0) in one interleaved scan, up to 4 + 4 Huffman
// tables and 4 8-bit quantisation tables redefined per frame, restart
// intervals, any size >= 1x1. Everything else is refused with its own code
// (rnb_jpeg_error_name).
//
// Frame record (the upload format), record_bytes >= 384 + 768 * mw * mh with
// mw = ceil(W / 16), mh = ceil(H / 16):
//   uint16 qt[3][64]   the quantisation table of Y, Cb, Cr, natural order
//   int16  blocks[][64] QUANTISED coefficients in natural order: the Y blocks
//                      row-major over the padded 2*mh x 2*mw grid, then the
//                      mh x mw Cb blocks, then the Cr blocks
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

namespace {

enum {
  E_OK = 0,
  E_ARG = -1,          // null pointer, negative length, bad thread / frame count
  E_TRUNCATED = -2,    // data ends inside a segment or inside the scan
  E_SOI = -3,          // frame does not start with SOI
  E_SOF = -4,          // progressive / extended / lossless frame (SOF1-3, 5-7, 9-15)
  E_ARITHMETIC = -5,   // arithmetic coding (SOF9-11, 13-15, DAC)
  E_PRECISION = -6,    // sample precision other than 8 bits
  E_QT16 = -7,         // 16-bit quantisation table
  E_COMPONENTS = -8,   // component count other than 3
  E_SAMPLING = -9,     // sampling factors other than 2x2, 1x1, 1x1
  E_MULTISCAN = -10,   // more than one scan, or a scan that is not all three components
  E_SIZE_CHANGE = -11, // frame size differs from the first frame's
  E_HUFFMAN = -12,     // a code that matches no entry / an invalid table
  E_RUN = -13,         // zero run past coefficient 63
  E_RESTART = -14,     // missing or wrong RSTn
  E_MARKER = -15,      // malformed marker segment
  E_EOI = -16,         // no EOI behind the scan
  E_TABLE = -17,       // scan refers to a table the frame did not define
  E_RECORD = -18,      // record_bytes too small for the frame
  E_DC_RANGE = -19,    // DC category > 11 or predictor outside int16
  E_SIZE = -20,        // zero width or height
};

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                             12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                             58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

constexpr int LOOK = 9;

struct Huff {
  bool set = false;
  uint8_t vals[256];
  int maxcode[18];      // largest code of each length, -1 if none
  int valptr[17];
  int mincode[17];
  uint16_t lut[1 << LOOK];   // (length << 8) | symbol for codes of <= LOOK bits, else 0
};

struct Frame {
  int w = 0, h = 0;
  int tq[3], td[3], ta[3];
  int restart = 0;
  bool qset[4] = {false, false, false, false};
  uint16_t qt[4][64];
  Huff dc[4], ac[4];
  long long scan_begin = 0;   // first entropy-coded byte
  long long frame_end = 0;    // one past EOI
};

int build_huff(const uint8_t* bits, const uint8_t* vals, int nvals, Huff& h) {
  int code = 0, k = 0;
  for (int i = 0; i < (1 << LOOK); ++i) h.lut[i] = 0;
  for (int l = 1; l <= 16; ++l) {
    h.valptr[l] = k;
    h.mincode[l] = code;
    for (int i = 0; i < bits[l]; ++i, ++k, ++code) {
      if (code >= (1 << l)) return E_HUFFMAN;          // over-subscribed code
      if (l <= LOOK) {
        const int lo = code << (LOOK - l), n = 1 << (LOOK - l);
        for (int j = 0; j < n; ++j) h.lut[lo + j] = (uint16_t)((l << 8) | vals[k]);
      }
    }
    h.maxcode[l] = bits[l] ? code - 1 : -1;
    code <<= 1;
  }
  h.maxcode[17] = 0x7FFFFFFF;
  if (k != nvals) return E_HUFFMAN;
  memset(h.vals, 0, sizeof h.vals);
  memcpy(h.vals, vals, (size_t)nvals);
  h.set = true;
  return E_OK;
}

inline int rd16(const uint8_t* p) { return (p[0] << 8) | p[1]; }

// Parse one frame that starts at p[0] (SOI); n bytes are readable. Walks the
// marker segments by their lengths and the scan up to EOI.
int parse_frame(const uint8_t* p, long long n, Frame& f, bool tables) {
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
        if (hv != (c == 0 ? 0x22 : 0x11)) return E_SAMPLING;
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
        if (tables) {
          const int rc = build_huff(bits, s + o + 17, total, tc ? f.ac[th] : f.dc[th]);
          if (rc) return rc;
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
        if (tables && (!f.dc[f.td[c]].set || !f.ac[f.ta[c]].set)) return E_TABLE;
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
        break;                                         // a marker: handled by the outer loop
      }
      continue;
    }
    // APPn, COM and anything else with a length: skipped
    pos += len;
  }
}

struct Bits {
  const uint8_t* p;
  long long pos, end;
  uint64_t acc = 0;   // next bit is the top one
  int n = 0;          // bits in acc
  int fake = 0;       // zero bits appended behind the data (at a marker / the end)
  bool marker = false;

  void fill() {
    while (n <= 56) {
      unsigned b = 0;
      if (!marker && pos < end) {
        b = p[pos];
        if (b == 0xFF) {
          if (pos + 1 >= end) {
            marker = true;
          } else if (p[pos + 1] == 0x00) {
            pos += 2;
          } else if (p[pos + 1] == 0xFF) {
            pos += 1;
            continue;
          } else {
            marker = true;
          }
        } else {
          pos += 1;
        }
      } else {
        marker = true;
      }
      if (marker) {
        b = 0;
        if (fake < (1 << 20)) fake += 8;
      }
      acc |= (uint64_t)b << (56 - n);
      n += 8;
    }
  }
  inline unsigned peek(int k) const { return (unsigned)(acc >> (64 - k)); }
  inline void skip(int k) { acc <<= k; n -= k; }
  inline bool overrun() const { return n < fake; }
};

inline int decode_symbol(Bits& b, const Huff& h) {
  const unsigned e = h.lut[b.peek(LOOK)];
  if (e) {
    b.skip(e >> 8);
    return e & 0xFF;
  }
  int l = LOOK + 1;
  int code = (int)b.peek(l);
  while (l <= 16 && code > h.maxcode[l]) {
    ++l;
    if (l <= 16) code = (int)b.peek(l);
  }
  if (l > 16) return E_HUFFMAN;
  b.skip(l);
  const int idx = h.valptr[l] + code - h.mincode[l];
  if (idx < 0 || idx > 255) return E_HUFFMAN;
  return h.vals[idx];
}

inline int receive_extend(Bits& b, int s) {
  const int v = (int)b.peek(s);
  b.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

int decode_block(Bits& b, const Huff& dc, const Huff& ac, int& pred, int16_t* blk) {
  memset(blk, 0, 128);
  if (b.n < 32) b.fill();
  int s = decode_symbol(b, dc);
  if (s < 0) return s;
  if (s > 11) return E_DC_RANGE;
  if (s) pred += receive_extend(b, s);
  if (pred < -32768 || pred > 32767) return E_DC_RANGE;
  blk[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    if (b.n < 32) b.fill();
    const int rs = decode_symbol(b, ac);
    if (rs < 0) return rs;
    const int r = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (r != 15) break;                  // EOB
      if (k + 15 > 63) return E_RUN;       // ZRL: 16 zeros at k .. k + 15
      k += 16;
      continue;
    }
    k += r;
    if (k > 63) return E_RUN;
    blk[kZigzag[k]] = (int16_t)receive_extend(b, s);
    ++k;
  }
  return b.overrun() ? E_TRUNCATED : E_OK;
}

// one frame -> one record; rec has room for 384 + 768 * mw * mh bytes
int decode_frame(const uint8_t* p, long long n, int want_w, int want_h, uint8_t* rec,
                 long long record_bytes, int* dims) {
  std::vector<Frame> holder(1);            // ~14 KB of tables: off the thread's stack
  Frame& f = holder[0];
  int rc = parse_frame(p, n, f, true);
  if (rc) return rc;
  if (dims) { dims[0] = f.w; dims[1] = f.h; }
  if (want_w > 0 && (f.w != want_w || f.h != want_h)) return E_SIZE_CHANGE;
  const long long mw = (f.w + 15) / 16, mh = (f.h + 15) / 16;
  if (384 + 768 * mw * mh > record_bytes) return E_RECORD;
  uint16_t* qt = (uint16_t*)rec;
  for (int c = 0; c < 3; ++c) memcpy(qt + 64 * c, f.qt[f.tq[c]], 128);
  int16_t* coef = (int16_t*)(rec + 384);      // every block is visited and zeroed first
  Bits b;
  b.p = p;
  b.pos = f.scan_begin;
  b.end = n;
  int pred[3] = {0, 0, 0};
  const long long nmcu = mw * mh;
  int next_rst = 0;
  long long in_interval = 0;
  for (long long m = 0; m < nmcu; ++m) {
    if (f.restart && in_interval == f.restart) {
      b.fill();
      // the marker follows the byte the interval ended in
      if (!b.marker || b.n - b.fake >= 8 || b.overrun()) return E_RESTART;
      if (b.pos + 1 >= b.end || p[b.pos] != 0xFF || p[b.pos + 1] != 0xD0 + next_rst)
        return E_RESTART;
      b.pos += 2;
      b.acc = 0; b.n = 0; b.fake = 0; b.marker = false;
      next_rst = (next_rst + 1) & 7;
      pred[0] = pred[1] = pred[2] = 0;
      in_interval = 0;
    }
    ++in_interval;
    const long long my = m / mw, mx = m - my * mw;
    for (int v = 0; v < 2; ++v)
      for (int h = 0; h < 2; ++h) {
        int16_t* blk = coef + 64 * ((2 * my + v) * (2 * mw) + 2 * mx + h);
        rc = decode_block(b, f.dc[f.td[0]], f.ac[f.ta[0]], pred[0], blk);
        if (rc) return rc;
      }
    for (int c = 1; c < 3; ++c) {
      int16_t* blk = coef + 64 * ((3 + c) * nmcu + m);
      rc = decode_block(b, f.dc[f.td[c]], f.ac[f.ta[c]], pred[c], blk);
      if (rc) return rc;
    }
  }
  return E_OK;
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
  if (!data || len < 0 || cap < 0 || (cap > 0 && (!offs || !lens)) || !info) return E_ARG;
  info[0] = info[1] = info[2] = info[3] = 0;
  std::vector<Frame> holder(1);
  long long pos = 0, count = 0;
  while (pos < len) {
    holder[0] = Frame();
    Frame& f = holder[0];
    info[2] = (int)count;
    const int rc = parse_frame(data + pos, len - pos, f, false);
    if (rc) return rc;
    if (count == 0) {
      info[0] = f.w; info[1] = f.h; info[3] = f.restart;
    } else if (f.w != info[0] || f.h != info[1]) {
      return E_SIZE_CHANGE;
    }
    if (count < cap) { offs[count] = pos; lens[count] = f.frame_end; }
    ++count;
    pos += f.frame_end;
  }
  return count;
}

// Entropy-decode nframes frames (data + frame_offs[i], frame_lens[i] bytes)
// into records of record_bytes each at out + i * record_bytes, on up to
// `threads` (<= 16) threads. All frames must have the first one's size.
// Returns 0, or the code of the lowest-numbered frame that failed.
int rnb_jpeg_decode_frames(const uint8_t* data, long long len, const long long* frame_offs,
                           const long long* frame_lens, int nframes, uint8_t* out,
                           long long record_bytes, int threads) {
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
  codes[0] = decode_frame(data + frame_offs[0], frame_lens[0], 0, 0, out, record_bytes, dims);
  if (codes[0]) return codes[0];
  if (threads > 16) threads = 16;
  if (threads > nframes - 1) threads = nframes - 1;
  std::atomic<int> next(1);
  auto work = [&]() {
    for (;;) {
      const int i = next.fetch_add(1);
      if (i >= nframes) return;
      codes[(size_t)i] = decode_frame(data + frame_offs[i], frame_lens[i], dims[0], dims[1],
                                      out + (long long)i * record_bytes, record_bytes, nullptr);
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

}  // extern "C"
