// Baseline-JPEG Huffman decode core shared by the host entropy decoder
// (jpeg_entropy.cpp, librnb_jpeg.so) and the GPU one (jpeg_huff.hip,
// librnb_kernels.so): error codes, the zigzag table, the canonical-table
// builder, the bit reader, decode_block, and decode_interval, the one loop both
// sides run over a restart interval. Plain C++17: every function carries
// RNB_HD, which is empty under a host compiler and __host__ __device__ under
// hipcc, and nothing here needs a HIP header.
//
// Frame record (what both decoders write; see jpeg_entropy.cpp):
//   uint16 qt[3][64], then int16 blocks[B * mw * mh][64] in natural order,
//   B = Hs Vs + 2 blocks per MCU for luma sampling factors Hs x Vs: 6 (4:2:0,
//   2x2), 4 (4:2:2, 2x1) or 3 (4:4:4, 1x1); see Geo below.
//
// Scan record (what rnb_jpeg_pack_scans writes and the interval decoders
// read), 16-byte aligned, all integers little endian:
//   offset 0     uint16 qt[3][64]          as in the frame record (Y, Cb, Cr)
//   offset 384   uint8  huff[6][16 + 256]  table 2c is the DC table and 2c + 1
//                                          the AC table of component c: the 16
//                                          counts of codes of length 1..16,
//                                          then the values, zero padded
//   offset 2016  uint32 n_intervals, mcus_per_interval, scan_len, sampling
//                                          sampling: 0 2x2, 1 2x1, 2 1x1 (so a
//                                          4:2:0 record ends in 0, as it always
//                                          did). It sizes nothing: the decoders
//                                          take the geometry from their caller
//                                          and refuse a record that disagrees.
//                                          mcus_per_interval = min(DRI, nmcu),
//                                          nmcu when DRI = 0; n_intervals =
//                                          ceil(nmcu / mcus_per_interval)
//   offset 2032  uint32 span[n_intervals][2]
//                                          begin / end offsets of each
//                                          interval's bytes inside scan[]: the
//                                          RSTn markers and the fill bytes in
//                                          front of them are outside every span
//   then         uint8  scan[scan_len]     the entropy-coded bytes verbatim
//                                          (FF00 stuffing and markers kept),
//                                          padded with zeros to 16 bytes
// A scan record is untrusted too: scan_record_check validates the header
// against the record's extent and the geometry, every span is checked against
// scan_len, and the tables are rebuilt (and refused) by build_huff.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RNB_HD __host__ __device__
#else
#define RNB_HD
#endif

namespace jpeg_huff {

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
  E_SAMPLING = -9,     // luma factors other than 2x2, 2x1, 1x1, or chroma other than 1x1
  E_MULTISCAN = -10,   // more than one scan, or a scan that is not all three components
  E_SIZE_CHANGE = -11, // frame size differs from the first frame's
  E_HUFFMAN = -12,     // a code that matches no entry / an invalid table
  E_RUN = -13,         // zero run past coefficient 63
  E_RESTART = -14,     // missing or wrong RSTn
  E_MARKER = -15,      // malformed marker segment
  E_EOI = -16,         // no EOI behind the scan
  E_TABLE = -17,       // scan refers to a table the frame did not define
  E_RECORD = -18,      // record_bytes / out_cap too small for the frame
  E_DC_RANGE = -19,    // DC category > 11 or predictor outside int16
  E_SIZE = -20,        // zero width or height
  E_SCANREC = -21,     // malformed scan record (header, span table, extent, sampling word)
  E_SAMPLING_CHANGE = -22,   // sampling differs from the first frame's
};

// The MCU of a sampling: luma factors (hs, vs) and nb = hs * vs + 2 blocks, the
// Y blocks row-major, then Cb, then Cr. It covers 8 hs x 8 vs luma pixels.
struct Geo {
  int hs, vs, nb;
};

enum { SAMPLING_420 = 0, SAMPLING_422 = 1, SAMPLING_444 = 2 };

// the sampling word of a scan record / the `sampling` argument of the entry
// points -> its geometry; false for anything else
RNB_HD inline bool geo_of(int sampling, Geo& g) {
  if (sampling < SAMPLING_420 || sampling > SAMPLING_444) return false;
  g.hs = sampling == SAMPLING_444 ? 1 : 2;
  g.vs = sampling == SAMPLING_420 ? 2 : 1;
  g.nb = g.hs * g.vs + 2;
  return true;
}

RNB_HD inline Geo geo_420() {
  Geo g = {2, 2, 6};
  return g;
}

// component of block j of an MCU
RNB_HD inline int block_comp(int j, const Geo& g) { return j < g.nb - 2 ? 0 : j - (g.nb - 3); }

#define RNB_JPEG_ZIGZAG                                                                   \
  {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, \
   41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, \
   30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

static const uint8_t kZigzag[64] = RNB_JPEG_ZIGZAG;
#if defined(__HIPCC__) || defined(__HIP__)
static __device__ const uint8_t kZigzagDev[64] = RNB_JPEG_ZIGZAG;
#endif

RNB_HD inline int zigzag(int k) {
#if defined(__HIP_DEVICE_COMPILE__)
  return kZigzagDev[k];
#else
  return kZigzag[k];
#endif
}

constexpr int LOOK = 9;

// scan record layout
constexpr int SR_HUFF = 384;                 // 6 tables of SR_TABLE bytes
constexpr int SR_TABLE = 16 + 256;
constexpr int SR_HEADER = SR_HUFF + 6 * SR_TABLE;   // 2016
constexpr int SR_SPANS = SR_HEADER + 16;            // 2032

// One canonical table: the LOOK-bit lookahead and the per-length slow path.
// Plain data, so that it can live in LDS as well.
struct Huff {
  uint8_t set;
  uint8_t vals[256];
  int maxcode[18];      // largest code of each length, -1 if none
  int valptr[17];
  int mincode[17];
  uint16_t lut[1 << LOOK];   // (length << 8) | symbol for codes of <= LOOK bits, else 0
};

// counts[l - 1]: number of codes of length l = 1..16; vals: nvals symbols
RNB_HD inline int build_huff(const uint8_t* counts, const uint8_t* vals, int nvals, Huff& h) {
  int total = 0;
  for (int l = 0; l < 16; ++l) total += counts[l];
  if (total > 256 || total != nvals) return E_HUFFMAN;
  int code = 0, k = 0;
  for (int i = 0; i < (1 << LOOK); ++i) h.lut[i] = 0;
  for (int l = 1; l <= 16; ++l) {
    h.valptr[l] = k;
    h.mincode[l] = code;
    const int cnt = counts[l - 1];
    for (int i = 0; i < cnt; ++i, ++k, ++code) {
      if (code >= (1 << l)) return E_HUFFMAN;          // over-subscribed code
      if (l <= LOOK) {
        const int lo = code << (LOOK - l), n = 1 << (LOOK - l);
        for (int j = 0; j < n; ++j) h.lut[lo + j] = (uint16_t)((l << 8) | vals[k]);
      }
    }
    h.maxcode[l] = cnt ? code - 1 : -1;
    code <<= 1;
  }
  h.maxcode[17] = 0x7FFFFFFF;
  for (int i = 0; i < 256; ++i) h.vals[i] = i < nvals ? vals[i] : (uint8_t)0;
  h.set = 1;
  return E_OK;
}

// Bit reader over p[pos .. end): removes FF00 stuffing and FF fill bytes, stops
// at a marker or at `end` and supplies zero bits from there on (`fake` counts
// them, so that overrun() tells whether any was consumed). No byte at or past
// `end` is read.
struct Bits {
  const uint8_t* p;
  long long pos, end;
  uint64_t acc = 0;   // next bit is the top one
  int n = 0;          // bits in acc
  int fake = 0;       // zero bits appended behind the data (at a marker / the end)
  bool marker = false;

  RNB_HD void fill() {
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
  RNB_HD inline unsigned peek(int k) const { return (unsigned)(acc >> (64 - k)); }
  RNB_HD inline void skip(int k) { acc <<= k; n -= k; }
  RNB_HD inline bool overrun() const { return n < fake; }
};

RNB_HD inline int decode_symbol(Bits& b, const Huff& h) {
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

RNB_HD inline int receive_extend(Bits& b, int s) {
  const int v = (int)b.peek(s);
  b.skip(s);
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// 128 zero bytes at blk (16-byte aligned in a frame record)
RNB_HD inline void zero_block(int16_t* blk) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));     // no HIP header needed
  for (int i = 0; i < 8; ++i) ((u32x4*)blk)[i] = (u32x4)(0u);
#else
  memset(blk, 0, 128);
#endif
}

RNB_HD inline int decode_block(Bits& b, const Huff& dc, const Huff& ac, int& pred, int16_t* blk) {
  zero_block(blk);
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
    blk[zigzag(k)] = (int16_t)receive_extend(b, s);
    ++k;
  }
  return b.overrun() ? E_TRUNCATED : E_OK;
}

// the DC and AC table of each component
struct Tables {
  const Huff* dc[3];
  const Huff* ac[3];
};

// block j = 0..nb-1 of MCU m (the Y blocks, Cb, Cr) inside a record's
// coefficients: a function of the geometry alone
RNB_HD inline int16_t* mcu_block(int16_t* coef, long long m, int j, long long mw, long long nmcu,
                                 const Geo& g = geo_420()) {
  if (j >= g.nb - 2) return coef + 64 * (j * nmcu + m);   // (hs vs - 1 + c) * nmcu + m
  const long long my = m / mw, mx = m - my * mw;
  // hs is 1 or 2: j / hs and j % hs
  return coef + 64 * ((g.vs * my + (j >> (g.hs - 1))) * (g.hs * mw) + g.hs * mx + (j & (g.hs - 1)));
}

// One restart interval: n_mcu MCUs from MCU m0 on, decoded from p[begin .. end)
// with the DC predictors starting at zero, into the blocks of `coef` (the
// int16 part of a frame record of mw MCUs per row, nmcu in all; the caller
// guarantees m0 + n_mcu <= nmcu). `b` is the reader it leaves behind, for the
// caller's check of what follows the interval. Every visited block is zeroed,
// then filled; on an error the code is returned and, with zero_tail, the block
// it happened in and the interval's remaining blocks are zeroed.
RNB_HD inline int decode_interval(Bits& b, const uint8_t* p, long long begin, long long end,
                                  const Tables& t, long long m0, long long n_mcu, long long mw,
                                  long long nmcu, int16_t* coef, bool zero_tail,
                                  const Geo& g = geo_420()) {
  b.p = p;
  b.pos = begin;
  b.end = end;
  b.acc = 0; b.n = 0; b.fake = 0; b.marker = false;
  int pred0 = 0, pred1 = 0, pred2 = 0;
  int rc = E_OK;
  long long i = 0;
  int j = 0;
  const int ny = g.nb - 2;
  for (; i < n_mcu; ++i) {
    const long long m = m0 + i;
    for (j = 0; j < ny; ++j) {
      rc = decode_block(b, *t.dc[0], *t.ac[0], pred0, mcu_block(coef, m, j, mw, nmcu, g));
      if (rc) break;
    }
    if (rc) break;
    rc = decode_block(b, *t.dc[1], *t.ac[1], pred1, mcu_block(coef, m, ny, mw, nmcu, g));
    if (rc) { j = ny; break; }
    rc = decode_block(b, *t.dc[2], *t.ac[2], pred2, mcu_block(coef, m, ny + 1, mw, nmcu, g));
    if (rc) { j = ny + 1; break; }
  }
  if (rc && zero_tail) {
    for (; i < n_mcu; ++i, j = 0)
      for (; j < g.nb; ++j) zero_block(mcu_block(coef, m0 + i, j, mw, nmcu, g));
  }
  return rc;
}

// What must hold behind an interval that a restart marker follows: the reader
// stopped at a marker (or the end of its bytes) with fewer than 8 real bits
// left and consumed none that were not there.
RNB_HD inline bool interval_ended(Bits& b) {
  b.fill();
  return b.marker && b.n - b.fake < 8 && !b.overrun();
}

struct ScanHeader {
  uint32_t n_intervals, mcus_per_interval, scan_len;
};

RNB_HD inline uint32_t load_u32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// Validate the header of the scan record at rec, which may use `extent` bytes,
// for a frame of nmcu MCUs: afterwards the span table and scan[] lie inside
// the extent, the intervals tile the frame's MCUs exactly, and the record's
// sampling word is the caller's `sampling` (SAMPLING_420 ..): the word is only
// compared, the geometry is the caller's.
RNB_HD inline int scan_record_check(const uint8_t* rec, long long extent, long long nmcu,
                                    ScanHeader& h, int sampling = SAMPLING_420) {
  h.n_intervals = h.mcus_per_interval = h.scan_len = 0;
  if (extent < SR_SPANS + 8) return E_SCANREC;
  if (load_u32(rec + SR_HEADER + 12) != (uint32_t)sampling) return E_SCANREC;
  h.n_intervals = load_u32(rec + SR_HEADER);
  h.mcus_per_interval = load_u32(rec + SR_HEADER + 4);
  h.scan_len = load_u32(rec + SR_HEADER + 8);
  const long long per = h.mcus_per_interval;
  if (per < 1 || per > nmcu) return E_SCANREC;
  if ((long long)h.n_intervals != (nmcu + per - 1) / per) return E_SCANREC;
  if (SR_SPANS + 8LL * h.n_intervals + (long long)h.scan_len > extent) return E_SCANREC;
  return E_OK;
}

// Interval i of a checked scan record into the frame record's coefficients:
// its span is checked against scan_len, a non-final interval must end exactly
// where its span ends (E_RESTART otherwise), the final one must only not
// overrun (E_TRUNCATED, from decode_block).
RNB_HD inline int decode_record_interval(const uint8_t* rec, const ScanHeader& h, long long i,
                                         const Tables& t, long long mw, long long nmcu,
                                         int16_t* coef, const Geo& g = geo_420()) {
  const long long per = h.mcus_per_interval;
  const long long m0 = i * per;
  const long long n_mcu = nmcu - m0 < per ? nmcu - m0 : per;
  const uint8_t* sp = rec + SR_SPANS + 8 * i;
  const long long begin = load_u32(sp), end = load_u32(sp + 4);
  if (begin > end || end > (long long)h.scan_len) {
    for (long long k = 0; k < n_mcu; ++k)
      for (int j = 0; j < g.nb; ++j) zero_block(mcu_block(coef, m0 + k, j, mw, nmcu, g));
    return E_SCANREC;
  }
  const uint8_t* scan = rec + SR_SPANS + 8LL * h.n_intervals;
  Bits b;
  const int rc = decode_interval(b, scan, begin, end, t, m0, n_mcu, mw, nmcu, coef, true, g);
  if (rc) return rc;
  if (i + 1 < (long long)h.n_intervals && (!interval_ended(b) || b.pos != end)) return E_RESTART;
  return E_OK;
}

// ---------------------------------------------------------------------------
// One interval decoded by synchronised subsequences (jpeg_huff_subseq_kernel
// and its host emulation rnb_jpeg_decode_scans_subseq_host run these
// functions pass by pass; the result equals decode_record_interval's byte for
// byte).
//
// The span [begin, end) is cut into subsequences of S raw bytes; a symbol
// belongs to the subsequence its first bit lies in. Positions are counted in
// DE-STUFFED bits: the raw bytes parse without context into data bytes (any
// byte but FF; FF 00, which starts at its FF), fill bytes (FF in front of FF)
// and a marker (FF in front of anything else, or as the span's last byte),
// because a 00 behind an FF is always the second byte of a pair. subseq_count
// counts the data bytes that start in a subsequence, so a prefix sum gives
// every boundary's bit position, and the first marker found anywhere ends the
// span for every reader, as it does for the serial one. The decoder's state
// between two symbols is (bit position, block in MCU j, coefficient index k;
// k = 0: DC next), kept relative to the subsequence's boundary: a symbol is at
// most 31 bits, so a state packs into 15 bits whatever the span's length.
//
// Passes: every subsequence is scanned (no coefficient written) from the
// guess (boundary, 0, 0); then each takes its left neighbour's exit state as
// its entry and is scanned again while any entry changes. Subsequence 0 starts
// at the truth, so after round r the first r + 1 are true and at most
// n_sub - 1 rounds run. Prefix sums of the blocks completed and of the DC
// differences per component give each entry's block index and predictors, and
// the write pass decodes every subsequence from its true entry into a frame
// whose coefficients were zeroed before: a block may begin in one subsequence
// and end in the next, so only non-zero coefficients are stored.
//
// A scan from a wrong guess meets invalid data at once. It must not stop
// there, or the error state is handed down the chain and nothing ever
// synchronises; subseq_scan recovers by one fixed rule: a code that matches
// no entry skips one bit, a DC category above 11 reads no bits, a run or ZRL
// past coefficient 63 ends the block. On the true chain no recovery happens in
// front of the first real error, which the write pass reports, and everything
// from the failing block on is zeroed, so the result does not depend on the
// rule.
// ---------------------------------------------------------------------------
constexpr int SUBSEQ_CAP = 1024;                     // subsequences per span at most
constexpr long long SUBSEQ_MAX_SPAN = 1LL << 28;     // bit positions and block counts fit 32 bits

RNB_HD inline bool subseq_bytes_ok(long long s) { return s >= 16 && s <= 4096 && s % 16 == 0; }

// the subsequence size used for a span of len bytes: S, raised so that at most
// SUBSEQ_CAP subsequences cover it
RNB_HD inline long long subseq_effective(long long S, long long len) {
  if ((len + S - 1) / S <= SUBSEQ_CAP) return S;
  return ((len + SUBSEQ_CAP - 1) / SUBSEQ_CAP + 15) & ~15LL;
}

struct SubseqPlan {
  long long begin, end, S;
  int n_sub;
};

// Whether the checked record's frame takes the subsequence path, and how: one
// interval whose span decode_record_interval would accept, short enough for
// 32-bit bit positions, and longer than one subsequence. Everything else is
// decoded as before, one interval per lane.
RNB_HD inline bool subseq_plan(const uint8_t* rec, const ScanHeader& h, int subseq_bytes,
                               SubseqPlan& pl) {
  pl.begin = pl.end = 0;
  pl.S = subseq_bytes;
  pl.n_sub = 1;
  if (h.n_intervals != 1 || !subseq_bytes_ok(subseq_bytes)) return false;
  pl.begin = load_u32(rec + SR_SPANS);
  pl.end = load_u32(rec + SR_SPANS + 4);
  if (pl.begin > pl.end || pl.end > (long long)h.scan_len) return false;
  const long long len = pl.end - pl.begin;
  if (len > SUBSEQ_MAX_SPAN) return false;
  pl.S = subseq_effective(subseq_bytes, len);
  const long long n = (len + pl.S - 1) / pl.S;
  if (n < 2) return false;
  pl.n_sub = (int)n;
  return true;
}

// The data bytes that start in p[b0 .. b1) of the span [begin, end), up to the
// first marker there. Returns the marker's position, or `end` without one.
// Reads p[b0 - 1] (when b0 > begin) and p[r + 1] behind an FF at r (when
// r + 1 < end): nothing outside the span.
RNB_HD inline long long subseq_count(const uint8_t* p, long long begin, long long end,
                                     long long b0, long long b1, uint32_t& count) {
  unsigned prev = b0 > begin ? p[b0 - 1] : 0u;
  uint32_t n = 0;
  long long at = end;
  for (long long r = b0; r < b1; ++r) {
    const unsigned c = p[r];
    if (c == 0xFF) {
      const unsigned nx = r + 1 < end ? p[r + 1] : 0xD9u;
      if (nx == 0x00) {
        ++n;
      } else if (nx != 0xFF) {
        at = r;
        break;
      }
    } else if (!(c == 0x00 && prev == 0xFF)) {
      ++n;
    }
    prev = c;
  }
  count = n;
  return at;
}

// where the reader of the subsequence at b0 starts: behind the 00 of a
// stuffing pair that the boundary cuts (fill bytes the reader skips itself)
RNB_HD inline long long subseq_start(const uint8_t* p, long long begin, long long b0) {
  return b0 + ((b0 > begin && p[b0] == 0x00 && p[b0 - 1] == 0xFF) ? 1 : 0);
}

// state: (bits behind the boundary << 9) | (j << 6) | k; an MCU has at most 6
// blocks whatever the sampling, so j fits its three bits
RNB_HD inline uint32_t subseq_state(int off, int j, int k) {
  return ((uint32_t)(off > 63 ? 63 : off) << 9) | ((uint32_t)j << 6) | (uint32_t)k;
}

// a reader at raw position `at`, `off` bits further
RNB_HD inline void subseq_open(Bits& b, const uint8_t* p, long long at, long long end, int off) {
  b.p = p;
  b.pos = at;
  b.end = end;
  b.acc = 0; b.n = 0; b.fake = 0; b.marker = false;
  while (off > 0) {
    b.fill();
    const int s = off < 32 ? off : 32;
    b.skip(s);
    off -= s;
  }
}

struct SubseqExit {
  uint32_t state;      // relative to the NEXT boundary
  uint32_t blocks;     // blocks completed
  int dc0, dc1, dc2;   // sum of the DC differences per component
};

// Scan the subsequence whose reader starts at `at` and which holds `limit`
// de-stuffed bits, from `entry`: every symbol that starts in front of `limit`,
// with the recovery rule above and without writing. Every iteration consumes
// at least one bit and at most 31, so the loop runs at most `limit` times and
// the exit state lies fewer than 31 bits behind the next boundary. tabs: the
// six tables of the scan record (2c: DC, 2c + 1: AC of component c).
RNB_HD inline void subseq_scan(const uint8_t* p, long long at, long long end, int limit,
                               const Huff* tabs, uint32_t entry, SubseqExit& x,
                               const Geo& geo = geo_420()) {
  int j = (int)(entry >> 6) & 7, k = (int)(entry & 63);
  int pos = (int)(entry >> 9);
  Bits b;
  subseq_open(b, p, at, end, pos);
  uint32_t nb = 0;
  int d0 = 0, d1 = 0, d2 = 0;
  while (pos < limit) {
    if (b.n < 32) b.fill();
    const int n0 = b.n;
    const int c = block_comp(j, geo);
    bool done = false;
    if (k == 0) {
      const int s = decode_symbol(b, tabs[2 * c]);
      if (s < 0) {
        if (b.n == n0) b.skip(1);
      } else {
        if (s >= 1 && s <= 11) {
          const int d = receive_extend(b, s);
          if (c == 0) d0 += d; else if (c == 1) d1 += d; else d2 += d;
        }
        k = 1;
      }
    } else {
      const int rs = decode_symbol(b, tabs[2 * c + 1]);
      if (rs < 0) {
        if (b.n == n0) b.skip(1);
      } else {
        const int r = rs >> 4, s = rs & 15;
        if (s == 0) {
          if (r != 15 || k + 15 > 63) {
            done = true;
          } else {
            k += 16;
            done = k > 63;
          }
        } else {
          k += r;
          if (k > 63) {
            done = true;
          } else {
            b.skip(s);
            ++k;
            done = k > 63;
          }
        }
      }
    }
    pos += n0 - b.n;
    if (done) {
      k = 0;
      j = j >= geo.nb - 1 ? 0 : j + 1;
      ++nb;
    }
  }
  x.state = subseq_state(pos - limit, j, k);
  x.blocks = nb;
  x.dc0 = d0; x.dc1 = d1; x.dc2 = d2;
}

// what a 64-bit prefix sum of DC differences is stored as: in front of the
// first error every true predictor is inside int16, so the clamp changes no
// value that counts, and a clamped one is out of range for whoever starts
// from it
RNB_HD inline int subseq_clamp_pred(long long v) {
  return v < -(1 << 20) ? -(1 << 20) : v > (1 << 20) ? (1 << 20) : (int)v;
}

// The write pass of one subsequence: from its true entry state, global block
// index g and predictors, decode every symbol that starts in front of `limit`
// (`last`: no limit, the span's last subsequence goes on over the reader's zero
// bits until its block ends, as the serial loop does) and store the non-zero
// coefficients of blocks g < nb nmcu; `rem` is the number of real bits from the
// subsequence's boundary to the end of the span, for E_TRUNCATED. Stops at the
// first error and returns its code, the block in bad_block: with decode_block's
// checks in decode_block's order, so the lowest subsequence that reports one
// reports the serial decoder's first error.
RNB_HD inline int subseq_write(const uint8_t* p, long long at, long long end, int limit, bool last,
                               long long rem, const Huff* tabs, uint32_t entry, long long g,
                               int p0, int p1, int p2, long long mw, long long nmcu, int16_t* coef,
                               long long& bad_block, const Geo& geo = geo_420()) {
  const long long total = geo.nb * nmcu;
  int k = (int)(entry & 63);
  long long pos = (long long)(entry >> 9);
  long long m = g / geo.nb;
  int j = (int)(g - geo.nb * m);
  Bits b;
  subseq_open(b, p, at, end, (int)pos);
  while (g < total && (last || pos < limit)) {
    int16_t* blk = mcu_block(coef, m, j, mw, nmcu, geo);
    const int c = block_comp(j, geo);
    bool done = false;
    while (!done && (last || pos < limit)) {
      if (b.n < 32) b.fill();
      const int n0 = b.n;
      int rc = E_OK;
      if (k == 0) {
        const int s = decode_symbol(b, tabs[2 * c]);
        if (s < 0) {
          rc = s;
        } else if (s > 11) {
          rc = E_DC_RANGE;
        } else {
          int pred = c == 0 ? p0 : c == 1 ? p1 : p2;
          if (s) pred += receive_extend(b, s);
          if (pred < -32768 || pred > 32767) {
            rc = E_DC_RANGE;
          } else {
            if (c == 0) p0 = pred; else if (c == 1) p1 = pred; else p2 = pred;
            if (pred) blk[0] = (int16_t)pred;
            k = 1;
          }
        }
      } else {
        const int rs = decode_symbol(b, tabs[2 * c + 1]);
        if (rs < 0) {
          rc = rs;
        } else {
          const int r = rs >> 4, s = rs & 15;
          if (s == 0) {
            if (r != 15) {
              done = true;                       // EOB
            } else if (k + 15 > 63) {
              rc = E_RUN;
            } else {
              k += 16;
              done = k > 63;
            }
          } else {
            k += r;
            if (k > 63) {
              rc = E_RUN;
            } else {
              blk[zigzag(k)] = (int16_t)receive_extend(b, s);
              ++k;
              done = k > 63;
            }
          }
        }
      }
      pos += n0 - b.n;
      if (rc) {
        bad_block = g;
        return rc;
      }
    }
    if (!done) break;                            // the boundary lies inside this block
    if (pos > rem) {
      bad_block = g;
      return E_TRUNCATED;
    }
    k = 0;
    ++g;
    if (++j == geo.nb) {
      j = 0;
      ++m;
    }
  }
  return E_OK;
}

}  // namespace jpeg_huff
