// Stand-alone check of the subsequence decoder's host emulation
// (rnb_jpeg_decode_scans_subseq_host in jpeg_entropy.cpp, the header functions
// jpeg_huff_subseq_kernel runs) against the serial interval decoder
// (rnb_jpeg_decode_scans_host). Meant to be compiled together with
// jpeg_entropy.cpp under -fsanitize=address,undefined and run directly:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       jpeg_entropy.cpp bench/jpeg_subseq_check.cpp -lpthread -o check
//   ./check [--sampling N] stream.mjpeg ...
//
// N: 0 4:2:0, 1 4:2:2, 2 4:4:4, which must be every stream's (default: whatever
// each stream's first frame has); both decoders are called through the entry
// points that carry the sampling, and the record corruptions include the
// sampling word.
//
// For S in {16, 64, 256} and every frame of every stream: the frame is packed,
// and the clean scan record and a list of damaged copies go through both
// decoders, which must give the same status and the same record, byte for
// byte: the span's end shortened by 1, 7 and 100 bytes, begin > end, single
// flipped bytes spread over the scan and next to subsequence boundaries, 40
// bytes of A5 behind the last block, a raised Huffman table count, a wrong
// n_intervals, and seeded single-byte corruptions of the scan and of the whole
// record. Every buffer is a heap block of exactly its size, so a read or write
// one byte outside is a sanitizer report. Exit status 0 and "no fault": all of
// that held.
//
//   ./check [--sampling N] --records W H record.bin ...
// runs both decoders at S = 16, 64, 128 and 256 on each file as one scan record
// of a W x H frame of sampling N (default 0) (the fixed damaged records that the
// GPU tests then give the kernel) and prints each status.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" {
long long rnb_mjpeg_index_s(const uint8_t* data, long long len, long long* offs, long long* lens,
                            long long cap, int* info);
long long rnb_jpeg_pack_scans_s(const uint8_t* data, long long len, const long long* frame_offs,
                                const long long* frame_lens, int nframes, uint8_t* out,
                                long long out_cap, long long* scan_offs, int want_w, int want_h,
                                int* info, int sampling);
int rnb_jpeg_decode_scans_host_s(const uint8_t* scans, long long scans_len,
                                 const long long* scan_offs, int nframes, int mw, int mh,
                                 uint8_t* out, long long out_len, long long record_bytes,
                                 int* status, int sampling);
int rnb_jpeg_decode_scans_subseq_host_s(const uint8_t* scans, long long scans_len,
                                        const long long* scan_offs, int nframes, int mw, int mh,
                                        uint8_t* out, long long out_len, long long record_bytes,
                                        int* status, int subseq_bytes, int* rounds, int sampling);
}

static uint32_t rng_state = 0x13579BDu;
static uint32_t rng() {                       // xorshift32
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

static int g_mw, g_mh, g_sampling;
static long long g_record_bytes;

// MCU grid and record size of a w x h frame of g_sampling
static void set_geometry(int w, int h) {
  const int hs = g_sampling == 2 ? 1 : 2, vs = g_sampling == 0 ? 2 : 1;
  g_mw = (w + 8 * hs - 1) / (8 * hs);
  g_mh = (h + 8 * vs - 1) / (8 * vs);
  g_record_bytes = 384 + 128LL * (hs * vs + 2) * g_mw * g_mh;
}
static long long g_cases = 0, g_failed = 0, g_rounds = 0;

// one scan record (an exact-size heap block) through a decoder; S = 0: the serial one
static int decode(const std::vector<uint8_t>& scans, int S, std::vector<uint8_t>& rec, int* status,
                  int* rounds) {
  uint8_t* s = new uint8_t[scans.size()];
  memcpy(s, scans.data(), scans.size());
  uint8_t* out = new uint8_t[g_record_bytes];
  memset(out, S ? 0xA5 : 0x5A, (size_t)g_record_bytes);
  const long long offs[2] = {0, (long long)scans.size()};
  *status = 12345;
  *rounds = 0;
  const int rc =
      S ? rnb_jpeg_decode_scans_subseq_host_s(s, (long long)scans.size(), offs, 1, g_mw, g_mh, out,
                                              g_record_bytes, g_record_bytes, status, S, rounds,
                                              g_sampling)
        : rnb_jpeg_decode_scans_host_s(s, (long long)scans.size(), offs, 1, g_mw, g_mh, out,
                                       g_record_bytes, g_record_bytes, status, g_sampling);
  rec.assign(out, out + g_record_bytes);
  delete[] out;
  delete[] s;
  return rc;
}

// both decoders on one record: 0 when codes, status and records are equal
static int compare(const std::vector<uint8_t>& scans, int S, const char* what, long long which,
                   int* status_out = nullptr) {
  std::vector<uint8_t> want, got;
  int ws = 0, gs = 0, wr = 0, gr = 0;
  const int wc = decode(scans, 0, want, &ws, &wr), gc = decode(scans, S, got, &gs, &gr);
  ++g_cases;
  if (ws < 0) ++g_failed;
  g_rounds += gr;
  if (status_out) *status_out = ws;
  if (wc != 0 || gc != 0 || ws != gs || ws > 0 || want != got) {
    fprintf(stderr, "S = %d, %s %lld: codes %d %d, status %d %d, records %s\n", S, what, which, wc,
            gc, ws, gs, want == got ? "equal" : "differ");
    return 1;
  }
  return 0;
}

static uint32_t get32(const std::vector<uint8_t>& v, size_t at) {
  uint32_t x;
  memcpy(&x, v.data() + at, 4);
  return x;
}
static void put32(std::vector<uint8_t>& v, size_t at, uint32_t x) { memcpy(v.data() + at, &x, 4); }

static bool read_file(const char* path, std::vector<uint8_t>& file) {
  FILE* fp = fopen(path, "rb");
  if (!fp) { perror(path); return false; }
  uint8_t chunk[4096];
  size_t got;
  while ((got = fread(chunk, 1, sizeof chunk, fp)) > 0) file.insert(file.end(), chunk, chunk + got);
  fclose(fp);
  return true;
}

// the damage list on one clean scan record
static int damage(const std::vector<uint8_t>& scans, int S) {
  if (compare(scans, S, "clean", 0)) return 1;
  const uint32_t n_int = get32(scans, 2016), scan_len = get32(scans, 2024);
  if (n_int != 1) return 0;                   // restart markers: passes through, checked above
  const size_t body = 2032 + 8;
  const uint32_t end = get32(scans, 2036);
  const uint32_t cuts[3] = {1, 7, 100};
  for (int i = 0; i < 3; ++i) {
    std::vector<uint8_t> bad(scans);
    put32(bad, 2036, end > cuts[i] ? end - cuts[i] : 0);
    if (compare(bad, S, "span end shortened by", cuts[i])) return 1;
  }
  {
    std::vector<uint8_t> bad(scans);
    put32(bad, 2032, end + 1);
    if (compare(bad, S, "begin past end", 0)) return 1;
    bad = scans;
    put32(bad, 2036, scan_len + 1);
    if (compare(bad, S, "end past scan_len", 0)) return 1;
    bad = scans;
    put32(bad, 2016, 2);
    if (compare(bad, S, "n_intervals", 2)) return 1;
    bad = scans;
    bad[384 + 272 + 15] = (uint8_t)(bad[384 + 272 + 15] + 40);
    if (compare(bad, S, "table count raised", 0)) return 1;
    // 40 bytes of A5 behind the last block: scan_len and the span grow
    bad.assign(scans.begin(), scans.begin() + body + scan_len);
    bad.insert(bad.end(), 40, 0xA5);
    bad.resize((bad.size() + 15) & ~(size_t)15, 0);
    put32(bad, 2024, scan_len + 40);
    put32(bad, 2036, end + 40);
    if (compare(bad, S, "bytes behind the last block", 40)) return 1;
  }
  if (scan_len < 4) return 0;
  for (uint32_t i = 0; i < 8; ++i) {          // spread over the scan
    std::vector<uint8_t> bad(scans);
    bad[body + (size_t)((2 * i + 1) * (unsigned long long)scan_len / 16)] ^= (uint8_t)(0x11 * (i + 1));
    if (compare(bad, S, "flip at sixteenth", 2 * i + 1)) return 1;
  }
  for (uint32_t at = S; at + 1 < scan_len && at <= 6u * S; at += S) {
    for (int d = -1; d <= 1; ++d) {           // next to a subsequence boundary
      std::vector<uint8_t> bad(scans);
      bad[body + at + d] ^= 0x81;
      if (compare(bad, S, "flip next to the boundary at", at)) return 1;
      bad = scans;
      bad[body + at + d] = 0xFF;              // a stuffing pair, fill byte or marker there
      if (compare(bad, S, "FF next to the boundary at", at)) return 1;
    }
  }
  for (int i = 0; i < 300; ++i) {
    std::vector<uint8_t> bad(scans);
    bad[body + rng() % scan_len] ^= (uint8_t)(1 + rng() % 255);
    if (compare(bad, S, "scan corruption", i)) return 1;
  }
  for (int i = 0; i < 100; ++i) {
    std::vector<uint8_t> bad(scans);
    size_t at = rng() % bad.size();
    if (i % 2) at = 2016 + rng() % 24;        // header and the span
    if (i % 8 == 3) at = 384 + 272 * (rng() % 6) + rng() % 16;      // a table's counts
    bad[at] ^= (uint8_t)(1 + rng() % 255);
    if (compare(bad, S, "record corruption", i)) return 1;
  }
  return 0;
}

static int check_records(int argc, char** argv) {
  const int w = atoi(argv[2]), h = atoi(argv[3]);
  if (w < 1 || h < 1 || w > 65535 || h > 65535) return 2;
  set_geometry(w, h);
  const int sizes[4] = {16, 64, 128, 256};
  for (int i = 4; i < argc; ++i) {
    std::vector<uint8_t> scans;
    if (!read_file(argv[i], scans)) return 2;
    int status = 0;
    for (int k = 0; k < 4; ++k)
      if (compare(scans, sizes[k], argv[i], 0, &status)) return 1;
    printf("%s: status %d\n", argv[i], status);
  }
  printf("jpeg_subseq_check: %d scan records, no fault\n", argc - 4);
  return 0;
}

int main(int argc, char** argv) {
  int want_sampling = -1;
  if (argc >= 3 && !strcmp(argv[1], "--sampling")) {
    want_sampling = atoi(argv[2]);
    if (want_sampling < 0 || want_sampling > 2) return 2;
    argv[2] = argv[0];
    argv += 2;
    argc -= 2;
  }
  g_sampling = want_sampling < 0 ? 0 : want_sampling;
  if (argc >= 5 && !strcmp(argv[1], "--records")) return check_records(argc, argv);
  if (argc < 2) {
    fprintf(stderr, "usage: %s [--sampling N] stream.mjpeg ... | --records W H record...\n",
            argv[0]);
    return 2;
  }
  const int sizes[3] = {16, 64, 256};
  long long frames = 0;
  for (int a = 1; a < argc; ++a) {
    std::vector<uint8_t> file;
    if (!read_file(argv[a], file)) return 2;
    int info[5];
    long long count = rnb_mjpeg_index_s(file.data(), (long long)file.size(), nullptr, nullptr, 0,
                                        info);
    if (count < 1) { fprintf(stderr, "%s: index failed: %lld\n", argv[a], count); return 1; }
    std::vector<long long> offs((size_t)count), lens((size_t)count);
    count = rnb_mjpeg_index_s(file.data(), (long long)file.size(), offs.data(), lens.data(), count,
                              info);
    if (want_sampling >= 0 && want_sampling != info[4]) {
      fprintf(stderr, "%s: the stream's sampling is %d, not %d\n", argv[a], info[4], want_sampling);
      return 2;
    }
    g_sampling = info[4];
    set_geometry(info[0], info[1]);
    for (long long i = 0; i < count; ++i, ++frames) {
      const long long cap = (2048 + 8LL * g_mw * g_mh + lens[(size_t)i] + 31) & ~15LL;
      uint8_t* out = new uint8_t[cap];
      long long so[2];
      int pinfo[3];
      const long long n = rnb_jpeg_pack_scans_s(file.data(), (long long)file.size(),
                                                &offs[(size_t)i], &lens[(size_t)i], 1, out, cap, so,
                                                0, 0, pinfo, g_sampling);
      if (n < 0) { fprintf(stderr, "%s: frame %lld is not packed: %lld\n", argv[a], i, n); return 1; }
      const std::vector<uint8_t> scans(out, out + n);
      delete[] out;
      for (int k = 0; k < 3; ++k)
        if (damage(scans, sizes[k])) return 1;
    }
  }
  // the emulation refuses a bad subseq_bytes and a missing rounds pointer
  {
    std::vector<uint8_t> rec((size_t)g_record_bytes), scans(4096, 0);
    const long long o[2] = {0, 4096};
    int status = 0, rounds = 0;
    const int bad[5] = {0, 8, 24, 4112, -16};
    for (int k = 0; k < 5; ++k)
      if (rnb_jpeg_decode_scans_subseq_host_s(scans.data(), 4096, o, 1, g_mw, g_mh, rec.data(),
                                              g_record_bytes, g_record_bytes, &status, bad[k],
                                              &rounds, g_sampling) >= 0) {
        fprintf(stderr, "subseq_bytes %d was accepted\n", bad[k]);
        return 1;
      }
    if (rnb_jpeg_decode_scans_subseq_host_s(scans.data(), 4096, o, 1, g_mw, g_mh, rec.data(),
                                            g_record_bytes, g_record_bytes, &status, 64, nullptr,
                                            g_sampling) >= 0)
      return 1;
  }
  printf("jpeg_subseq_check: %lld frames, %lld records through both decoders (%lld refused by "
         "both), %lld synchronisation rounds; no fault\n", frames, g_cases, g_failed, g_rounds);
  return 0;
}
