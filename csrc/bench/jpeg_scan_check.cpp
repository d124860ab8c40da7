// Stand-alone check of the scan packer and the interval decoder that the GPU
// kernel shares with the host (jpeg_huff.h, through rnb_jpeg_pack_scans and
// rnb_jpeg_decode_scans_host in jpeg_entropy.cpp). Meant to be compiled
// together with jpeg_entropy.cpp under -fsanitize=address,undefined and run
// directly:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       jpeg_entropy.cpp bench/jpeg_scan_check.cpp -lpthread -o check
//   ./check [--sampling N] stream.mjpeg
//
// N: 0 4:2:0, 1 4:2:2, 2 4:4:4, which must be the stream's (default: whatever
// its first frame has); everything below runs through the entry points that
// carry the sampling, and the scan record corruptions include its sampling word.
//
// For every frame of the stream: pack + interval decode must equal
// rnb_jpeg_decode_frames. Then, on the first frame: every truncation length
// and 3000 single-byte corruptions of the STREAM go through the packer (and
// the interval decoder where the packer accepts), and must be accepted or
// refused as rnb_jpeg_decode_frames accepts or refuses them, with equal
// records where both accept; and 4000 single-byte corruptions of the PACKED
// SCAN RECORD (tables, counts, header, span table, scan bytes) go straight
// into the interval decoder, twice, and must give the same status and record
// both times. Every buffer is a heap block of exactly its size, so a read or
// write one byte outside is a sanitizer report. Exit status 0 and "no fault":
// all of that held.
//
//   ./check [--sampling N] --records W H record.bin ...
// runs the interval decoder, twice, on each file as one scan record of a
// W x H frame of sampling N (default 0) (the fixed damaged records that the GPU tests then give the
// kernel) and prints each status.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

extern "C" {
long long rnb_mjpeg_index_s(const uint8_t* data, long long len, long long* offs, long long* lens,
                            long long cap, int* info);
int rnb_jpeg_decode_frames_s(const uint8_t* data, long long len, const long long* frame_offs,
                             const long long* frame_lens, int nframes, uint8_t* out,
                             long long record_bytes, int threads, int sampling);
long long rnb_jpeg_pack_scans_s(const uint8_t* data, long long len, const long long* frame_offs,
                                const long long* frame_lens, int nframes, uint8_t* out,
                                long long out_cap, long long* scan_offs, int want_w, int want_h,
                                int* info, int sampling);
int rnb_jpeg_decode_scans_host_s(const uint8_t* scans, long long scans_len,
                                 const long long* scan_offs, int nframes, int mw, int mh,
                                 uint8_t* out, long long out_len, long long record_bytes,
                                 int* status, int sampling);
}

static uint32_t rng_state = 0x2468ACEu;
static uint32_t rng() {                       // xorshift32
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

static int g_mw, g_mh, g_w, g_h, g_sampling;
static long long g_record_bytes;
static int g_resized = 0;        // disagreements on a frame whose header announces another size

// MCU grid and record size of a g_w x g_h frame of g_sampling
static void set_geometry() {
  const int hs = g_sampling == 2 ? 1 : 2, vs = g_sampling == 0 ? 2 : 1;
  g_mw = (g_w + 8 * hs - 1) / (8 * hs);
  g_mh = (g_h + 8 * vs - 1) / (8 * vs);
  g_record_bytes = 384 + 128LL * (hs * vs + 2) * g_mw * g_mh;
}

// a heap block of exactly n bytes holding src (operator new aligns to 16)
static uint8_t* exact(const uint8_t* src, size_t n) {
  uint8_t* p = new uint8_t[n ? n : 1];
  if (n) memcpy(p, src, n);
  return p;
}

// the host decoder's verdict on one frame's bytes; rec receives its record
static int host_decode(const std::vector<uint8_t>& bytes, std::vector<uint8_t>& rec) {
  uint8_t* data = exact(bytes.data(), bytes.size());
  const long long off = 0, len = (long long)bytes.size();
  uint8_t* out = new uint8_t[g_record_bytes];
  const int rc = rnb_jpeg_decode_frames_s(data, len, &off, &len, 1, out, g_record_bytes, 1,
                                          g_sampling);
  rec.assign(out, out + g_record_bytes);
  delete[] out;
  delete[] data;
  return rc;
}

// pack one frame's bytes into an exact-size scan record; < 0: the packer's refusal
static long long pack(const std::vector<uint8_t>& bytes, std::vector<uint8_t>& scans) {
  uint8_t* data = exact(bytes.data(), bytes.size());
  const long long off = 0, len = (long long)bytes.size();
  const long long cap = (2048 + 8LL * g_mw * g_mh + len + 31) & ~15LL;
  uint8_t* out = new uint8_t[cap];
  long long offs[2];
  int info[3];
  const long long n = rnb_jpeg_pack_scans_s(data, len, &off, &len, 1, out, cap, offs, g_w, g_h,
                                            info, g_sampling);
  if (n >= 0) {
    if (offs[0] != 0 || offs[1] != n || n % 16 != 0 || n > cap) {
      fprintf(stderr, "the packer's offsets do not fit what it wrote\n");
      delete[] out;
      delete[] data;
      return 1LL << 40;
    }
    scans.assign(out, out + n);
  }
  delete[] out;
  delete[] data;
  return n;
}

// the interval decoder on one exact-size scan record; returns the launcher-level code
static int mirror(const std::vector<uint8_t>& scans, std::vector<uint8_t>& rec, int* status) {
  uint8_t* s = exact(scans.data(), scans.size());
  uint8_t* out = new uint8_t[g_record_bytes];
  memset(out, 0xA5, (size_t)g_record_bytes);
  const long long offs[2] = {0, (long long)scans.size()};
  *status = 12345;
  const int rc = rnb_jpeg_decode_scans_host_s(s, (long long)scans.size(), offs, 1, g_mw, g_mh, out,
                                              g_record_bytes, g_record_bytes, status, g_sampling);
  rec.assign(out, out + g_record_bytes);
  delete[] out;
  delete[] s;
  return rc;
}

// one (possibly damaged) frame through both paths: equal verdicts, equal records
static int compare_paths(const std::vector<uint8_t>& bytes, int* ok, int* refused,
                         const char* what, long long which) {
  std::vector<uint8_t> want, scans, got;
  const int host_rc = host_decode(bytes, want);
  if (host_rc > 0) return 1;
  const long long n = pack(bytes, scans);
  if (n >= (1LL << 40)) return 1;
  bool accepted = false;
  if (n >= 0) {
    int status = 0;
    if (mirror(scans, got, &status) != 0) {
      fprintf(stderr, "%s %lld: the interval decoder refused what the packer wrote\n", what, which);
      return 1;
    }
    if (status > 0) return 1;
    accepted = status == 0;
  }
  if (accepted != (host_rc == 0)) {
    // Damage to the size in the frame header: the frame decoder is given one
    // frame and takes its size from that header (it decodes the MCUs the header
    // announces), the packer is told the stream's size and refuses another. The
    // two were not asked the same question then; both returned cleanly.
    int info[5];
    long long o = 0, l = 0;
    uint8_t* data = exact(bytes.data(), bytes.size());
    const long long c = rnb_mjpeg_index_s(data, (long long)bytes.size(), &o, &l, 1, info);
    delete[] data;
    if (c >= 1 && (info[0] != g_w || info[1] != g_h)) {
      ++g_resized;
      return 0;
    }
    fprintf(stderr, "%s %lld: host decoder %d, packed path %s\n", what, which, host_rc,
            accepted ? "accepts" : "refuses");
    return 1;
  }
  if (accepted && got != want) {
    fprintf(stderr, "%s %lld: both accept, records differ\n", what, which);
    return 1;
  }
  ++*(accepted ? ok : refused);
  return 0;
}

static bool read_file(const char* path, std::vector<uint8_t>& file) {
  FILE* fp = fopen(path, "rb");
  if (!fp) { perror(path); return false; }
  uint8_t chunk[4096];
  size_t got;
  while ((got = fread(chunk, 1, sizeof chunk, fp)) > 0) file.insert(file.end(), chunk, chunk + got);
  fclose(fp);
  return true;
}

// --records W H file...: each file is one (damaged) scan record of a W x H
// frame; run the interval decoder on each, twice, and print its status
static int check_records(int argc, char** argv) {
  g_w = atoi(argv[2]); g_h = atoi(argv[3]);
  if (g_w < 1 || g_h < 1 || g_w > 65535 || g_h > 65535) return 2;
  set_geometry();
  for (int i = 4; i < argc; ++i) {
    std::vector<uint8_t> scans, r1, r2;
    if (!read_file(argv[i], scans)) return 2;
    int s1 = 0, s2 = 0;
    const int c1 = mirror(scans, r1, &s1), c2 = mirror(scans, r2, &s2);
    if (c1 != c2 || s1 != s2 || s1 > 0 || r1 != r2) {
      fprintf(stderr, "%s: codes %d %d, status %d %d\n", argv[i], c1, c2, s1, s2);
      return 1;
    }
    printf("%s: code %d status %d\n", argv[i], c1, s1);
  }
  printf("jpeg_scan_check: %d scan records, no fault\n", argc - 4);
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
  if (argc != 2) {
    fprintf(stderr, "usage: %s [--sampling N] stream.mjpeg | --records W H record...\n", argv[0]);
    return 2;
  }
  std::vector<uint8_t> file;
  if (!read_file(argv[1], file)) return 2;
  int info[5];
  long long count = rnb_mjpeg_index_s(file.data(), (long long)file.size(), nullptr, nullptr, 0,
                                      info);
  if (count < 1) { fprintf(stderr, "index of the intact stream failed: %lld\n", count); return 1; }
  std::vector<long long> offs((size_t)count), lens((size_t)count);
  count = rnb_mjpeg_index_s(file.data(), (long long)file.size(), offs.data(), lens.data(), count,
                            info);
  g_w = info[0]; g_h = info[1];
  if (want_sampling >= 0 && want_sampling != info[4]) {
    fprintf(stderr, "the stream's sampling is %d, not %d\n", info[4], want_sampling);
    return 2;
  }
  g_sampling = info[4];
  set_geometry();
  int ok = 0, refused = 0;
  // 1. every intact frame
  for (long long i = 0; i < count; ++i) {
    const std::vector<uint8_t> frame(file.begin() + offs[(size_t)i],
                                     file.begin() + offs[(size_t)i] + lens[(size_t)i]);
    if (compare_paths(frame, &ok, &refused, "frame", i)) return 1;
  }
  if (ok != count) { fprintf(stderr, "an intact frame did not decode\n"); return 1; }
  const std::vector<uint8_t> frame(file.begin() + offs[0], file.begin() + offs[0] + lens[0]);
  // 2. every truncation length of the stream's first frame
  for (size_t cut = 0; cut < frame.size(); ++cut)
    if (compare_paths(std::vector<uint8_t>(frame.begin(), frame.begin() + cut), &ok, &refused,
                      "truncation", (long long)cut))
      return 1;
  // 3. single-byte corruptions of the stream
  for (int i = 0; i < 3000; ++i) {
    std::vector<uint8_t> bad(frame);
    bad[rng() % bad.size()] ^= (uint8_t)(1 + rng() % 255);
    if (compare_paths(bad, &ok, &refused, "corruption", i)) return 1;
  }
  // 4. single-byte corruptions of the packed scan record, straight into the
  // interval decoder: header fields, table counts and the span table included
  std::vector<uint8_t> scans;
  if (pack(frame, scans) < 0) return 1;
  int rec_ok = 0, rec_bad = 0;
  for (int i = 0; i < 4000; ++i) {
    std::vector<uint8_t> bad(scans);
    // every other case inside the 16-byte header and the span table
    size_t at = rng() % bad.size();
    if (i % 2) at = 2016 + rng() % (16 + 8 * (bad.size() > 2112 ? 10 : 1));
    if (i % 8 == 3) at = 384 + 272 * (rng() % 6) + rng() % 16;      // a table's counts
    if (at >= bad.size()) at = bad.size() - 1;
    bad[at] ^= (uint8_t)(1 + rng() % 255);
    std::vector<uint8_t> r1, r2;
    int s1 = 0, s2 = 0;
    const int c1 = mirror(bad, r1, &s1), c2 = mirror(bad, r2, &s2);
    if (c1 != 0 || c2 != 0 || s1 > 0 || s1 != s2 || r1 != r2) {
      fprintf(stderr, "scan record corruption %d at %zu: codes %d %d, status %d %d\n", i, at, c1,
              c2, s1, s2);
      return 1;
    }
    ++*(s1 == 0 ? &rec_ok : &rec_bad);
  }
  // 5. buffer-level refusals of the interval decoder and the packer's out_cap
  {
    std::vector<uint8_t> rec((size_t)g_record_bytes);
    int status = 0;
    const long long o[2] = {0, (long long)scans.size()};
    const long long past[2] = {0, (long long)scans.size() + 16};
    if (rnb_jpeg_decode_scans_host_s(scans.data(), (long long)scans.size(), past, 1, g_mw, g_mh,
                                     rec.data(), g_record_bytes, g_record_bytes, &status,
                                     g_sampling) >= 0 ||
        rnb_jpeg_decode_scans_host_s(scans.data(), (long long)scans.size(), o, 1, g_mw, g_mh,
                                     rec.data(), g_record_bytes - 16, g_record_bytes, &status,
                                     g_sampling) >= 0) {
      fprintf(stderr, "a scan record / frame record outside its buffer was accepted\n");
      return 1;
    }
    uint8_t* out = new uint8_t[scans.size() - 16];
    const long long off = 0, len = (long long)frame.size();
    long long so[2];
    int pinfo[3];
    if (rnb_jpeg_pack_scans_s(frame.data(), len, &off, &len, 1, out, (long long)scans.size() - 16,
                              so, 0, 0, pinfo, g_sampling) >= 0) {
      fprintf(stderr, "a short out_cap was accepted\n");
      return 1;
    }
    delete[] out;
  }
  printf("jpeg_scan_check: sampling %d: %d streams accepted by both paths, %d refused by both, "
         "%d apart on a damaged size; %d damaged scan records decoded, %d refused; no fault\n",
         g_sampling, ok, refused, g_resized, rec_ok, rec_bad);
  return 0;
}
