// Stand-alone robustness check of the host entropy decoder (jpeg_entropy.cpp):
// feeds it truncated and corrupted copies of a valid stream and requires a
// clean return (success or a negative code) every time. Meant to be compiled
// together with jpeg_entropy.cpp under -fsanitize=address,undefined and run
// directly:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       jpeg_entropy.cpp bench/jpeg_entropy_check.cpp -lpthread -o check
//   ./check stream.mjpeg [sampling]
//
// sampling: 0 4:2:0, 1 4:2:2, 2 4:4:4, which must be the stream's (default:
// whatever its first frame has). The truncation and corruption loops then run
// through the entry points that carry the sampling.
//
// Every input lives in an exactly-sized heap buffer, so a read one byte past
// the data is a sanitizer report. Exit status 0: all calls returned cleanly.
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
}

static int g_sampling = 0;

static uint32_t rng_state = 0x1234567u;
static uint32_t rng() {                       // xorshift32
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

// index + decode a copy of `bytes` placed in a heap block of exactly that size
static int run(const std::vector<uint8_t>& bytes, long long record_bytes, int* ok, int* refused) {
  uint8_t* data = new uint8_t[bytes.size() ? bytes.size() : 1];
  if (!bytes.empty()) memcpy(data, bytes.data(), bytes.size());
  const long long len = (long long)bytes.size();
  int info[5];
  long long off = 0, flen = len;
  const long long n = rnb_mjpeg_index_s(data, len, &off, &flen, 1, info);
  // decode whatever the frame claims to be, whether or not the index accepted it
  if (n <= 0) { off = 0; flen = len; }
  uint8_t* rec = new uint8_t[record_bytes];
  const int rc = rnb_jpeg_decode_frames_s(data, len, &off, &flen, 1, rec, record_bytes, 1,
                                          g_sampling);
  delete[] rec;
  delete[] data;
  if (rc > 0) return 1;
  if (rc == 0) ++*ok; else ++*refused;
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s stream.mjpeg [sampling]\n", argv[0]);
    return 2;
  }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  std::vector<uint8_t> file;
  uint8_t chunk[4096];
  size_t got;
  while ((got = fread(chunk, 1, sizeof chunk, fp)) > 0) file.insert(file.end(), chunk, chunk + got);
  fclose(fp);
  int info[5];
  long long off = 0, flen = 0;
  const long long n = rnb_mjpeg_index_s(file.data(), (long long)file.size(), &off, &flen, 1, info);
  if (n < 1) { fprintf(stderr, "index of the intact stream failed: %lld\n", n); return 1; }
  g_sampling = info[4];
  if (argc > 2 && atoi(argv[2]) != g_sampling) {
    fprintf(stderr, "the stream's sampling is %d, not %s\n", g_sampling, argv[2]);
    return 2;
  }
  const std::vector<uint8_t> frame(file.begin() + off, file.begin() + off + flen);
  const int hs = g_sampling == 2 ? 1 : 2, vs = g_sampling == 0 ? 2 : 1;
  const long long mw = (info[0] + 8 * hs - 1) / (8 * hs), mh = (info[1] + 8 * vs - 1) / (8 * vs);
  const long long record_bytes = 384 + 128 * (hs * vs + 2) * mw * mh;
  int ok = 0, refused = 0;
  if (run(frame, record_bytes, &ok, &refused) || ok != 1) {
    fprintf(stderr, "the intact frame did not decode\n");
    return 1;
  }
  // 64 evenly spaced truncations
  for (int i = 0; i < 64; ++i) {
    const size_t cut = frame.size() * (size_t)i / 64;
    if (run(std::vector<uint8_t>(frame.begin(), frame.begin() + cut), record_bytes, &ok,
            &refused))
      return 1;
  }
  // 500 single-byte corruptions
  for (int i = 0; i < 500; ++i) {
    std::vector<uint8_t> bad(frame);
    bad[rng() % bad.size()] ^= (uint8_t)(1 + rng() % 255);
    if (run(bad, record_bytes, &ok, &refused)) return 1;
  }
  // the whole multi-frame stream cut inside its last frame, and a record too small
  if (file.size() > 8) {
    std::vector<uint8_t> cut(file.begin(), file.end() - 3);
    long long c = rnb_mjpeg_index_s(cut.data(), (long long)cut.size(), nullptr, nullptr, 0, info);
    if (c >= 0) { fprintf(stderr, "a stream without its last EOI was indexed\n"); return 1; }
  }
  {
    std::vector<uint8_t> rec((size_t)record_bytes - 16);
    const long long o = 0, l = (long long)frame.size();
    if (rnb_jpeg_decode_frames_s(frame.data(), l, &o, &l, 1, rec.data(), record_bytes - 16, 1,
                                 g_sampling) >= 0) {
      fprintf(stderr, "a short record was accepted\n");
      return 1;
    }
  }
  printf("jpeg_entropy_check: sampling %d: %d decoded, %d refused, no fault\n", g_sampling, ok,
         refused);
  return 0;
}
