// CPU check of csrc/png_frame.hpp (the host half of the device PNG encoder): CRC-32 against known vectors and a bitwise reference,
// the Adler-32 combine against the serial sum over split buffers, the frame writer and the size bound against frames built here.
// Built with -fsanitize=address,undefined by tests/test_png_frame.py and run directly.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../panorama-opticalflow_amd/csrc/png_frame.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
  } while (0)

static uint32_t crc_bitwise(const uint8_t* p, size_t n) {
  uint32_t c = 0xffffffffu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
  }
  return ~c;
}
static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static std::vector<uint8_t> bytes(size_t n, uint32_t seed) {
  std::vector<uint8_t> v(n);
  for (auto& b : v) b = (uint8_t)rnd(seed);
  return v;
}
static uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

static void check_crc() {
  using png_frame::crc32;
  const auto s = [](const char* t) { return crc32(0, (const uint8_t*)t, strlen(t)); };
  CHECK(s("") == 0u);
  CHECK(s("a") == 0xE8B7BE43u);
  CHECK(s("123456789") == 0xCBF43926u);
  CHECK(s("IEND") == 0xAE426082u);
  CHECK(s("The quick brown fox jumps over the lazy dog") == 0x414FA339u);
  for (size_t n : {size_t(0), size_t(1), size_t(7), size_t(8), size_t(9), size_t(63), size_t(4099), size_t(100003)}) {
    const std::vector<uint8_t> v = bytes(n + 3, (uint32_t)n + 1);
    for (size_t off = 0; off < 3; ++off) {   // every alignment of the start
      CHECK(crc32(0, v.data() + off, n) == crc_bitwise(v.data() + off, n));
      const size_t cut = n / 3;              // the running form
      CHECK(crc32(crc32(0, v.data() + off, cut), v.data() + off + cut, n - cut) == crc_bitwise(v.data() + off, n));
    }
  }
}

static void check_adler() {
  using png_frame::adler32; using png_frame::adler32_combine;
  CHECK(adler32(1, (const uint8_t*)"", 0) == 1u);
  CHECK(adler32(1, (const uint8_t*)"Wikipedia", 9) == 0x11E60398u);
  const std::vector<uint8_t> ff(70000, 0xff);   // the sums wrap 65521 many times
  const std::vector<uint8_t> v = bytes(3 * png_frame::kSegBytes + 17, 99);
  for (const std::vector<uint8_t>* buf : {&v, &ff}) {
    const uint8_t* p = buf->data(); const size_t n = buf->size();
    const uint32_t whole = adler32(1, p, n);
    for (size_t cut : {size_t(0), size_t(1), size_t(2), size_t(5551), size_t(5552), size_t(5553), n / 2, n - 1, n}) {
      if (cut > n) continue;
      CHECK(adler32_combine(adler32(1, p, cut), adler32(1, p + cut, n - cut), n - cut) == whole);
      CHECK(adler32(adler32(1, p, cut), p + cut, n - cut) == whole);
    }
    // the encoder's use: a left fold over segments, from 1
    for (size_t seg : {size_t(1), size_t(64), png_frame::kSegBytes}) {
      uint32_t ad = 1;
      for (size_t at = 0; at < n; at += seg) { const size_t len = at + seg < n ? seg : n - at; ad = adler32_combine(ad, adler32(1, p + at, len), len); }
      CHECK(ad == whole);
    }
  }
  CHECK(adler32_combine(1, 1, 0) == 1u);
  CHECK(adler32_combine(0xFFF0FFF0u, 0xFFF0FFF0u, 0xFFFFFFFFFFull) == adler32_combine(0xFFF0FFF0u, 0xFFF0FFF0u, 0xFFFFFFFFFFull % 65521));
}

// the worst case the bound covers: every segment of `stream` as one stored block and the sync marker
static std::vector<uint8_t> stored_deflate(const std::vector<uint8_t>& stream) {
  std::vector<uint8_t> d;
  const size_t nseg = png_frame::segments(stream.size());
  for (size_t s = 0; s < nseg; ++s) {
    const size_t at = s * png_frame::kSegBytes, n = s + 1 < nseg ? png_frame::kSegBytes : stream.size() - at;
    const uint8_t h[5] = {0, (uint8_t)(n & 0xff), (uint8_t)(n >> 8), (uint8_t)(~n & 0xff), (uint8_t)((~n >> 8) & 0xff)};
    d.insert(d.end(), h, h + 5);
    d.insert(d.end(), stream.begin() + at, stream.begin() + at + n);
    const uint8_t m[5] = {(uint8_t)(s + 1 == nseg), 0, 0, 0xff, 0xff};
    d.insert(d.end(), m, m + 5);
  }
  return d;
}

// frame `deflate` the way the library does and take the file apart again
static void check_frame(int cols, int rows, const std::vector<uint8_t>& deflate, uint32_t adler, size_t idat_max) {
  const png_frame::Frame fr(cols, rows, deflate.size(), idat_max);
  std::vector<uint8_t> file(fr.file_size() + 8, 0xA5);   // 8 guard bytes behind the file
  fr.write_head(file.data());
  for (size_t d = 0; d < deflate.size();) {
    size_t run = 0;
    const size_t at = fr.deflate_run(d, deflate.size() - d, &run);
    CHECK(run > 0 && at + run <= fr.file_size());
    if (!run) return;
    memcpy(file.data() + at, deflate.data() + d, run);
    d += run;
  }
  fr.write_tail(file.data(), adler);
  for (size_t i = 0; i < 8; ++i) CHECK(file[fr.file_size() + i] == 0xA5);
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  CHECK(memcmp(file.data(), sig, 8) == 0);
  std::vector<uint8_t> z;
  size_t pos = 8, nchunk = 0;
  bool ended = false;
  while (pos + 12 <= fr.file_size() && !ended) {
    const size_t len = be32(&file[pos]);
    CHECK(pos + 12 + len <= fr.file_size());
    if (pos + 12 + len > fr.file_size()) return;
    const std::string type((const char*)&file[pos + 4], 4);
    CHECK(be32(&file[pos + 8 + len]) == crc_bitwise(&file[pos + 4], len + 4));
    if (nchunk == 0) {
      CHECK(type == "IHDR" && len == 13);
      CHECK(be32(&file[pos + 8]) == (uint32_t)cols && be32(&file[pos + 12]) == (uint32_t)rows);
      CHECK(file[pos + 16] == 8 && file[pos + 17] == 6 && file[pos + 18] == 0 && file[pos + 19] == 0 && file[pos + 20] == 0);
    } else if (type == "IDAT") {
      CHECK(len >= 1 && len <= idat_max);
      z.insert(z.end(), &file[pos + 8], &file[pos + 8] + len);
    } else {
      CHECK(type == "IEND" && len == 0);
      ended = true;
    }
    pos += 12 + len; ++nchunk;
  }
  CHECK(ended && pos == fr.file_size());
  CHECK(nchunk == 2 + fr.idat_chunks());
  CHECK(z.size() == deflate.size() + 6);
  if (z.size() != deflate.size() + 6) return;
  CHECK(z[0] == 0x78 && ((z[0] << 8 | z[1]) % 31) == 0 && (z[1] & 0x20) == 0);
  CHECK(deflate.empty() || memcmp(z.data() + 2, deflate.data(), deflate.size()) == 0);
  CHECK(be32(&z[z.size() - 4]) == adler);
}

static void check_frames_and_bound() {
  using namespace png_frame;
  CHECK(kSegBytes % 4 == 0 && kSegSlot % 4 == 0 && kSegSlot >= kSegBytes + kSegOverhead);
  CHECK(segments(1) == 1 && segments(kSegBytes) == 1 && segments(kSegBytes + 1) == 2);
  const int shapes[][2] = {{1, 1}, {1, 5}, {7, 1}, {16, 251}, {16, 252}, {16, 253}, {16, 504}, {16, 505}, {300, 200}};
  for (const auto& sh : shapes) {
    const int cols = sh[0], rows = sh[1];
    const std::vector<uint8_t> stream = bytes(stream_bytes(cols, rows), cols * 31 + rows);
    CHECK(stream.size() == size_t(rows) * (4 * size_t(cols) + 1));
    const std::vector<uint8_t> worst = stored_deflate(stream);
    CHECK(worst.size() == deflate_bound(stream.size()));
    CHECK(Frame(cols, rows, worst.size()).file_size() == bound(cols, rows));   // the bound is reached by the all-stored stream, never exceeded
    const uint32_t ad = adler32(1, stream.data(), stream.size());
    check_frame(cols, rows, worst, ad, kIdatMax);
    // several IDAT chunks, with boundaries inside the zlib header, the data and the Adler-32
    for (size_t idat_max : {size_t(1), size_t(2), size_t(5), size_t(4096), worst.size() + 5, worst.size() + 6}) {
      check_frame(cols, rows, worst, ad, idat_max);
      CHECK(Frame(cols, rows, worst.size(), idat_max).file_size() == 8 + 25 + worst.size() + 6 + 12 * ((worst.size() + 6 + idat_max - 1) / idat_max) + 12);
    }
    const std::vector<uint8_t> small(worst.begin(), worst.begin() + worst.size() / 3);   // any shorter stream fits the bound
    CHECK(Frame(cols, rows, small.size()).file_size() <= bound(cols, rows));
    check_frame(cols, rows, small, 0x12345678u, kIdatMax);
  }
  check_frame(3, 2, std::vector<uint8_t>(), 1, kIdatMax);   // an empty deflate stream still frames (header and Adler only)
  // a canvas of the largest accepted pixel count: 64-bit sizes, several IDAT chunks
  const size_t big = stream_bytes(50000, 40000);
  CHECK(big == size_t(40000) * 200001);
  CHECK(Frame(50000, 40000, deflate_bound(big)).idat_chunks() == (deflate_bound(big) + 6 + kIdatMax - 1) / kIdatMax);
  CHECK(bound(50000, 40000) > big);
}

int main() {
  check_crc();
  check_adler();
  check_frames_and_bound();
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}
