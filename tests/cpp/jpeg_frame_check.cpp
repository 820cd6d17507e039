// Host-only check of csrc/jpeg_frame.hpp, the framing of the device JPEG encoder: the header (SOI .. SOS) for every quality and both
// subsamplings against the header bytes of files libjpeg wrote (passed in by tests/test_jpeg_frame.py, which has Pillow write them), the
// bound's arithmetic at both ends of the format's range, the Huffman code tables, and the GPano XMP segment.
// Stand-alone, with its own main:  g++ -std=c++17 -fsanitize=address,undefined -o jpeg_frame_check jpeg_frame_check.cpp
// Arguments, in groups of `HEADER.bin cols rows quality subsampling restart`.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../panorama-opticalflow_amd/csrc/jpeg_frame.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
  } while (0)

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  uint8_t buf[4096];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  using namespace jpeg_frame;
  if ((argc - 1) % 6) { printf("usage: %s [HEADER.bin cols rows quality subsampling restart]...\n", argv[0]); return 2; }
  int headers = 0;
  for (int i = 1; i < argc; i += 6, ++headers) {
    const std::vector<uint8_t> want = read_file(argv[i]);
    const int cols = atoi(argv[i + 1]), rows = atoi(argv[i + 2]), quality = atoi(argv[i + 3]), sub = atoi(argv[i + 4]), restart = atoi(argv[i + 5]);
    std::vector<uint8_t> got(kHeadPlain);   // exactly the plain header's size
    const size_t n = write_head(cols, rows, quality, sub, restart, 0, got.data());
    CHECK(n == kHeadPlain && want.size() == n && memcmp(want.data(), got.data(), n) == 0);
    if (want.size() != n || memcmp(want.data(), got.data(), n) != 0) printf("  header of %dx%d quality %d subsampling %d differs\n", cols, rows, quality, sub);
  }
  printf("%d headers compared\n", headers);

  // ---- the bound: no overflow at either end, and it grows with the shape ----
  for (int sub = 0; sub < 2; ++sub) {
    const size_t one = bound(1, 1, sub), big = bound(kMaxSide, kMaxSide, sub);
    CHECK(one == kHeadMax + size_t(sub ? 6 : 3) * 416 + 4 + 2);
    const size_t side = sub ? 4096 : 8192;   // MCUs a side at 65535
    CHECK(mcus(kMaxSide, kMaxSide, sub) == side * side);
    CHECK(big == kHeadMax + side * side * (sub ? 6 : 3) * 416 + (side * side / restart_interval(sub)) * 4 + 2);
    CHECK(big > one && big > size_t(kMaxSide) * kMaxSide);
    CHECK(coef_bytes(kMaxSide, kMaxSide, sub) == side * side * (sub ? 6 : 3) * 128);
    CHECK(intervals(17 * 16, 17 * 16, 1, 32) == 10 && intervals(8, 8, sub, restart_interval(sub)) == 1);
  }
  CHECK(restart_interval(0) == 64 && restart_interval(1) == 32 && restart_interval(2) == 0);
  CHECK(size_t(kBlockBits + 7) / 8 == kBlockBytes);

  // ---- quality scaling at the ends ----
  uint8_t q[64];
  quant_table(kQuantLuma, 100, q);
  for (int k = 0; k < 64; ++k) CHECK(q[k] == 1);
  quant_table(kQuantLuma, 1, q);
  for (int k = 0; k < 64; ++k) CHECK(q[k] == 255);
  quant_table(kQuantChroma, 50, q);
  CHECK(memcmp(q, kQuantChroma, 64) == 0);

  // ---- the code tables: complete prefix codes over exactly the symbols of the DHTs ----
  Tables t;
  make_tables(90, &t);
  for (int c = 0; c < 2; ++c) {
    int n = 0;
    for (int s = 0; s < 256; ++s) {
      const uint32_t h = t.ac[c][s];
      if (!h) continue;
      ++n;
      CHECK((h & 31) >= 2 && (h & 31) <= 16 && (h >> 5) < (1u << (h & 31)));
      for (int o = 0; o < 256; ++o) {   // no code is the start of another
        const uint32_t g = t.ac[c][o];
        if (!g || o == s || (g & 31) < (h & 31)) continue;
        CHECK(((g >> 5) >> ((g & 31) - (h & 31))) != (h >> 5));
      }
    }
    CHECK(n == 162 && t.ac[c][0] && t.ac[c][0xF0]);
    for (int s = 0; s < 16; ++s) CHECK((t.dc[c][s] != 0) == (s < 12));
    for (int z = 0; z < 64; ++z) CHECK(t.unzig[kZigzag[z]] == z && t.qv[c][z] % 8 == 0 && t.qv[c][z] >= 8);
  }

  // ---- the XMP segment ----
  for (int cols : {2, 200, 9000, 65534}) {
    const int rows = cols / 2;
    std::vector<uint8_t> seg(4 + sizeof kXmpId + kXmpMax);
    const size_t n = write_xmp(cols, rows, seg.data());
    CHECK(n <= seg.size() && seg[0] == 0xFF && seg[1] == 0xE1);
    CHECK((size_t(seg[2]) << 8 | seg[3]) == n - 2);   // the length counts itself and not the marker
    CHECK(memcmp(seg.data() + 4, "http://ns.adobe.com/xap/1.0/\0", 29) == 0);
    const std::string xmp((const char*)seg.data() + 4 + 29, n - 4 - 29);
    CHECK(xmp.size() < kXmpMax && xmp.find('\0') == std::string::npos);
    const std::string w = std::to_string(cols), h = std::to_string(rows);
    for (const std::string& f : {std::string("GPano:ProjectionType=\"equirectangular\""), std::string("GPano:UsePanoramaViewer=\"True\""),
                                 "GPano:FullPanoWidthPixels=\"" + w + "\"", "GPano:FullPanoHeightPixels=\"" + h + "\"",
                                 "GPano:CroppedAreaImageWidthPixels=\"" + w + "\"", "GPano:CroppedAreaImageHeightPixels=\"" + h + "\"",
                                 std::string("GPano:CroppedAreaLeftPixels=\"0\""), std::string("GPano:CroppedAreaTopPixels=\"0\"")})
      CHECK(xmp.find(f) != std::string::npos);
    CHECK(xmp.rfind("</x:xmpmeta>") == xmp.size() - 12);
    // with the segment the header is the plain one with it spliced in behind APP0
    std::vector<uint8_t> plain(kHeadMax), pano(kHeadMax);
    const size_t np = write_head(cols, rows, 90, 1, 32, 0, plain.data()), ng = write_head(cols, rows, 90, 1, 32, 1, pano.data());
    CHECK(ng == np + n && ng <= kHeadMax);
    CHECK(memcmp(pano.data(), plain.data(), 20) == 0 && memcmp(pano.data() + 20, seg.data(), n) == 0 && memcmp(pano.data() + 20 + n, plain.data() + 20, np - 20) == 0);
  }
  uint8_t eoi[2];
  write_eoi(eoi);
  CHECK(eoi[0] == 0xFF && eoi[1] == 0xD9);

  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}
