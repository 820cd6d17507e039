// The PNG encoder's kernels (csrc/kernels_png.hip) run on the host, thread for thread, under the address and undefined-behaviour
// sanitizers: every buffer has exactly the size the library gives it, so an index past a segment, a slot or the stream is caught here,
// without a GPU.  Each file is then framed (csrc/png_frame.hpp), inflated with zlib, unfiltered and compared with the image.
// Built and run by tests/test_png_kernels_host.py:  g++ -std=c++20 -fsanitize=address,undefined -Itests/cpp/hip_host_shim ... -lz -pthread
#include <stdio.h>
#include <string.h>
#include <zlib.h>

#include "../../panorama-opticalflow_amd/csrc/kernels_png.hip"

using namespace pf;

static int g_fail = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_fail; } \
  } while (0)

static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

// 0 noise, 1 a gentle gradient, 2 constant zero, 3 constant (7, 7, 7, 255), 4 alpha noise over a flat colour, 5 noise rows between flat rows
static std::vector<uint8_t> make_image(int cols, int rows, int kind, uint32_t seed) {
  std::vector<uint8_t> v(size_t(cols) * rows * 4);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x) {
      uint8_t* p = &v[(size_t(y) * cols + x) * 4];
      for (int ch = 0; ch < 4; ++ch) {
        const uint8_t noise = (uint8_t)rnd(seed);
        const uint8_t flat[4] = {40, 90, 90, 200};
        switch (kind) {
          case 0: p[ch] = noise; break;
          case 1: p[ch] = (uint8_t)(3 * y + 2 * x + 50 * ch); break;
          case 2: p[ch] = 0; break;
          case 3: p[ch] = ch == 3 ? 255 : 7; break;
          case 4: p[ch] = ch == 3 ? noise : flat[ch]; break;
          default: p[ch] = (y / 7) % 2 ? noise : flat[ch]; break;
        }
      }
    }
  return v;
}

static int ref_paeth(int a, int b, int c) {   // the check's own predictor, not the kernel's
  const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

static void encode_and_check(int cols, int rows, int kind) {
  const std::vector<uint8_t> img = make_image(cols, rows, kind, cols * 131 + rows * 7 + kind);
  const size_t stream = png_frame::stream_bytes(cols, rows), nseg = png_frame::segments(stream);
  std::vector<uint8_t> st(png_stream_alloc_bytes(cols, rows)), slots(nseg * png_frame::kSegSlot), packed(png_frame::deflate_bound(stream));
  std::vector<unsigned> sizes(nseg), adler(nseg);
  std::vector<unsigned long long> offs(nseg + 1);
  host_shim_launch(k_png_filter, (unsigned)std::min(rows, 3), 256u, (const uint32_t*)img.data(), cols, rows, st.data());
  host_shim_launch(k_png_deflate, (unsigned)nseg, 256u, (const uint8_t*)st.data(), (unsigned long long)stream, slots.data(), sizes.data(), adler.data());
  host_shim_launch(k_png_scan, 1u, 1024u, (const unsigned*)sizes.data(), (int)nseg, offs.data());
  host_shim_launch(k_png_gather, (unsigned)nseg, 256u, (const uint8_t*)slots.data(), (const unsigned*)sizes.data(), (const unsigned long long*)offs.data(), packed.data());
  const size_t dlen = offs[nseg];
  CHECK(dlen <= png_frame::deflate_bound(stream));
  if (dlen > png_frame::deflate_bound(stream)) return;
  for (size_t s = 0; s < nseg; ++s) CHECK(sizes[s] <= std::min(png_frame::kSegBytes, stream - s * png_frame::kSegBytes) + png_frame::kSegOverhead);
  // the zlib stream as the library frames it
  const png_frame::Frame fr(cols, rows, dlen);
  std::vector<uint8_t> file(fr.file_size());
  fr.write_head(file.data());
  for (size_t d = 0; d < dlen;) { size_t run; const size_t at = fr.deflate_run(d, dlen - d, &run); memcpy(file.data() + at, packed.data() + d, run); d += run; }
  uint32_t ad = 1;
  for (size_t s = 0; s < nseg; ++s) ad = png_frame::adler32_combine(ad, adler[s], s + 1 < nseg ? png_frame::kSegBytes : stream - s * png_frame::kSegBytes);
  fr.write_tail(file.data(), ad);
  CHECK(file.size() <= png_frame::bound(cols, rows));
  // inflate (zlib checks the Adler-32), unfilter, compare
  std::vector<uint8_t> raw(stream);
  uLongf rn = (uLongf)raw.size();
  const int zr = uncompress(raw.data(), &rn, file.data() + fr.file_offset(0), (uLong)fr.zlib_len());
  CHECK(zr == Z_OK && rn == stream);
  if (zr != Z_OK || rn != stream) { printf("  %dx%d kind %d: zlib says %d\n", cols, rows, kind, zr); return; }
  CHECK(memcmp(raw.data(), st.data(), stream) == 0);
  const size_t stride = size_t(cols) * 4;
  std::vector<uint8_t> prev(stride, 0), cur(stride);
  size_t bad = 0;
  for (int y = 0; y < rows; ++y) {
    const uint8_t* r = raw.data() + size_t(y) * (stride + 1);
    const int ft = r[0];
    CHECK(ft <= 4);
    for (size_t i = 0; i < stride; ++i) {
      const int a = i >= 4 ? cur[i - 4] : 0, b = prev[i], c = i >= 4 ? prev[i - 4] : 0;
      int v = r[1 + i];
      if (ft == 1) v += a; else if (ft == 2) v += b; else if (ft == 3) v += (a + b) >> 1; else if (ft == 4) v += ref_paeth(a, b, c);
      cur[i] = (uint8_t)v;
    }
    const uint8_t* src = &img[size_t(y) * stride];
    for (int x = 0; x < cols; ++x)
      bad += cur[4 * x] != src[4 * x + 2] || cur[4 * x + 1] != src[4 * x + 1] || cur[4 * x + 2] != src[4 * x] || cur[4 * x + 3] != src[4 * x + 3];
    prev.swap(cur);
  }
  CHECK(bad == 0);
  printf("  %dx%d kind %d: %zu segments, file %zu bytes (%.4f of raw)\n", cols, rows, kind, nseg, file.size(), double(file.size()) / double(img.size()));
}

int main() {
  // (a barrier of 256 host threads is slow: few rows, and only the shapes at which an index can go wrong)
  const int cases[][3] = {{1, 1, 0}, {1, 5, 1}, {7, 1, 1}, {65, 3, 0}, {65, 3, 1},   // no neighbours; a row around 256 bytes
                          {341, 12, 0}, {341, 12, 1}, {341, 13, 1},                     // rows of 1365 bytes: exactly one segment, and a row more
                          {1366, 9, 4}, {1366, 9, 5}};                                  // four segments; runs across thread chunks and segment ends
  for (const auto& cs : cases) encode_and_check(cs[0], cs[1], cs[2]);
  encode_and_check(4099, 3, 2);   // matches of 258 end to end, a run longer than a segment
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("ok\n");
  return 0;
}
