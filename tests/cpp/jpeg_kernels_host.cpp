// The JPEG encoder's kernels (csrc/kernels_jpeg.hip) run on the host, thread for thread, under the address and undefined-behaviour
// sanitizers: every buffer has exactly the size the library gives it (the packed segment: exactly the length the size pass found), so an
// index past the image, the coefficients, an interval's place or an LDS array is caught here, without a GPU.
// Arguments, in groups of `IN.bgra cols rows quality subsampling restart OUT.jpg`: each raw BGRA file is encoded by the kernels at that
// restart interval (any that jpeg_restart_fits admits) and framed as the library frames it (csrc/jpeg_frame.hpp), for the byte
// comparison with the serial model (tests/jpeg_model.py).  The one argument `scan`: k_jpeg_scan alone, on size arrays of up to five
// elements per thread and values up to 2^32 - 1, against a serial prefix sum.
// Built and run by tests/test_jpeg_kernels_host.py:  g++ -std=c++20 -fsanitize=address,undefined -Itests/cpp/hip_host_shim ... -pthread
#include <stdio.h>
#include <string.h>

#include "../../panorama-opticalflow_amd/csrc/kernels_jpeg.hip"

using namespace pf;

static std::vector<uint8_t> read_file(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

static std::vector<uint8_t> encode_file(const std::vector<uint8_t>& img, int cols, int rows, int quality, int sub, int restart) {
  const size_t nint = jpeg_frame::intervals(cols, rows, sub, restart), nmcu = jpeg_frame::mcus(cols, rows, sub);
  const int mc = (int)jpeg_frame::mcu_cols(cols, sub), mr = (int)jpeg_frame::mcu_cols(rows, sub);
  const int tile_mcus = sub ? 16 : 32, tiles_x = (mc + tile_mcus - 1) / tile_mcus;
  std::vector<jpeg_frame::Tables> tab(1);
  jpeg_frame::make_tables(quality, tab.data());
  std::vector<int16_t> coef(jpeg_frame::coef_bytes(cols, rows, sub) / 2);
  std::vector<unsigned> sizes(nint);
  std::vector<unsigned long long> offs(nint + 1);
  host_shim_launch(k_jpeg_blocks, (unsigned)(tiles_x * mr), (unsigned)kBlkThreads, (const uint32_t*)img.data(), cols, rows, sub, mc, tiles_x,
                   (const jpeg_frame::Tables*)tab.data(), coef.data());
  host_shim_launch(k_jpeg_size, (unsigned)nint, (unsigned)kEntThreads, (const int16_t*)coef.data(), (unsigned long long)nmcu, sub, restart,
                   (const jpeg_frame::Tables*)tab.data(), sizes.data());
  host_shim_launch(k_jpeg_scan, 1u, 1024u, (const unsigned*)sizes.data(), (int)nint, offs.data());
  // (the bound is the product interval's, as in the library)
  if (restart == jpeg_frame::restart_interval(sub) && offs[nint] > jpeg_frame::scan_bound(cols, rows, sub)) { printf("FAIL: the segment exceeds its bound\n"); return {}; }
  std::vector<uint8_t> packed(offs[nint]);
  host_shim_launch(k_jpeg_write, (unsigned)nint, (unsigned)kEntThreads, (const int16_t*)coef.data(), (unsigned long long)nmcu, sub, restart,
                   (const jpeg_frame::Tables*)tab.data(), (const unsigned long long*)offs.data(), packed.data());
  std::vector<uint8_t> head(jpeg_frame::kHeadMax);
  head.resize(jpeg_frame::write_head(cols, rows, quality, sub, restart, 0, head.data()));
  std::vector<uint8_t> file(head);
  file.insert(file.end(), packed.begin(), packed.end());
  file.resize(file.size() + 2);
  jpeg_frame::write_eoi(file.data() + file.size() - 2);
  return file;
}

static uint32_t rnd(uint32_t& s) { s = s * 1664525u + 1013904223u; return s; }

// k_jpeg_scan on n sizes, buffers at their exact lengths: a thread sums ceil(n / 1024) of them
static int check_scan() {
  int fail = 0;
  for (int n : {1, 1023, 1024, 1025, 2048, 2049, 5000}) {
    uint32_t seed = 77u + (uint32_t)n;
    std::vector<unsigned> sizes(n);
    for (int i = 0; i < n; ++i) sizes[i] = i % 5 == 0 ? 0xffffffffu : i % 7 == 0 ? 0u : rnd(seed);   // sums beyond 32 bits from the second element on
    std::vector<unsigned long long> offs(n + 1, 0xA5A5A5A5A5A5A5A5ull);
    host_shim_launch(k_jpeg_scan, 1u, 1024u, (const unsigned*)sizes.data(), n, offs.data());
    unsigned long long acc = 0;
    int bad = 0;
    for (int i = 0; i < n; ++i) { bad += offs[i] != acc; acc += sizes[i]; }
    bad += offs[n] != acc;
    if (bad) { printf("FAIL: k_jpeg_scan, n = %d: %d of %d offsets are not the serial prefix sum\n", n, bad, n + 1); ++fail; }
    else printf("  k_jpeg_scan n = %d (%d per thread): total %llu\n", n, (n + 1023) / 1024, acc);
  }
  if (fail) return 1;
  printf("ok\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "scan")) return check_scan();
  if (argc < 2 || (argc - 1) % 7) { printf("usage: %s scan | [IN.bgra cols rows quality subsampling restart OUT.jpg]...\n", argv[0]); return 2; }
  for (int i = 1; i < argc; i += 7) {
    const int cols = atoi(argv[i + 1]), rows = atoi(argv[i + 2]), quality = atoi(argv[i + 3]), sub = atoi(argv[i + 4]), restart = atoi(argv[i + 5]);
    if ((sub != 0 && sub != 1) || !jpeg_restart_fits(sub, restart)) { printf("a restart interval of %d MCUs at subsampling %d does not fit the coder\n", restart, sub); return 2; }
    const std::vector<uint8_t> img = read_file(argv[i]);
    if (cols <= 0 || rows <= 0 || img.size() != size_t(cols) * rows * 4) { printf("%s is not %d x %d BGRA\n", argv[i], cols, rows); return 2; }
    const std::vector<uint8_t> file = encode_file(img, cols, rows, quality, sub, restart);
    if (file.empty()) return 1;
    FILE* f = fopen(argv[i + 6], "wb");
    if (!f || fwrite(file.data(), 1, file.size(), f) != file.size()) { printf("cannot write %s\n", argv[i + 6]); return 2; }
    fclose(f);
  }
  printf("ok\n");
  return 0;
}
