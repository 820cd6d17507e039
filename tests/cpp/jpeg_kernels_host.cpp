// The JPEG encoder's kernels (csrc/kernels_jpeg.hip) run on the host, thread for thread, under the address and undefined-behaviour
// sanitizers: every buffer has exactly the size the library gives it (the packed segment: exactly the length the size pass found), so an
// index past the image, the coefficients, an interval's place or an LDS array is caught here, without a GPU.
// Arguments, in groups of `IN.bgra cols rows quality subsampling OUT.jpg`: each raw BGRA file is encoded by the kernels and framed as the
// library frames it (csrc/jpeg_frame.hpp), for the byte comparison with the serial model (tests/jpeg_model.py).
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

static std::vector<uint8_t> encode_file(const std::vector<uint8_t>& img, int cols, int rows, int quality, int sub) {
  const int restart = jpeg_frame::restart_interval(sub);
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
  if (offs[nint] > jpeg_frame::scan_bound(cols, rows, sub)) { printf("FAIL: the segment exceeds its bound\n"); return {}; }
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

int main(int argc, char** argv) {
  if (argc < 2 || (argc - 1) % 6) { printf("usage: %s [IN.bgra cols rows quality subsampling OUT.jpg]...\n", argv[0]); return 2; }
  for (int i = 1; i < argc; i += 6) {
    const int cols = atoi(argv[i + 1]), rows = atoi(argv[i + 2]), quality = atoi(argv[i + 3]), sub = atoi(argv[i + 4]);
    const std::vector<uint8_t> img = read_file(argv[i]);
    if (cols <= 0 || rows <= 0 || img.size() != size_t(cols) * rows * 4) { printf("%s is not %d x %d BGRA\n", argv[i], cols, rows); return 2; }
    const std::vector<uint8_t> file = encode_file(img, cols, rows, quality, sub);
    if (file.empty()) return 1;
    FILE* f = fopen(argv[i + 5], "wb");
    if (!f || fwrite(file.data(), 1, file.size(), f) != file.size()) { printf("cannot write %s\n", argv[i + 5]); return 2; }
    fclose(f);
  }
  printf("ok\n");
  return 0;
}
