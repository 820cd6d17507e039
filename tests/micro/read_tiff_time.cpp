// The host reader's time for one TIFF (tools/image_io.hpp read_tiff: file read, serial strip decode, predictor, swizzle), the baseline of
// tests/micro/tiff_device_ab.py.  usage: read_tiff_time FILE [runs]; prints one line of seconds per run and a checksum of the pixels.
//   g++ -O2 -std=c++17 -o read_tiff_time tests/micro/read_tiff_time.cpp -lz
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "../../panorama-opticalflow_amd/tools/image_io.hpp"

int main(int argc, char** argv) {
  if (argc < 2) { printf("usage: %s FILE [runs]\n", argv[0]); return 2; }
  const int runs = argc > 2 ? atoi(argv[2]) : 1;
  try {
    for (int r = 0; r < runs; ++r) {
      const auto t0 = std::chrono::steady_clock::now();
      const panocv::Mat m = pano_io::read_tiff(argv[1]);
      const auto t1 = std::chrono::steady_clock::now();
      unsigned long long sum = 0;
      for (int y = 0; y < m.rows; y += 97) for (int x = 0; x < m.cols * 4; x += 13) sum = sum * 31 + m.data[size_t(y) * m.step + x];
      printf("%.4f %dx%d %llx\n", std::chrono::duration<double>(t1 - t0).count(), m.cols, m.rows, sum);
    }
  } catch (const util::VrCamException& e) { printf("error: %s\n", e.what()); return 1; }
  return 0;
}
