// The device inflate kernel (csrc/kernels_tiff.hip k_tiff_inflate) and the finish kernel run on the host, thread for thread, under the
// address and undefined-behaviour sanitizers.  Every buffer has exactly the size the library gives it -- the file, the strip tables, the
// samples plane, the status words, the output -- so a read past a strip or the file, a copy source past the strip's bytes or a write past
// the plane is caught here, without a GPU.  Arguments, in groups of three: IN.tif OUT.bgra OUT.status.  Each deflate file is parsed
// (csrc/tiff_parse.hpp), decoded into a zeroed plane and written as raw BGRA; OUT.status gets one line per strip,
// "bytes_decoded expected reason".  The grid is smaller than the number of strips, so the kernel's stride over strips runs too.
// Built and run by tests/test_tiff_inflate_host.py:  g++ -std=c++20 -fsanitize=address,undefined -Itests/cpp/hip_host_shim ... -pthread
#include <stdio.h>
#include <string.h>

#include <memory>

// the one primitive the stand-in header lacks (the LZW kernel in the same source uses it)
inline unsigned atomicMin(unsigned* p, unsigned v) {
  unsigned old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (old > v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
  return old;
}

#include "../../panorama-opticalflow_amd/csrc/kernels_tiff.hip"
#include "../../panorama-opticalflow_amd/csrc/tiff_parse.hpp"

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

// exact-size heap blocks (a std::vector may round its capacity up; new[] of n bytes is n bytes to the sanitizer)
template <class T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]()); }

static int decode_one(const char* in, const char* out_bgra, const char* out_status) {
  const std::vector<uint8_t> data = read_file(in);
  tiff_parse::Info f;
  std::string why;
  if (!tiff_parse::parse(data.data(), data.size(), &f, &why)) { printf("%s: %s\n", in, why.c_str()); return 2; }
  if ((f.compression != 8 && f.compression != 32946) || tiff_parse::device_decodable(f) || !tiff_parse::device_decodable_with_inflate(f)) {
    printf("%s: not a deflate file the switch admits\n", in); return 2;
  }
  const size_t ns = f.n_strips(), plane_bytes = size_t(f.row_bytes()) * f.rows, px = size_t(f.cols) * f.rows;
  auto file = exact<uint8_t>(data.size());
  memcpy(file.get(), data.data(), data.size());
  auto offs = exact<uint32_t>(ns), cnts = exact<uint32_t>(ns);
  for (size_t s = 0; s < ns; ++s) { offs[s] = f.offsets[s]; cnts[s] = f.counts[s]; }
  auto plane = exact<uint8_t>(plane_bytes);
  auto status = exact<unsigned long long>(ns);
  auto bgra = exact<uint32_t>(px);
  TiffWork w;
  w.file = file.get(); w.bytes = data.size(); w.offsets = offs.get(); w.counts = cnts.get();
  w.n_strips = (int)ns; w.cols = (int)f.cols; w.rows = (int)f.rows; w.samples = (int)f.samples; w.rows_per_strip = (int)f.rows_per_strip; w.predictor = (int)f.predictor;
  w.plane = plane.get(); w.status = status.get();
  host_shim_launch(k_tiff_inflate, (unsigned)std::min<size_t>(ns, 3), (unsigned)kStripThreads, w);
  host_shim_launch(k_tiff_finish, (unsigned)std::min<uint32_t>(f.rows, 3), (unsigned)kRowThreads, w, 0, bgra.get());
  FILE* fo = fopen(out_bgra, "wb");
  if (!fo || fwrite(bgra.get(), 4, px, fo) != px) { printf("cannot write %s\n", out_bgra); return 2; }
  fclose(fo);
  fo = fopen(out_status, "w");
  if (!fo) { printf("cannot write %s\n", out_status); return 2; }
  for (size_t s = 0; s < ns; ++s) fprintf(fo, "%llu %llu %llu\n", status[s] & 0xffffffffull, (unsigned long long)f.strip_bytes(s), status[s] >> 32);
  fclose(fo);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 4 || (argc - 1) % 3) { printf("usage: %s IN.tif OUT.bgra OUT.status ...\n", argv[0]); return 2; }
  for (int i = 1; i < argc; i += 3)
    if (int e = decode_one(argv[i], argv[i + 1], argv[i + 2])) return e;
  printf("ok\n");
  return 0;
}
