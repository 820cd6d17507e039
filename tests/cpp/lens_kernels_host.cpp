// The lens remap kernel (csrc/kernels_lens.hip) run on the host, thread for thread, under the address and undefined-behaviour
// sanitizers: the photo, the canvases, the coordinate planes and both tables have exactly the sizes the library gives them, so a tap
// past the photo or an index past a table is caught here, without a GPU.  The tables are the library's own (csrc/reproject_math.hpp).
// The kernel has no barrier and no LDS, so a workgroup's threads run one after the other on one host thread.
// Argument: a list file of groups.  A group is a line
//   group N IN.bgra photo_cols photo_rows cols rows filter
// followed by N (1 .. 16) lens lines
//   model crop_cx256 crop_cy256 crop_r256 focal_px a b c dd shift_x shift_y min_cos rot0 .. rot8      (doubles as hex floats)
// and an output file that takes, per lens in the list's order, the canvas (cols * rows * 4 bytes), then the fx and the fy plane
// (int32 each).  A group's canvases come from ONE launch, a batch of N images (blockIdx.z) each under its own lens; a lens's
// coordinate planes come from a launch of its own without a destination.  Every launch has fewer workgroups than tiles where there
// are several, so the grid-stride walk runs.
// Built and run by tests/test_lens_kernels_host.py:  g++ -std=c++20 -fsanitize=address,undefined -Itests/cpp/hip_host_shim ...
#include <stdio.h>
#include <string.h>

#include <map>
#include <memory>
#include <string>

#include "../../panorama-opticalflow_amd/csrc/kernels_lens.hip"

using namespace pf;

static std::vector<uint32_t> read_file(const char* path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path, "rb");
  if (!f) return {};
  uint8_t buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
  fclose(f);
  std::vector<uint32_t> out(v.size() / 4);
  memcpy(out.data(), v.data(), out.size() * 4);
  return out;
}

static void launch(const LensArgs& a, unsigned grid_x, unsigned grid_z) {
  for (unsigned z = 0; z < grid_z; ++z)
    for (unsigned b = 0; b < grid_x; ++b)
      for (unsigned t = 0; t < (unsigned)kLnThreads; ++t) {
        threadIdx = dim3(t, 0, 0); blockIdx = dim3(b, 0, z); gridDim = dim3(grid_x, 1, grid_z);
        if (a.g.filter == reproject::kBicubic) k_lens_remap<reproject::kBicubic>(a); else k_lens_remap<reproject::kBilinear>(a);
      }
}

// an array of exactly n elements on the heap (no vector capacity behind it)
template <class T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }

int main(int argc, char** argv) {
  if (argc != 3) { printf("usage: %s CASES.txt OUT.bin\n", argv[0]); return 2; }
  FILE* list = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "wb");
  if (!list || !out) { printf("cannot open %s or %s\n", argv[1], argv[2]); return 2; }
  std::map<std::string, std::vector<uint32_t>> photos;
  char path[4096], num[17][64];
  int n, photo_cols, photo_rows, cols, rows, filter, n_cases = 0;
  while (fscanf(list, " group %d %4095s %d %d %d %d %d", &n, path, &photo_cols, &photo_rows, &cols, &rows, &filter) == 7) {
    if (!photos.count(path)) photos[path] = read_file(path);
    const std::vector<uint32_t>& file = photos[path];
    if (n < 1 || n > kMaxBatch || photo_cols <= 0 || photo_rows <= 0 || cols <= 0 || rows <= 0 || file.size() != size_t(photo_cols) * photo_rows) {
      printf("%s is not %d x %d BGRA, or a bad size or count\n", path, photo_cols, photo_rows);
      return 2;
    }
    const size_t px = size_t(photo_cols) * photo_rows, out_px = size_t(cols) * rows;
    auto src = exact<uint32_t>(px);
    memcpy(src.get(), file.data(), px * 4);
    LensArgs a;
    memset(&a, 0, sizeof a);
    a.g.filter = filter; a.g.photo_cols = photo_cols; a.g.photo_rows = photo_rows; a.g.cols = cols; a.g.rows = rows;
    auto eq = exact<double>(2 * (size_t(cols) + rows));
    reproject::make_equirect_tables(cols, rows, eq.get());
    a.eq = eq.get();
    auto cubic = exact<int>(1024);
    if (filter == reproject::kBicubic) { reproject::make_cubic_table(cubic.get()); a.cubic = cubic.get(); }
    std::unique_ptr<uint32_t[]> dst[kMaxBatch];
    for (int k = 0; k < n; ++k) {
      lens::Lens& l = a.lens[k];
      if (fscanf(list, "%d %d %d %d %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s", &l.model, &l.crop_cx256, &l.crop_cy256, &l.crop_r256,
                 num[0], num[1], num[2], num[3], num[4], num[5], num[6], num[7], num[8], num[9], num[10], num[11], num[12], num[13], num[14], num[15], num[16]) != 21) {
        printf("bad lens line in group of case %d\n", n_cases);
        return 2;
      }
      double v[17];
      for (int q = 0; q < 17; ++q) v[q] = strtod(num[q], nullptr);
      l.focal_px = v[0]; l.a = v[1]; l.b = v[2]; l.c = v[3]; l.dd = v[4]; l.shift_x = v[5]; l.shift_y = v[6]; l.min_cos = v[7];
      for (int q = 0; q < 9; ++q) l.rot[q] = v[8 + q];
      dst[k] = exact<uint32_t>(out_px);
      a.src[k] = src.get(); a.dst[k] = dst[k].get();
    }
    const unsigned tiles = ln_grid(cols, rows);
    const unsigned grid = tiles > 1 ? (tiles + 1) / 2 : 1;
    launch(a, grid, (unsigned)n);
    auto fx = exact<int>(out_px), fy = exact<int>(out_px);
    for (int k = 0; k < n; ++k) {
      LensArgs c = a;   // the lens alone, coordinates only
      c.lens[0] = a.lens[k]; c.src[0] = nullptr; c.dst[0] = nullptr; c.cubic = nullptr;
      c.fx_out = fx.get(); c.fy_out = fy.get();
      launch(c, grid, 1);
      if (fwrite(dst[k].get(), 4, out_px, out) != out_px || fwrite(fx.get(), 4, out_px, out) != out_px || fwrite(fy.get(), 4, out_px, out) != out_px) { printf("cannot write %s\n", argv[2]); return 2; }
      ++n_cases;
    }
  }
  fclose(list);
  if (fclose(out) != 0) { printf("cannot write %s\n", argv[2]); return 2; }
  printf("%d cases ok\n", n_cases);
  return 0;
}
