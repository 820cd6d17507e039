// The reprojection kernel (csrc/kernels_reproject.hip) run on the host, thread for thread, under the address and undefined-behaviour
// sanitizers: the source, the outputs, the coordinate planes and both tables have exactly the sizes the library gives them, so a tap
// past the image or an index past a table is caught here, without a GPU.  The tables are the library's own (csrc/reproject_math.hpp).
// The kernel has no barrier and no LDS, so a workgroup's threads run one after the other on one host thread.
// Argument: a list file with one case per line,
//   IN.bgra cols rows out_cols out_rows projection face filter hfov rot0 .. rot8      (doubles as hex floats)
// and an output file that takes, per case, the image (out_cols * out_rows * 4 bytes), then the fx and the fy plane (int32 each).
// Every launch has fewer workgroups than tiles where there are several, so the grid-stride walk runs; the image is launched as a
// batch of two (blockIdx.z) whose results must agree.  A cube case runs as the one-launch set of six as well and its face must agree.
// Built and run by tests/test_reproject_kernels_host.py:  g++ -std=c++20 -fsanitize=address,undefined -Itests/cpp/hip_host_shim ...
#include <stdio.h>
#include <string.h>

#include <map>
#include <memory>
#include <string>

#include "../../panorama-opticalflow_amd/csrc/kernels_reproject.hip"

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

static void launch(const ReprojectArgs& a, unsigned grid_x, unsigned grid_z) {
  for (unsigned z = 0; z < grid_z; ++z)
    for (unsigned b = 0; b < grid_x; ++b)
      for (unsigned t = 0; t < (unsigned)kRpThreads; ++t) {
        threadIdx = dim3(t, 0, 0); blockIdx = dim3(b, 0, z); gridDim = dim3(grid_x, 1, grid_z);
        if (a.g.filter == reproject::kBicubic) k_reproject<reproject::kBicubic>(a); else k_reproject<reproject::kBilinear>(a);
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
  std::map<std::string, std::vector<uint32_t>> sources;
  char path[4096], num[10][64];
  int cols, rows, out_cols, out_rows, projection, face, filter, n_cases = 0;
  while (fscanf(list, "%4095s %d %d %d %d %d %d %d %63s %63s %63s %63s %63s %63s %63s %63s %63s %63s", path, &cols, &rows, &out_cols, &out_rows, &projection,
                &face, &filter, num[0], num[1], num[2], num[3], num[4], num[5], num[6], num[7], num[8], num[9]) == 18) {
    if (!sources.count(path)) sources[path] = read_file(path);
    const std::vector<uint32_t>& file = sources[path];
    if (cols <= 0 || rows <= 0 || out_cols <= 0 || out_rows <= 0 || file.size() != size_t(cols) * rows) { printf("%s is not %d x %d BGRA, or a bad size\n", path, cols, rows); return 2; }
    const size_t px = size_t(cols) * rows, out_px = size_t(out_cols) * out_rows;
    auto src = exact<uint32_t>(px);
    memcpy(src.get(), file.data(), px * 4);
    ReprojectArgs a;
    memset(&a, 0, sizeof a);
    a.g.projection = projection; a.g.filter = filter; a.g.cols = cols; a.g.rows = rows; a.g.out_cols = out_cols; a.g.out_rows = out_rows;
    a.g.t = projection == reproject::kRectilinear ? reproject::tan_half_fov(strtod(num[0], nullptr)) : 0.0;
    for (int k = 0; k < 9; ++k) a.g.rot[k] = strtod(num[1 + k], nullptr);
    auto eq = exact<double>(2 * (size_t(out_cols) + out_rows));
    if (projection == reproject::kEquirect) { reproject::make_equirect_tables(out_cols, out_rows, eq.get()); a.eq = eq.get(); }
    auto cubic = exact<int>(1024);
    if (filter == reproject::kBicubic) { reproject::make_cubic_table(cubic.get()); a.cubic = cubic.get(); }
    auto d0 = exact<uint32_t>(out_px), d1 = exact<uint32_t>(out_px);
    auto fx = exact<int>(out_px), fy = exact<int>(out_px);
    a.src[0] = a.src[1] = src.get(); a.dst[0] = d0.get(); a.dst[1] = d1.get(); a.face[0] = a.face[1] = face;
    a.fx_out = fx.get(); a.fy_out = fy.get();
    const unsigned tiles = rp_grid(out_cols, out_rows);
    launch(a, tiles > 1 ? (tiles + 1) / 2 : 1, 2);
    if (memcmp(d0.get(), d1.get(), out_px * 4)) { printf("FAIL case %d: the two images of the batch differ\n", n_cases); return 1; }
    if (projection == reproject::kCube) {   // the set of six, as pf_reproject_cube_dev launches it; no coordinate planes
      std::unique_ptr<uint32_t[]> faces[6];
      for (int k = 0; k < 6; ++k) { faces[k] = exact<uint32_t>(out_px); a.src[k] = src.get(); a.dst[k] = faces[k].get(); a.face[k] = k; }
      a.fx_out = a.fy_out = nullptr;
      launch(a, tiles, 6);
      if (memcmp(d0.get(), faces[face].get(), out_px * 4)) { printf("FAIL case %d: face %d of the set of six differs from the single launch\n", n_cases, face); return 1; }
    }
    if (fwrite(d0.get(), 4, out_px, out) != out_px || fwrite(fx.get(), 4, out_px, out) != out_px || fwrite(fy.get(), 4, out_px, out) != out_px) { printf("cannot write %s\n", argv[2]); return 2; }
    ++n_cases;
  }
  fclose(list);
  if (fclose(out) != 0) { printf("cannot write %s\n", argv[2]); return 2; }
  printf("%d cases ok\n", n_cases);
  return 0;
}
