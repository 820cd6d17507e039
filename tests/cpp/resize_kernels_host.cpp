// The resize kernels (csrc/kernels_resize.hip) run on the host, thread for thread, under the address and undefined-behaviour
// sanitizers: the images, the intermediate plane and both tables have exactly the sizes the library gives them, so an index past an
// image, a table or the LDS window is caught here, without a GPU.  The tables are the library's own (csrc/resize_table.hpp).
// Arguments, in groups of `IN.bgra cols rows out_cols out_rows filter OUT.bgra`: each raw image is resized as pf_resize_dev does it
// (an axis whose size stays runs no pass), for the byte comparison with the serial model (tests/resize_model.py).  Every launch has
// fewer workgroups than tiles, so the grid-stride walk runs; an image pair is launched as a batch of two (blockIdx.z).
// A group `pass IN.bgra cols rows axis n_out filter premul unpremul OUT.bgra` runs one pass alone, as pf_stage_resize_pass does: axis 0
// k_resize_h to n_out columns, axis 1 k_resize_v to n_out rows, with the two fusions as given.
// Built and run by tests/test_resize_kernels_host.py:  g++ -std=c++20 -fsanitize=address,undefined -Itests/cpp/hip_host_shim ... -pthread
#include <stdio.h>
#include <string.h>

#include "../../panorama-opticalflow_amd/csrc/kernels_resize.hip"
#include "../../panorama-opticalflow_amd/csrc/resize_table.hpp"

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

// the shim's launcher with the image index of a batch in blockIdx.z
template <class Kernel, class... Args>
static void launch_xz(Kernel kernel, unsigned grid_x, unsigned grid_z, unsigned block, Args... args) {
  for (unsigned z = 0; z < grid_z; ++z)
    for (unsigned b = 0; b < grid_x; ++b) {
      std::barrier<> bar(block);
      host_shim_barrier = &bar;
      std::vector<std::thread> threads;
      for (unsigned t = 0; t < block; ++t)
        threads.emplace_back([=]() { threadIdx = dim3(t, 0, 0); blockIdx = dim3(b, 0, z); gridDim = dim3(grid_x, 1, grid_z); kernel(args...); });
      for (auto& th : threads) th.join();
    }
}

static unsigned few(unsigned tiles) { return std::min(tiles, 3u); }

// two copies of the image as a batch of two; the results must agree and the first is returned
static std::vector<uint32_t> resize(const std::vector<uint32_t>& img, int cols, int rows, int out_cols, int out_rows, int filter) {
  const bool do_h = out_cols != cols, do_v = out_rows != rows;
  if (!do_h && !do_v) return img;
  const std::vector<uint32_t> img2(img);
  std::vector<uint32_t> out[2] = {std::vector<uint32_t>(size_t(out_cols) * out_rows), std::vector<uint32_t>(size_t(out_cols) * out_rows)};
  std::vector<uint32_t> mid[2];
  if (do_h && do_v) for (auto& m : mid) m.resize(size_t(out_cols) * rows);
  ResizePtrs h, v;
  memset(&h, 0, sizeof h); memset(&v, 0, sizeof v);
  for (int k = 0; k < 2; ++k) {
    h.src[k] = k ? img2.data() : img.data(); h.dst[k] = do_v ? mid[k].data() : out[k].data();
    v.src[k] = do_h ? mid[k].data() : h.src[k]; v.dst[k] = out[k].data();
  }
  resize_table::Table th, tv;
  if (do_h) {
    resize_table::make(cols, out_cols, filter, &th);
    const std::vector<int> bounds(th.bounds), k(th.k);   // (exact sizes: no vector capacity behind them)
    launch_xz(k_resize_h, few(rz_grid(out_cols, rows)), 2u, (unsigned)kRzThreads, h, cols, rows, out_cols, bounds.data(), k.data(), 1, (int)!do_v);
  }
  if (do_v) {
    resize_table::make(rows, out_rows, filter, &tv);
    const std::vector<int> bounds(tv.bounds), k(tv.k);
    launch_xz(k_resize_v, few(rz_grid(out_cols, out_rows)), 2u, (unsigned)kRzThreads, v, out_cols, rows, out_rows, bounds.data(), k.data(), (int)!do_h, 1);
  }
  if (out[0] != out[1]) { printf("FAIL: the two images of the batch differ\n"); return {}; }
  return out[0];
}

// one pass alone, a batch of one
static std::vector<uint32_t> one_pass(const std::vector<uint32_t>& img, int cols, int rows, int axis, int n_out, int filter, int premul, int unpremul) {
  std::vector<uint32_t> out(axis ? size_t(cols) * n_out : size_t(n_out) * rows);
  ResizePtrs io;
  memset(&io, 0, sizeof io);
  io.src[0] = img.data(); io.dst[0] = out.data();
  resize_table::Table t;
  resize_table::make(axis ? rows : cols, n_out, filter, &t);
  const std::vector<int> bounds(t.bounds), k(t.k);
  if (axis) launch_xz(k_resize_v, few(rz_grid(cols, n_out)), 1u, (unsigned)kRzThreads, io, cols, rows, n_out, bounds.data(), k.data(), premul, unpremul);
  else launch_xz(k_resize_h, few(rz_grid(n_out, rows)), 1u, (unsigned)kRzThreads, io, cols, rows, n_out, bounds.data(), k.data(), premul, unpremul);
  return out;
}

static bool write_file(const char* path, const std::vector<uint32_t>& out) {
  FILE* f = fopen(path, "wb");
  const bool ok = f && fwrite(out.data(), 4, out.size(), f) == out.size();
  if (f) fclose(f);
  if (!ok) printf("cannot write %s\n", path);
  return ok;
}

static int run_pass(char** a) {   // a[0] = "pass"
  const int cols = atoi(a[2]), rows = atoi(a[3]), axis = atoi(a[4]), n_out = atoi(a[5]), filter = atoi(a[6]), premul = atoi(a[7]), unpremul = atoi(a[8]);
  const std::vector<uint8_t> raw = read_file(a[1]);
  if (cols <= 0 || rows <= 0 || n_out <= 0 || (axis != 0 && axis != 1) || !resize_table::known(filter) || raw.size() != size_t(cols) * rows * 4) {
    printf("%s is not %d x %d BGRA, or a bad axis, size or filter\n", a[1], cols, rows);
    return 2;
  }
  std::vector<uint32_t> img(size_t(cols) * rows);
  memcpy(img.data(), raw.data(), raw.size());
  return write_file(a[9], one_pass(img, cols, rows, axis, n_out, filter, premul, unpremul)) ? 0 : 2;
}

int main(int argc, char** argv) {
  const char* usage = "usage: %s [IN.bgra cols rows out_cols out_rows filter OUT.bgra | pass IN.bgra cols rows axis n_out filter premul unpremul OUT.bgra]...\n";
  if (argc < 2) { printf(usage, argv[0]); return 2; }
  for (int i = 1; i < argc; i += 7) {
    if (!strcmp(argv[i], "pass")) {
      if (i + 10 > argc) { printf(usage, argv[0]); return 2; }
      if (int e = run_pass(argv + i)) return e;
      i += 3;
      continue;
    }
    if (i + 7 > argc) { printf(usage, argv[0]); return 2; }
    const int cols = atoi(argv[i + 1]), rows = atoi(argv[i + 2]), out_cols = atoi(argv[i + 3]), out_rows = atoi(argv[i + 4]), filter = atoi(argv[i + 5]);
    const std::vector<uint8_t> raw = read_file(argv[i]);
    if (cols <= 0 || rows <= 0 || out_cols <= 0 || out_rows <= 0 || !resize_table::known(filter) || raw.size() != size_t(cols) * rows * 4) {
      printf("%s is not %d x %d BGRA, or a bad size or filter\n", argv[i], cols, rows);
      return 2;
    }
    std::vector<uint32_t> img(size_t(cols) * rows);
    memcpy(img.data(), raw.data(), raw.size());
    const std::vector<uint32_t> out = resize(img, cols, rows, out_cols, out_rows, filter);
    if (out.empty()) return 1;
    if (!write_file(argv[i + 6], out)) return 2;
  }
  printf("ok\n");
  return 0;
}
