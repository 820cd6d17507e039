// Reprojection on the device: a packed BGRA equirectangular sphere in HBM -> a cube face, a rectilinear view or a
// turned sphere.  One kernel, k_reproject<filter>, one thread per output pixel: the pixel's ray, the rotation, the source position
// in fp64 (reproject_math.hpp: add, subtract, multiply, divide, sqrt and a polynomial arctangent, nothing fused, no libm), quantised to
// 8 fractional bits; then 2 x 2 (bilinear) or 4 x 4 (Catmull-Rom) taps in integer arithmetic over alpha-premultiplied colour
// (reproject_sample.hpp over premul.hpp, the resize's own functions), columns wrapped modulo the width, rows clamped, and one dword store.
// A wave owns a 16 x 4 tile of the output and a workgroup 32 x 8, so that the footprints of a wave's taps share cache lines; the taps
// are direct dword loads.  blockIdx.z is the image of a batch (or the face of a cube set: each image has its own face index); the
// tiles of an image are walked with a grid stride.  No LDS, no barrier.
// Plain C++ throughout: the host-run test (tests/cpp/reproject_kernels_host.cpp) compiles this file as it is.
#include <algorithm>

#include "pf_common.hpp"
#include "reproject_sample.hpp"

namespace pf {
namespace {

constexpr int kRpThreads = 256;
constexpr int kRpWaveX = 16, kRpWaveY = 4;    // output pixels of a wave
constexpr int kRpTileX = 32, kRpTileY = 8;    // ... of a workgroup: 2 x 2 waves

template <int FILTER>
__global__ __launch_bounds__(kRpThreads) void k_reproject(ReprojectArgs a) {
  const uint32_t* __restrict__ src = a.src[blockIdx.z];
  uint32_t* __restrict__ dst = a.dst[blockIdx.z];
  const int face = a.face[blockIdx.z];
  const reproject::Geometry& g = a.g;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int tx = (wave % 2) * kRpWaveX + lane % kRpWaveX, ty = (wave / 2) * kRpWaveY + lane / kRpWaveX;
  const long long tiles_x = (g.out_cols + kRpTileX - 1) / kRpTileX, tiles_y = (g.out_rows + kRpTileY - 1) / kRpTileY;
  for (long long tile = blockIdx.x; tile < tiles_x * tiles_y; tile += gridDim.x) {
    const int u = int(tile % tiles_x) * kRpTileX + tx, v = int(tile / tiles_x) * kRpTileY + ty;
    if (u >= g.out_cols || v >= g.out_rows) continue;
    double d[3];
    reproject::ray(g, face, u, v, a.eq, d);
    int fx, fy;
    reproject::source_fixed(g, d, &fx, &fy);
    const size_t at = size_t(v) * g.out_cols + u;
    if (a.fx_out) { a.fx_out[at] = fx; a.fy_out[at] = fy; }
    if (!dst) continue;
    uint32_t px = 0;
    if (reproject::inside(g, fy)) px = FILTER == reproject::kBicubic ? rp_bicubic<true>(src, g.cols, g.rows, fx, fy, a.cubic) : rp_bilinear<true>(src, g.cols, g.rows, fx, fy);
    dst[at] = px;
  }
}

// workgroups of a launch: every tile once up to this many, a grid stride beyond
constexpr long long kRpMaxGrid = 1 << 20;

unsigned rp_grid(int w, int h) {
  const long long tiles = (long long)((w + kRpTileX - 1) / kRpTileX) * ((h + kRpTileY - 1) / kRpTileY);
  return (unsigned)std::min(tiles, kRpMaxGrid);
}

}  // namespace

void launch_reproject(hipStream_t st, int n, const ReprojectArgs& a) {
  const dim3 grid(rp_grid(a.g.out_cols, a.g.out_rows), 1, n);
  if (a.g.filter == reproject::kBicubic) hipLaunchKernelGGL(k_reproject<reproject::kBicubic>, grid, dim3(kRpThreads), 0, st, a);
  else hipLaunchKernelGGL(k_reproject<reproject::kBilinear>, grid, dim3(kRpThreads), 0, st, a);
}

}  // namespace pf
