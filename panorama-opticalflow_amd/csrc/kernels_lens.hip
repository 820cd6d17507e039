// Lens remap on the device: packed BGRA photos of a camera rig in HBM -> each camera's equirectangular canvas, the
// warp the stitcher's inputs have been through.  The inverse of kernels_reproject.hip: one kernel, k_lens_remap<filter>, one thread per
// canvas pixel: the pixel's ray from the canvas's tables, the rotation into the camera, the lens model's radius, the radial polynomial
// and the position in the photo in fp64 (lens_math.hpp: add, subtract, multiply, divide, sqrt and the reprojection's polynomial
// arctangent, nothing fused, no libm), quantised to 8 fractional bits; then 2 x 2 (bilinear) or 4 x 4 (Catmull-Rom) taps in integer
// arithmetic over alpha-premultiplied colour (reproject_sample.hpp), columns and rows both clamped to the photo, and one dword store.
// Most canvas pixels of a camera are outside its photo: they leave before any tap is loaded and store four zero bytes.
// The launch shape is k_reproject's: a wave owns a 16 x 4 tile of the canvas and a workgroup 32 x 8; blockIdx.z is the image of a batch
// and has its own camera (a.lens[z]) and photo; the tiles of an image are walked with a grid stride.  No LDS, no barrier.
// Plain C++ throughout: the host-run test (tests/cpp/lens_kernels_host.cpp) compiles this file as it is.
#include <algorithm>

#include "pf_common.hpp"
#include "reproject_sample.hpp"

namespace pf {
namespace {

constexpr int kLnThreads = 256;
constexpr int kLnWaveX = 16, kLnWaveY = 4;    // canvas pixels of a wave
constexpr int kLnTileX = 32, kLnTileY = 8;    // ... of a workgroup: 2 x 2 waves

template <int FILTER>
__global__ __launch_bounds__(kLnThreads) void k_lens_remap(LensArgs a) {
  const uint32_t* __restrict__ src = a.src[blockIdx.z];
  uint32_t* __restrict__ dst = a.dst[blockIdx.z];
  const lens::Lens& l = a.lens[blockIdx.z];
  const lens::Geometry& g = a.g;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int tx = (wave % 2) * kLnWaveX + lane % kLnWaveX, ty = (wave / 2) * kLnWaveY + lane / kLnWaveX;
  const long long tiles_x = (g.cols + kLnTileX - 1) / kLnTileX, tiles_y = (g.rows + kLnTileY - 1) / kLnTileY;
  for (long long tile = blockIdx.x; tile < tiles_x * tiles_y; tile += gridDim.x) {
    const int i = int(tile % tiles_x) * kLnTileX + tx, j = int(tile / tiles_x) * kLnTileY + ty;
    if (i >= g.cols || j >= g.rows) continue;
    double d[3];
    lens::ray(g, i, j, a.eq, d);
    int fx, fy;
    lens::photo_fixed(g, l, d, &fx, &fy);
    const size_t at = size_t(j) * g.cols + i;
    if (a.fx_out) { a.fx_out[at] = fx; a.fy_out[at] = fy; }
    if (!dst) continue;
    uint32_t px = 0;
    if (lens::inside(g, l, fx, fy))
      px = FILTER == reproject::kBicubic ? rp_bicubic<false>(src, g.photo_cols, g.photo_rows, fx, fy, a.cubic) : rp_bilinear<false>(src, g.photo_cols, g.photo_rows, fx, fy);
    dst[at] = px;
  }
}

// workgroups of a launch: every tile once up to this many, a grid stride beyond
constexpr long long kLnMaxGrid = 1 << 20;

unsigned ln_grid(int w, int h) {
  const long long tiles = (long long)((w + kLnTileX - 1) / kLnTileX) * ((h + kLnTileY - 1) / kLnTileY);
  return (unsigned)std::min(tiles, kLnMaxGrid);
}

}  // namespace

void launch_lens_remap(hipStream_t st, int n, const LensArgs& a) {
  const dim3 grid(ln_grid(a.g.cols, a.g.rows), 1, n);
  if (a.g.filter == reproject::kBicubic) hipLaunchKernelGGL(k_lens_remap<reproject::kBicubic>, grid, dim3(kLnThreads), 0, st, a);
  else hipLaunchKernelGGL(k_lens_remap<reproject::kBilinear>, grid, dim3(kLnThreads), 0, st, a);
}

}  // namespace pf
