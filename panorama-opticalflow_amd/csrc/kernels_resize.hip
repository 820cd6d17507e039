// Resize on the device: packed BGRA in HBM -> packed BGRA of another size, byte for byte what Pillow's Image.resize
// gives for an RGBA image: a separable antialiased resample in 22-bit fixed point over alpha-premultiplied colour.
//   k_resize_h   the horizontal pass, out_cols x rows: premultiply fused into its loads.  A workgroup takes 64 output columns of 4 rows
//                and stages the source columns its taps reach through LDS, kRzPiece of them at a time, so that no tap count outgrows
//                LDS (300 -> 1 has 300 taps); a thread keeps the four accumulators of its output pixel across the pieces
//   k_resize_v   the vertical pass, out_cols x out_rows: un-premultiply fused into its store.  A wave takes 64 adjacent columns of one
//                output row: every tap is one coalesced dword load per lane, and the row's bounds and coefficients are wave-uniform
// A one-axis resize runs one of them with both fusions in it (the flags).  The tables are the host's (pf_api_resize.inl): per output
// index its first source index and tap count, and the coefficients tap-major (k[t * out + index]), so that the horizontal pass reads
// them coalesced.  Integer arithmetic only.  blockIdx.z is the image of a batch; the tiles of an image are walked with a grid stride.
// Plain C++ throughout: the host-run test (tests/cpp/resize_kernels_host.cpp) compiles this file as it is.
#include <algorithm>

#include "pf_common.hpp"
#include "premul.hpp"   // rz_premultiply, rz_unpremultiply

namespace pf {
namespace {

constexpr int kRzThreads = 256;
constexpr int kRzTileX = 64, kRzTileY = 4;   // output pixels of a workgroup: a wave per row
constexpr int kRzPiece = 256;                // source columns of the horizontal pass staged at a time (4 rows x 256 dwords = 4 KB of LDS)
constexpr int kRzPrecBits = 22;

// Pillow accumulates in a 32-bit int; unsigned here, so that a table past the issue's bound wraps as the hardware does instead of being undefined
struct RzAcc {
  uint32_t c[4];
  __device__ __forceinline__ void init() { c[0] = c[1] = c[2] = c[3] = 1u << (kRzPrecBits - 1); }
  __device__ __forceinline__ void tap(uint32_t v, int k) {
    for (int i = 0; i < 4; ++i) c[i] += ((v >> (8 * i)) & 0xffu) * (uint32_t)k;
  }
  // min(255, max(0, (int)c >> 22)) per channel, written as a clamp of the sum and then the shift: shift first and hipcc packs two channels
  // with gfx950's v_ashr_pk_u8_i32, whose upper half the hardware does not clear (reproject_sample.hpp).  The bytes are the
  // same for every accumulator (tests/cpp/resize_pack_check.cpp); tests/test_pack_isa.py keeps the instruction out of every kernel.
  __device__ __forceinline__ uint32_t pack() const {
    constexpr int kTop = (255 << kRzPrecBits) | ((1 << kRzPrecBits) - 1);
    uint32_t out = 0;
    for (int i = 0; i < 4; ++i) out |= (uint32_t(min(kTop, max(0, (int)c[i]))) >> kRzPrecBits) << (8 * i);
    return out;
  }
};

__global__ __launch_bounds__(kRzThreads) void k_resize_h(ResizePtrs io, int cols, int rows, int out_cols, const int* __restrict__ bounds,
                                                          const int* __restrict__ k, int premul, int unpremul) {
  __shared__ uint32_t win[kRzTileY][kRzPiece];
  const uint32_t* __restrict__ src = io.src[blockIdx.z];
  uint32_t* __restrict__ dst = io.dst[blockIdx.z];
  const int tx = threadIdx.x % kRzTileX, ty = threadIdx.x / kRzTileX;
  const long long tiles_x = (out_cols + kRzTileX - 1) / kRzTileX, tiles_y = (rows + kRzTileY - 1) / kRzTileY;
  for (long long tile = blockIdx.x; tile < tiles_x * tiles_y; tile += gridDim.x) {
    const int x0 = int(tile % tiles_x) * kRzTileX, y0 = int(tile / tiles_x) * kRzTileY;
    const int xx = x0 + tx, y = y0 + ty, x_last = min(x0 + kRzTileX, out_cols) - 1;
    const bool live = xx < out_cols && y < rows;
    // the first source index and the end of the window never decrease along the axis: the tile's window is [first's start, last's end)
    const int lo = bounds[2 * x0], hi = bounds[2 * x_last] + bounds[2 * x_last + 1];
    const int xmin = live ? bounds[2 * xx] : 0, xend = live ? xmin + bounds[2 * xx + 1] : 0;
    RzAcc acc; acc.init();
    for (int p0 = lo; p0 < hi; p0 += kRzPiece) {
      const int pn = min(kRzPiece, hi - p0);
      for (int i = threadIdx.x; i < kRzTileY * kRzPiece; i += kRzThreads) {
        const int r = i / kRzPiece, col = i % kRzPiece;
        if (col < pn && y0 + r < rows) {
          const uint32_t v = src[size_t(y0 + r) * cols + p0 + col];
          win[r][col] = premul ? rz_premultiply(v) : v;
        }
      }
      __syncthreads();
      for (int x = max(xmin, p0); x < min(xend, p0 + pn); ++x) acc.tap(win[ty][x - p0], k[size_t(x - xmin) * out_cols + xx]);
      __syncthreads();
    }
    if (live) { const uint32_t v = acc.pack(); dst[size_t(y) * out_cols + xx] = unpremul ? rz_unpremultiply(v) : v; }
  }
}

__global__ __launch_bounds__(kRzThreads) void k_resize_v(ResizePtrs io, int cols, int rows, int out_rows, const int* __restrict__ bounds,
                                                          const int* __restrict__ k, int premul, int unpremul) {
  const uint32_t* __restrict__ src = io.src[blockIdx.z];
  uint32_t* __restrict__ dst = io.dst[blockIdx.z];
  const int tx = threadIdx.x % kRzTileX, ty = threadIdx.x / kRzTileX;
  const long long tiles_x = (cols + kRzTileX - 1) / kRzTileX, tiles_y = (out_rows + kRzTileY - 1) / kRzTileY;
  for (long long tile = blockIdx.x; tile < tiles_x * tiles_y; tile += gridDim.x) {
    const int x = int(tile % tiles_x) * kRzTileX + tx, yy = int(tile / tiles_x) * kRzTileY + ty;
    if (x >= cols || yy >= out_rows) continue;
    const int ymin = bounds[2 * yy], n = bounds[2 * yy + 1];
    RzAcc acc; acc.init();
    for (int t = 0; t < n; ++t) {
      const uint32_t v = src[size_t(ymin + t) * cols + x];
      acc.tap(premul ? rz_premultiply(v) : v, k[size_t(t) * out_rows + yy]);
    }
    const uint32_t v = acc.pack();
    dst[size_t(yy) * cols + x] = unpremul ? rz_unpremultiply(v) : v;
  }
}

// workgroups of a launch: every tile once up to this many, a grid stride beyond (a canvas of 9000 x 4000 has 141 000 tiles)
constexpr long long kRzMaxGrid = 1 << 20;

unsigned rz_grid(int w, int h) {
  const long long tiles = (long long)((w + kRzTileX - 1) / kRzTileX) * ((h + kRzTileY - 1) / kRzTileY);
  return (unsigned)std::min(tiles, kRzMaxGrid);
}

}  // namespace

void launch_resize_h(hipStream_t st, int n, const ResizePtrs& io, int cols, int rows, int out_cols, const int* bounds, const int* k, bool premul, bool unpremul) {
  hipLaunchKernelGGL(k_resize_h, dim3(rz_grid(out_cols, rows), 1, n), dim3(kRzThreads), 0, st, io, cols, rows, out_cols, bounds, k, (int)premul, (int)unpremul);
}

void launch_resize_v(hipStream_t st, int n, const ResizePtrs& io, int cols, int rows, int out_rows, const int* bounds, const int* k, bool premul, bool unpremul) {
  hipLaunchKernelGGL(k_resize_v, dim3(rz_grid(cols, out_rows), 1, n), dim3(kRzThreads), 0, st, io, cols, rows, out_rows, bounds, k, (int)premul, (int)unpremul);
}

}  // namespace pf
