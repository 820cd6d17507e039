// The integer sampling of the reprojection, shared by the kernels that take an interpolated sample at a position of
// 8 fractional bits (kernels_reproject.hip, kernels_lens.hip): 2 x 2 (bilinear) or 4 x 4 (Catmull-Rom) taps over alpha-premultiplied
// colour (premul.hpp), rows clamped.  The column rule is the template's argument: WRAP columns modulo the width (a sphere), or clamp
// them like the rows (a flat photo).  The taps are direct dword loads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "premul.hpp"

namespace pf {

__device__ __forceinline__ int rp_wrap(int x, int n) {   // a true modulo; the taps of a pixel reach at most two columns past either edge
  while (x < 0) x += n;
  while (x >= n) x -= n;
  return x;
}

template <bool WRAP>
__device__ __forceinline__ int rp_col(int x, int n) { return WRAP ? rp_wrap(x, n) : min(max(x, 0), n - 1); }

template <bool WRAP>
__device__ __forceinline__ uint32_t rp_bilinear(const uint32_t* __restrict__ src, int cols, int rows, int fx, int fy) {
  const int x0 = fx >> 8, y0 = fy >> 8;
  const uint32_t wx[2] = {256u - uint32_t(fx & 255), uint32_t(fx & 255)}, wy[2] = {256u - uint32_t(fy & 255), uint32_t(fy & 255)};
  uint32_t acc[4] = {32768u, 32768u, 32768u, 32768u};
  for (int j = 0; j < 2; ++j) {
    const uint32_t* row = src + size_t(min(max(y0 + j, 0), rows - 1)) * cols;
    for (int i = 0; i < 2; ++i) {
      const uint32_t p = rz_premultiply(row[rp_col<WRAP>(x0 + i, cols)]), w = wx[i] * wy[j];
      for (int c = 0; c < 4; ++c) acc[c] += w * ((p >> (8 * c)) & 0xffu);
    }
  }
  uint32_t out = 0;
  for (int c = 0; c < 4; ++c) out |= (acc[c] >> 16) << (8 * c);
  return rz_unpremultiply(out);
}

// tab: 256 phases x 4 taps, each phase summing to 2048.  |sum of wx wy| <= 1.5625 * 2^22, times 255 and plus 2^21 stays below 2^31
template <bool WRAP>
__device__ __forceinline__ uint32_t rp_bicubic(const uint32_t* __restrict__ src, int cols, int rows, int fx, int fy, const int* __restrict__ tab) {
  const int x0 = fx >> 8, y0 = fy >> 8;
  const int* wx = tab + 4 * (fx & 255);
  const int* wy = tab + 4 * (fy & 255);
  int cx[4];
  for (int i = 0; i < 4; ++i) cx[i] = rp_col<WRAP>(x0 - 1 + i, cols);
  int acc[4] = {0, 0, 0, 0};
  for (int j = 0; j < 4; ++j) {
    const uint32_t* row = src + size_t(min(max(y0 - 1 + j, 0), rows - 1)) * cols;
    int r[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
      const uint32_t p = rz_premultiply(row[cx[i]]);
      for (int c = 0; c < 4; ++c) r[c] += wx[i] * int((p >> (8 * c)) & 0xffu);
    }
    for (int c = 0; c < 4; ++c) acc[c] += wy[j] * r[c];
  }
  // min(255, max(0, (acc + 2^21) >> 22)), written as a clamp of the sum and then the shift.  Shift first and hipcc (ROCm 7) packs two
  // channels with gfx950's v_ashr_pk_u8_i32 and ors the register in as if its upper half were zero; the hardware keeps what the
  // register held there, so a negative tap weight that lived in it showed up as 255 in the other two channels (tests/test_gpu_lens.py).
  constexpr int kTop = (255 << 22) | ((1 << 22) - 1);
  uint32_t out = 0;
  for (int c = 0; c < 4; ++c) out |= (uint32_t(min(kTop, max(0, acc[c] + (1 << 21)))) >> 22) << (8 * c);
  return rz_unpremultiply(out);
}

}  // namespace pf
