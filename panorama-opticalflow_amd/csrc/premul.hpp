// Alpha premultiplication as Pillow does it, shared by the kernels that filter colour next to alpha (kernels_resize.hip,
// kernels_reproject.hip): a packed pixel with alpha in its top byte, the three colour bytes treated alike.  Integer arithmetic only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pf {

// colour * alpha / 255, rounded, as Pillow's MULDIV255; alpha stays
__device__ __forceinline__ uint32_t rz_premultiply(uint32_t v) {
  const uint32_t a = v >> 24;
  uint32_t out = v & 0xff000000u;
  for (int s = 0; s < 24; s += 8) {
    const uint32_t t = ((v >> s) & 0xffu) * a + 128u;
    out |= (((t >> 8) + t) >> 8) << s;
  }
  return out;
}

// the inverse as Pillow's rgbA2rgba: a true integer division (c <= 255 and 1 <= a <= 254 here, so 255 * c fits easily)
__device__ __forceinline__ uint32_t rz_unpremultiply(uint32_t v) {
  const uint32_t a = v >> 24;
  if (a == 0u || a == 255u) return v;
  uint32_t out = v & 0xff000000u;
  for (int s = 0; s < 24; s += 8) out |= min(255u, (255u * ((v >> s) & 0xffu)) / a) << s;
  return out;
}

}  // namespace pf
