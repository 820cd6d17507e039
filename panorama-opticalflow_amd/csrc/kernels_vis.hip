// Flow visualisers (CPU/OpticalFlow.cpp:147-204, the panel of CPU/main.cpp:20-45) on the device: debug output of a flow
// that lives in HBM.  Byte-identical restatements of the reference's OpenCV 3.2 calls:
//   * grey disparity: normalize(NORM_MINMAX, CV_32F) + convertTo(CV_8U) -- min/max reduction, then ONE float scale / shift
//     (computed in double from the two extremes, as normalize does) and round-half-even + saturate per pixel;
//   * colour wheel: per-pixel magnitude / hue bytes (glibc's atan2f, csrc/libm_exact.hpp) + cvtColor(HSV2BGR) on 8-bit;
//   * vector field: line(..., CV_AA) = LineAA (drawing.cpp) per 12-px grid point, in GATHER form: each output pixel applies,
//     in the reference's row-major arrow order, the blend each arrow whose footprint can reach it writes there.
// Non-finite flow components are counted on the way (the entry points refuse such a flow: the reference's result there rests
// on OpenCV's SIMD min/max and on undefined float -> uchar conversions).
#include "pf_common.hpp"
#include "libm_exact.hpp"

namespace pf {

namespace {

constexpr int kVisBlocks = 1024;   // partial min/max slots of the grey reduction (grid-stride)
constexpr int kGrid = 12;          // kGridSpacing, CPU/OpticalFlow.cpp:161

// [OpenCV 3.2 drawing.cpp] LineAA's tables
__constant__ int kSlopeCorr[32] = {181, 181, 181, 182, 182, 183, 184, 185, 187, 188, 190, 192, 194, 196, 198, 201,
                                   203, 206, 209, 211, 214, 218, 221, 224, 227, 231, 235, 238, 242, 246, 250, 254};
__constant__ int kFilter[64] = {168, 177, 185, 194, 202, 210, 218, 224, 231, 236, 241, 246, 249, 252, 254, 254,
                                254, 254, 252, 249, 246, 241, 236, 231, 224, 218, 210, 202, 194, 185, 177, 168,
                                158, 149, 140, 131, 122, 114, 105, 97,  89,  82,  75,  68,  62,  56,  50,  45,
                                40,  36,  32,  28,  25,  22,  19,  16,  14,  12,  11,  9,   8,   7,   5,   5};

__device__ __forceinline__ bool finite2(float2 f) { return isfinite(f.x) && isfinite(f.y); }

// saturate_cast<uchar>(float): cvRound (round half to even) + clamp
__device__ __forceinline__ unsigned sat_u8(float v) {
  const int i = (int)__builtin_rintf(v);
  return (unsigned)(i < 0 ? 0 : i > 255 ? 255 : i);
}

__device__ __forceinline__ unsigned grey_byte(float fx, const VisParams& p) { return sat_u8(fx * p.scale + p.shift); }

// visualizeFlowColorWheel's pixel (CPU/OpticalFlow.cpp:189-200) + cvtColor(HSV2BGR) for 8-bit, hrange 180
// ([OpenCV 3.2 color.cpp] HSV2RGB_b -> HSV2RGB_f).  Returns B | G << 8 | R << 16.
__device__ __forceinline__ unsigned wheel_bgr(float2 f, float max_disp) {
  const float mag = sqrtf(f.x * f.x + f.y * f.y);
  const float vx = f.x / mag, vy = f.y / mag;   // 0 / 0 = NaN for a zero vector, as in the reference
  const float r = mag / max_disp;
  const float brightness = .25f + .75f * (r < 1.0f ? r : 1.0f);   // std::min(1.0f, r)
  const float hue = (float)(((double)pf_libm::atan2f_exact(vy, vx) + 3.14159265358979323846) / (2.0 * 3.14159265358979323846));
  const float th = 180.0f * hue, tv = 255.0f * brightness;
  // (uchar)float truncates; a NaN hue (zero vector) is undefined behaviour in C++ -- defined here as x86-64's cvttss2si
  // result INT_MIN, whose low byte is 0
  const int H = th != th ? 0 : ((int)th & 255), S = (int)tv & 255;
  float h = (float)H, s = (float)S * (1.f / 255.f), v = (float)S * (1.f / 255.f);
  float b, g, rr;
  if (s == 0) b = g = rr = v;
  else {
    h *= 6.f / 180.f;
    if (h < 0) do h += 6; while (h < 0);
    else if (h >= 6) do h -= 6; while (h >= 6);
    int sector = (int)floorf(h);
    h -= (float)sector;
    if ((unsigned)sector >= 6u) { sector = 0; h = 0.f; }
    const float t0 = v, t1 = v * (1.f - s), t2 = v * (1.f - s * h), t3 = v * (1.f - s * (1.f - h));
    // sector_data {1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0} -> (b, g, r)
    switch (sector) {
      case 0: b = t1; g = t3; rr = t0; break;
      case 1: b = t1; g = t0; rr = t2; break;
      case 2: b = t3; g = t0; rr = t1; break;
      case 3: b = t0; g = t2; rr = t1; break;
      case 4: b = t0; g = t1; rr = t3; break;
      default: b = t2; g = t1; rr = t0; break;
    }
  }
  return sat_u8(b * 255.f) | sat_u8(g * 255.f) << 8 | sat_u8(rr * 255.f) << 16;
}

// ---- LineAA, restated per arrow ----
// An arrow starts at a grid point (12 <= x < cols-12, 12 <= y < rows-12) and ends at most 7 px away, so both end points lie
// inside LineAA's clip rectangle (2 px in from every border): clipLine never changes them and is not restated.  With integer
// end points LineAA walks the major axis from the smaller end to one past the larger; step s writes the three pixels
// (major0 + s, c - 1 .. c + 1) with c = (minor0 + s * step) >> 16 -- every pixel at most once per line.
struct Arrow {
  int major0;   // first major coordinate; bit 31 of `flags` = x is the major axis
  int minor0;   // 16.16 minor coordinate at step 0 (incl. LineAA's + 0.5)
  int step;     // 16.16 minor increment per step
  int flags;    // ecount (bits 0-7) | slope (bits 8-16) | i (bits 17-23) | j (bits 24-30) | xmajor (bit 31)
};

__device__ __forceinline__ Arrow make_arrow(int x0, int y0, int x1, int y1) {
  constexpr int S = 16, ONE = 1 << S;
  long long p1x = (long long)x0 << S, p1y = (long long)y0 << S, p2x = (long long)x1 << S, p2y = (long long)y1 << S;
  long long dx = p2x - p1x, dy = p2y - p1y;
  const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
  Arrow a;
  long long ecount, i, j, st;
  int slope;
  if (ax > ay) {
    if (dx < 0) { dy = -dy; long long t = p1x; p1x = p2x; p2x = t; t = p1y; p1y = p2y; p2y = t; }
    st = (dy * ONE) / (ax | 1);
    p2x += ONE;
    ecount = (p2x >> S) - (p1x >> S);
    const long long jj = -(p1x & (ONE - 1));
    p1y += ((st * jj) >> S) + (ONE >> 1);
    slope = (int)((st >> (S - 5)) & 0x3f);
    slope ^= (st < 0 ? 0x3f : 0);
    i = (p1x >> (S - 7)) & 0x78;
    j = (p2x >> (S - 7)) & 0x78;
    a.major0 = (int)(p1x >> S); a.minor0 = (int)p1y;
  } else {
    if (dy < 0) { dx = -dx; long long t = p1x; p1x = p2x; p2x = t; t = p1y; p1y = p2y; p2y = t; }
    st = (dx * ONE) / (ay | 1);
    p2y += ONE;
    ecount = (p2y >> S) - (p1y >> S);
    const long long jj = -(p1y & (ONE - 1));
    p1x += ((st * jj) >> S) + (ONE >> 1);
    slope = (int)((st >> (S - 5)) & 0x3f);
    slope ^= (st < 0 ? 0x3f : 0);
    i = (p1y >> (S - 7)) & 0x78;
    j = (p2y >> (S - 7)) & 0x78;
    a.major0 = (int)(p1y >> S); a.minor0 = (int)p1x;
  }
  slope = (slope & 0x20) ? 0x100 : kSlopeCorr[slope];
  a.step = (int)st;
  a.flags = (int)ecount | slope << 8 | (int)i << 17 | (int)j << 24 | (ax > ay ? (int)0x80000000 : 0);
  return a;
}

// LineAA's end-point correction table entry k (drawing.cpp: ep_table[0..8])
__device__ __forceinline__ int ep_entry(int k, int slope, int i, int j) {
  const int t0 = slope << 7, t1 = ((0x78 - i) | 4) * slope, t2 = (j | 4) * slope;
  switch (k) {
    case 0: return 0;
    case 1: case 3: return ((((j - i) & 0x78) | 4) * slope >> 8) & 0x1ff;
    case 2: return (t1 >> 8) & 0x1ff;
    case 4: return ((((j - i) + 0x80) | 4) * slope >> 8) & 0x1ff;
    case 5: return ((t1 + t0) >> 8) & 0x1ff;
    case 6: return (t2 >> 8) & 0x1ff;
    case 7: return ((t2 + t0) >> 8) & 0x1ff;
    default: return slope;
  }
}

// The blend arrow `a` applies to pixel (px, py), if it touches it: ICV_PUT_POINT for 4 channels, colour (0, 0, 0, 255)
__device__ __forceinline__ uchar4 arrow_apply(const Arrow& a, int px, int py, uchar4 p) {
  const bool xmajor = a.flags < 0;
  const int ecount0 = a.flags & 0xff, slope = (a.flags >> 8) & 0x1ff, i = (a.flags >> 17) & 0x7f, j = (a.flags >> 24) & 0x7f;
  const int s = (xmajor ? px : py) - a.major0;
  if (s < 0 || s > ecount0) return p;
  const int m = a.minor0 + s * a.step;
  const int d = (xmajor ? py : px) - (m >> 16);
  if (d < -1 || d > 1) return p;
  const int dist = (m >> 11) & 31, ec = ecount0 - s;
  const int sidx = ((s >= 2) + 1) & (s | 2), eidx = ((ec >= 2) + 1) & (ec | 2);
  const int ep = ep_entry(sidx * 3 + eidx, slope, i, j);
  const int ft = kFilter[d < 0 ? dist + 32 : d == 0 ? dist : 63 - dist];
  const int al = (ep * ft >> 8) & 0xff;
  int cb = p.x, cg = p.y, cr = p.z, ca = p.w;
  cb += ((0 - cb) * al + 127) >> 8;
  cg += ((0 - cg) * al + 127) >> 8;
  cr += ((0 - cr) * al + 127) >> 8;
  ca += ((255 - ca) * al + 127) >> 8;
  return make_uchar4((unsigned char)cb, (unsigned char)cg, (unsigned char)cr, (unsigned char)ca);
}

// Every arrow that can reach (px, py) -- its grid point within 10 px on both axes (an arrow's footprint stays within 9), at
// most 2 x 2 of them -- in the reference's loop order (y outer, x inner).
__device__ __forceinline__ uchar4 field_pixel(const Arrow* __restrict__ arrows, int nax, int nay, int px, int py, uchar4 p) {
  if (nax <= 0 || nay <= 0) return p;
  int gy0 = (py - 10 + kGrid - 1) / kGrid, gy1 = (py + 10) / kGrid, gx0 = (px - 10 + kGrid - 1) / kGrid, gx1 = (px + 10) / kGrid;
  gy0 = gy0 < 1 ? 1 : gy0; gx0 = gx0 < 1 ? 1 : gx0;
  gy1 = gy1 > nay ? nay : gy1; gx1 = gx1 > nax ? nax : gx1;
  for (int gy = gy0; gy <= gy1; ++gy)
    for (int gx = gx0; gx <= gx1; ++gx) p = arrow_apply(arrows[size_t(gy - 1) * nax + (gx - 1)], px, py, p);
  return p;
}

// ---- kernels ----

// pass 1 of the grey disparity: partial min / max of flow.x per block, count of non-finite components
__global__ __launch_bounds__(256) void k_vis_minmax(const float2* __restrict__ flow, size_t n, float* __restrict__ part, VisParams* __restrict__ par) {
  float mn = INFINITY, mx = -INFINITY;
  int bad = 0;
  const size_t stride = size_t(gridDim.x) * blockDim.x;
  size_t k = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
  for (; k + 3 * stride < n; k += 4 * stride) {   // four independent loads in flight per thread
    const float2 a = flow[k], b = flow[k + stride], c = flow[k + 2 * stride], d = flow[k + 3 * stride];
    mn = fminf(mn, fminf(fminf(a.x, b.x), fminf(c.x, d.x)));
    mx = fmaxf(mx, fmaxf(fmaxf(a.x, b.x), fmaxf(c.x, d.x)));
    bad += !finite2(a) + !finite2(b) + !finite2(c) + !finite2(d);
  }
  for (; k < n; k += stride) {
    const float2 a = flow[k];
    mn = fminf(mn, a.x); mx = fmaxf(mx, a.x); bad += !finite2(a);
  }
  for (int o = 32; o > 0; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); bad += __shfl_xor(bad, o);
  }
  __shared__ float smn[4], smx[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { smn[w] = mn; smx[w] = mx; if (bad) atomicAdd(&par->nonfinite, bad); }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x] = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
    part[kVisBlocks + blockIdx.x] = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  }
}

// tail of the reduction: normalize()'s scale and shift in double ([OpenCV 3.2 convert.cpp] normalize, NORM_MINMAX, a = 0, b = 255),
// handed to convertTo as floats
__global__ __launch_bounds__(64) void k_vis_params(const float* __restrict__ part, int nb, VisParams* __restrict__ par) {
  float mn = INFINITY, mx = -INFINITY;
  for (int k = threadIdx.x; k < nb; k += 64) { mn = fminf(mn, part[k]); mx = fmaxf(mx, part[kVisBlocks + k]); }
  for (int o = 32; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
  if (threadIdx.x == 0) {
    const double smin = mn, smax = mx, dmin = 0.0, dmax = 255.0;
    const double scale = (dmax - dmin) * (smax - smin > 2.2204460492503131e-16 ? 1. / (smax - smin) : 0);
    const double shift = dmin - smin * scale;
    par->scale = (float)scale;
    par->shift = (float)shift;
  }
}

// one thread per arrow: LineAA's set-up for the arrow of grid point (12 (ax + 1), 12 (ay + 1)) (CPU/OpticalFlow.cpp:166-178)
__global__ __launch_bounds__(256) void k_vis_arrows(const float2* __restrict__ flow, int cols, int nax, int nay, Arrow* __restrict__ arrows) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nax * nay) return;
  const int x = kGrid * (k % nax + 1), y = kGrid * (k / nax + 1);
  float2 f = flow[size_t(y) * cols + x];
  const float mag = sqrtf(f.x * f.x + f.y * f.y);
  const float den = mag + 0.1f;
  f.x = f.x / den; f.y = f.y / den;
  // Point(x + fxy.x * kArrowLen, y + fxy.y * kArrowLen): float sums, truncated by Point's int constructor
  const int x1 = (int)((float)x + f.x * 7.0f), y1 = (int)((float)y + f.y * 7.0f);
  arrows[k] = make_arrow(x, y, x1, y1);
}

// grey disparity alone, CV_8UC1 packed: 4 pixels per thread, one dword store
__global__ __launch_bounds__(256) void k_vis_grey(const float2* __restrict__ flow, size_t n, const VisParams* __restrict__ par, uint8_t* __restrict__ out) {
  const size_t q = size_t(blockIdx.x) * blockDim.x + threadIdx.x, k = q * 4;
  if (k >= n) return;
  const VisParams p = *par;
  if (k + 4 <= n) {
    const float4 a = reinterpret_cast<const float4*>(flow)[q * 2], b = reinterpret_cast<const float4*>(flow)[q * 2 + 1];
    reinterpret_cast<unsigned*>(out)[q] = grey_byte(a.x, p) | grey_byte(a.z, p) << 8 | grey_byte(b.x, p) << 16 | grey_byte(b.z, p) << 24;
  } else {
    for (size_t e = k; e < n; ++e) out[e] = (uint8_t)grey_byte(flow[e].x, p);
  }
}

// colour wheel alone, CV_8UC3 packed: 4 pixels (12 bytes) per thread, three dword stores
__global__ __launch_bounds__(256) void k_vis_wheel(const float2* __restrict__ flow, size_t n, float max_disp, VisParams* __restrict__ par, uint8_t* __restrict__ out) {
  const size_t q = size_t(blockIdx.x) * blockDim.x + threadIdx.x, k = q * 4;
  if (k >= n) return;
  if (k + 4 <= n) {
    const float4 a = reinterpret_cast<const float4*>(flow)[q * 2], b = reinterpret_cast<const float4*>(flow)[q * 2 + 1];
    const float2 f0 = make_float2(a.x, a.y), f1 = make_float2(a.z, a.w), f2 = make_float2(b.x, b.y), f3 = make_float2(b.z, b.w);
    if (!finite2(f0) || !finite2(f1) || !finite2(f2) || !finite2(f3)) atomicAdd(&par->nonfinite, 1);
    const unsigned c0 = wheel_bgr(f0, max_disp), c1 = wheel_bgr(f1, max_disp), c2 = wheel_bgr(f2, max_disp), c3 = wheel_bgr(f3, max_disp);
    unsigned* o = reinterpret_cast<unsigned*>(out) + q * 3;
    o[0] = c0 | c1 << 24;
    o[1] = c1 >> 8 | c2 << 16;
    o[2] = c2 >> 16 | c3 << 8;
  } else {
    for (size_t e = k; e < n; ++e) {
      if (!finite2(flow[e])) atomicAdd(&par->nonfinite, 1);
      const unsigned c = wheel_bgr(flow[e], max_disp);
      out[e * 3] = (uint8_t)c; out[e * 3 + 1] = (uint8_t)(c >> 8); out[e * 3 + 2] = (uint8_t)(c >> 16);
    }
  }
}

// vector field alone, CV_8UC4 packed
__global__ __launch_bounds__(256) void k_vis_field(const uchar4* __restrict__ img, int cols, int rows, const Arrow* __restrict__ arrows, int nax, int nay,
                                                   uchar4* __restrict__ out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= cols) return;
  const size_t k = size_t(y) * cols + x;
  out[k] = field_pixel(arrows, nax, nay, x, y, img[k]);
}

// the panel of buildvisualizations (CPU/main.cpp:29-37): [GRAY2BGRA(grey) | BGR2BGRA(wheel) | vector field], 3 cols x rows BGRA.
// One thread per flow pixel: the flow and the image are read once, the three output pixels are dword stores.
__global__ __launch_bounds__(256) void k_vis_panel(const float2* __restrict__ flow, const uchar4* __restrict__ img, int cols, int rows, float max_disp,
                                                   const VisParams* __restrict__ par, const Arrow* __restrict__ arrows, int nax, int nay,
                                                   uchar4* __restrict__ out) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= cols) return;
  const size_t k = size_t(y) * cols + x;
  const float2 f = flow[k];
  const unsigned g = grey_byte(f.x, *par), c = wheel_bgr(f, max_disp);
  uchar4* o = out + size_t(y) * 3 * cols;
  o[x] = make_uchar4(g, g, g, 255);
  o[cols + x] = make_uchar4(c & 255, (c >> 8) & 255, (c >> 16) & 255, 255);
  o[2 * cols + x] = field_pixel(arrows, nax, nay, x, y, img[k]);
}

}  // namespace

// arrows per axis: grid points 12, 24, ... below size - 12
void vis_grid(int cols, int rows, int* nax, int* nay) {
  *nax = cols > 2 * kGrid ? (cols - kGrid - 1) / kGrid : 0;
  *nay = rows > 2 * kGrid ? (rows - kGrid - 1) / kGrid : 0;
}
size_t vis_part_bytes() { return size_t(2) * kVisBlocks * sizeof(float); }

void launch_vis_reduce(hipStream_t st, const float* flow, int cols, int rows, float* part, VisParams* par) {
  const size_t n = size_t(cols) * rows;
  size_t nb = (n + 1023) / 1024;
  if (nb > kVisBlocks) nb = kVisBlocks;
  hipLaunchKernelGGL(k_vis_minmax, dim3((unsigned)nb), dim3(256), 0, st, reinterpret_cast<const float2*>(flow), n, part, par);
  hipLaunchKernelGGL(k_vis_params, dim3(1), dim3(64), 0, st, part, (int)nb, par);
}

void launch_vis_arrows(hipStream_t st, const float* flow, int cols, int rows, void* arrows) {
  int nax, nay;
  vis_grid(cols, rows, &nax, &nay);
  if (nax * nay == 0) return;
  hipLaunchKernelGGL(k_vis_arrows, dim3((nax * nay + 255) / 256), dim3(256), 0, st, reinterpret_cast<const float2*>(flow), cols, nax, nay,
                     static_cast<Arrow*>(arrows));
}
size_t vis_arrow_bytes(int cols, int rows) {
  int nax, nay;
  vis_grid(cols, rows, &nax, &nay);
  return size_t(nax) * nay * sizeof(Arrow) + sizeof(Arrow);
}

static float max_disp(int cols, int rows) { return float(cols > rows ? cols : rows) / 20.0f; }   // maxExpectedDisplacement, :187-188

void launch_vis_grey(hipStream_t st, const float* flow, int cols, int rows, const VisParams* par, uint8_t* out) {
  const size_t n = size_t(cols) * rows, nq = (n + 3) / 4;
  hipLaunchKernelGGL(k_vis_grey, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float2*>(flow), n, par, out);
}

void launch_vis_wheel(hipStream_t st, const float* flow, int cols, int rows, VisParams* par, uint8_t* out) {
  const size_t n = size_t(cols) * rows, nq = (n + 3) / 4;
  hipLaunchKernelGGL(k_vis_wheel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float2*>(flow), n, max_disp(cols, rows), par, out);
}

void launch_vis_field(hipStream_t st, const uint8_t* img, int cols, int rows, const void* arrows, uint8_t* out) {
  int nax, nay;
  vis_grid(cols, rows, &nax, &nay);
  hipLaunchKernelGGL(k_vis_field, dim3((cols + 255) / 256, rows), dim3(256), 0, st, reinterpret_cast<const uchar4*>(img), cols, rows,
                     static_cast<const Arrow*>(arrows), nax, nay, reinterpret_cast<uchar4*>(out));
}

void launch_vis_panel(hipStream_t st, const float* flow, const uint8_t* img, int cols, int rows, const VisParams* par, const void* arrows, uint8_t* out) {
  int nax, nay;
  vis_grid(cols, rows, &nax, &nay);
  hipLaunchKernelGGL(k_vis_panel, dim3((cols + 255) / 256, rows), dim3(256), 0, st, reinterpret_cast<const float2*>(flow),
                     reinterpret_cast<const uchar4*>(img), cols, rows, max_disp(cols, rows), par, static_cast<const Arrow*>(arrows), nax, nay,
                     reinterpret_cast<uchar4*>(out));
}

}  // namespace pf
