// The geometry of the reprojection, one copy for the kernel (kernels_reproject.hip), the host API (pf_api_reproject.inl)
// and the host-run test: an output pixel's ray, its rotation, the source position and its quantisation to 8 fractional bits.  fp64
// add, subtract, multiply, divide and sqrt only, every product and sum rounded on its own (-ffp-contract=off), in exactly the order
// written here; tests/reproject_model.py restates it.  The arctangent is a range reduction and a fixed odd polynomial, no libm.
// The host-only part below makes the tables a launch reads (Catmull-Rom phases, the equirect output's sines and cosines) and the
// rotation of pf_reproject_rotation; those go through the host's sin / cos.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace pf {
namespace reproject {

#define PF_RP_FN __host__ __device__ __forceinline__

// the numbering of include/panoflow.h (PF_PROJ_*, PF_FACE_*, PF_REPROJECT_*)
constexpr int kCube = 0, kRectilinear = 1, kEquirect = 2;
constexpr int kFront = 0, kRight = 1, kBack = 2, kLeft = 3, kUp = 4, kDown = 5;
constexpr int kBilinear = 2, kBicubic = 3;

constexpr double kPi = 0x1.921fb54442d18p+1, kTwoPi = 0x1.921fb54442d18p+2, kHalfPi = 0x1.921fb54442d18p+0, kPi6 = 0x1.0c152382d7365p-1;
constexpr double kSqrt3 = 0x1.bb67ae8584caap+0, kTanPi12 = 0x1.126145e9ecd56p-2;
// atan t = t * sum_k c[k] * t^(2k), c[k] = (-1)^k / (2k + 1) rounded to double: thirteen Taylor terms.  |t| <= tan(pi/12) after the
// reduction, so the first term left out is below 0.268^27 / 27 = 1.4e-17; with the roundings of the Horner sum, the reduction and
// the quadrant the angle is good to a few 1e-16 rad (measured against libm in tests/test_reproject_model.py: below 1e-15)
constexpr int kAtanTerms = 13;
#define PF_RP_ATAN_COEF \
    0x1.0000000000000p+0,  -0x1.5555555555555p-2, 0x1.999999999999ap-3,  -0x1.2492492492492p-3, 0x1.c71c71c71c71cp-4,  \
    -0x1.745d1745d1746p-4, 0x1.3b13b13b13b14p-4,  -0x1.1111111111111p-4, 0x1.e1e1e1e1e1e1ep-5,  -0x1.af286bca1af28p-5, \
    0x1.8618618618618p-5,  -0x1.642c8590b2164p-5, 0x1.47ae147ae147bp-5

// what a launch knows of its images: the kernel's argument, the model's parameters
struct Geometry {
  int projection, filter;
  int cols, rows;           // the source sphere
  int out_cols, out_rows;
  double t;                 // rectilinear: tan(hfov / 2)
  double rot[9];            // row-major
};

// atan of 0 <= t <= 1.  Above tan(pi/12): atan t = pi/6 + atan((t sqrt3 - 1) / (sqrt3 + t)); below, the same division runs with
// t / 1 (exact) so that every lane executes one instruction stream.  Horner from the highest coefficient down.
PF_RP_FN double atan_unit(double t) {
  const bool big = t > kTanPi12;
  const double num = big ? t * kSqrt3 - 1.0 : t, den = big ? kSqrt3 + t : 1.0;
  const double r = num / den, z = r * r;
  const double c[kAtanTerms] = {PF_RP_ATAN_COEF};   // (a local: device code cannot index a host constant)
  double p = c[kAtanTerms - 1];
#pragma unroll
  for (int k = kAtanTerms - 2; k >= 0; --k) p = p * z + c[k];
  return (big ? kPi6 : 0.0) + r * p;
}

// atan2(y, x) in [-pi, pi]; 0 where both are zero (of either sign)
PF_RP_FN double atan2_poly(double y, double x) {
  const double ax = x < 0.0 ? -x : x, ay = y < 0.0 ? -y : y;
  const bool swap = ay > ax;
  const double mn = swap ? ax : ay, mx = swap ? ay : ax;
  double r = atan_unit(mn / (mx == 0.0 ? 1.0 : mx));
  if (swap) r = kHalfPi - r;
  if (x < 0.0) r = kPi - r;
  return y < 0.0 ? -r : r;
}

// the ray of output pixel (u, v).  eq: the equirect output's tables, cos lon[out_cols], sin lon[out_cols], cos lat[out_rows], sin lat[out_rows]
PF_RP_FN void ray(const Geometry& g, int face, int u, int v, const double* eq, double d[3]) {
  if (g.projection == kEquirect) {
    const double cl = eq[u], sl = eq[g.out_cols + u], cb = eq[2 * g.out_cols + v], sb = eq[2 * g.out_cols + g.out_rows + v];
    d[0] = cb * cl; d[1] = cb * sl; d[2] = sb;
    return;
  }
  const double a = (2.0 * (u + 0.5)) / g.out_cols - 1.0, b = 1.0 - (2.0 * (v + 0.5)) / g.out_rows;
  if (g.projection == kRectilinear) { d[0] = 1.0; d[1] = a * g.t; d[2] = ((b * g.t) * g.out_rows) / g.out_cols; return; }
  switch (face) {
    case kFront: d[0] = 1.0;  d[1] = a;    d[2] = b;    break;
    case kRight: d[0] = -a;   d[1] = 1.0;  d[2] = b;    break;
    case kBack:  d[0] = -1.0; d[1] = -a;   d[2] = b;    break;
    case kLeft:  d[0] = a;    d[1] = -1.0; d[2] = b;    break;
    case kUp:    d[0] = -b;   d[1] = a;    d[2] = 1.0;  break;
    default:     d[0] = b;    d[1] = a;    d[2] = -1.0; break;
  }
}

// floor of a double inside the int range, without a library call
PF_RP_FN int floor_int(double v) { const int i = (int)v; return i - (v < (double)i); }

// s = R d; lon, lat; the position in source pixels; 256 * position + 1/2, floored.  A rotation whose entries overflow the
// arithmetic gives no position: the pixel is outside (fy = INT32_MIN).
PF_RP_FN void source_fixed(const Geometry& g, const double d[3], int* fx, int* fy) {
  const double* R = g.rot;
  const double sx = (R[0] * d[0] + R[1] * d[1]) + R[2] * d[2];
  const double sy = (R[3] * d[0] + R[4] * d[1]) + R[5] * d[2];
  const double sz = (R[6] * d[0] + R[7] * d[1]) + R[8] * d[2];
  const double lon = atan2_poly(sy, sx);
  const double lat = atan2_poly(sz, sqrt(sx * sx + sy * sy));
  const double px = (lon / kTwoPi + 0.5) * g.cols - 0.5;
  const double py = (g.rows * 0.5 - 0.5) - (lat * g.cols) / kTwoPi;
  const double qx = 256.0 * px + 0.5, qy = 256.0 * py + 0.5;
  const bool number = qx >= -1.0e9 && qx <= 1.0e9 && qy >= -1.0e9 && qy <= 1.0e9;   // false for a NaN
  *fx = number ? floor_int(qx) : 0;
  *fy = number ? floor_int(qy) : INT32_MIN;
}

PF_RP_FN bool inside(const Geometry& g, int fy) { return fy >= -128 && fy <= 256 * (g.rows - 1) + 128; }

#undef PF_RP_FN
#undef PF_RP_ATAN_COEF

// ---- host only ----

// Catmull-Rom (a = -0.5) at phase f / 256: the taps at x0 - 1 .. x0 + 2 in 11-bit fixed point, floor(w * 2048 + 1/2) (every w is a
// multiple of 2^-25: the products are exact), the largest tap of a phase (the first of equals) adjusted so that the phase sums to 2048
inline double cubic_weight(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
  return 0.0;
}
inline void make_cubic_table(int* tab /* 256 * 4 */) {
  for (int f = 0; f < 256; ++f) {
    const double t = f / 256.0;
    int sum = 0, big = 0;
    for (int i = 0; i < 4; ++i) {
      tab[4 * f + i] = (int)floor(cubic_weight(t - (i - 1)) * 2048.0 + 0.5);
      sum += tab[4 * f + i];
      if (tab[4 * f + i] > tab[4 * f + big]) big = i;
    }
    tab[4 * f + big] += 2048 - sum;
  }
}

// the equirect output's tables (the layout ray() reads), with the source's conventions at the output's size
inline void make_equirect_tables(int out_cols, int out_rows, double* eq /* 2 * (out_cols + out_rows) */) {
  for (int u = 0; u < out_cols; ++u) {
    const double lon = ((u + 0.5) / out_cols - 0.5) * kTwoPi;
    eq[u] = cos(lon); eq[out_cols + u] = sin(lon);
  }
  for (int v = 0; v < out_rows; ++v) {
    const double lat = ((out_rows * 0.5 - (v + 0.5)) * kTwoPi) / out_cols;
    eq[2 * out_cols + v] = cos(lat); eq[2 * out_cols + out_rows + v] = sin(lat);
  }
}

// the rectilinear view's tan(hfov / 2)
inline double tan_half_fov(double hfov_deg) { return tan((hfov_deg * kPi) / 360.0); }

// R = Rz(yaw) Ry(-pitch) Rx(roll), multiplied out
inline void rotation(double yaw_deg, double pitch_deg, double roll_deg, double* R) {
  const double yaw = (yaw_deg * kPi) / 180.0, pitch = (pitch_deg * kPi) / 180.0, roll = (roll_deg * kPi) / 180.0;
  const double cy = cos(yaw), sy = sin(yaw), cp = cos(pitch), sp = sin(pitch), cr = cos(roll), sr = sin(roll);
  R[0] = cy * cp; R[1] = -(sy * cr) - (cy * sp) * sr; R[2] = sy * sr - (cy * sp) * cr;
  R[3] = sy * cp; R[4] = cy * cr - (sy * sp) * sr;    R[5] = -(cy * sr) - (sy * sp) * cr;
  R[6] = sp;      R[7] = cp * sr;                     R[8] = cp * cr;
}

}  // namespace reproject
}  // namespace pf
