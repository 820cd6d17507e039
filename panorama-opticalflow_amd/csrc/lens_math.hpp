// The geometry of the lens remap, one copy for the kernel (kernels_lens.hip), the host API (pf_api_lens.inl) and the
// host-run test: a canvas pixel's ray, its rotation into the camera, the lens model's radius, the radial polynomial, the position in
// the photo and its quantisation to 8 fractional bits.  The rules are reproject_math.hpp's: fp64 add, subtract, multiply, divide and
// sqrt only, every product and sum rounded on its own (-ffp-contract=off), in exactly the order written here; the one arctangent is
// reproject::atan2_poly.  tests/lens_model.py restates it.  The host-only part makes focal_px from a field of view (the host's tan /
// sin) and the rotation of a posed camera.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "reproject_math.hpp"

namespace pf {
namespace lens {

#define PF_LENS_FN __host__ __device__ __forceinline__

// the numbering of include/panoflow.h (PF_LENS_*)
constexpr int kRectilinear = 0, kEquidistant = 1, kStereographic = 2, kEquisolid = 3;

// one camera: the kernel's per-image argument, the model's parameters (pf_lens without its filter)
struct Lens {
  int model;
  int crop_cx256, crop_cy256, crop_r256;   // the image circle in 1/256 px; crop_r256 == 0: none
  double focal_px;
  double a, b, c, dd;                      // s = ((a rn + b) rn + c) rn + dd
  double shift_x, shift_y;
  double min_cos;                          // outside where c.x <= min_cos * |c|
  double rot[9];                           // c = rot * d, row-major
};

// what a launch knows of all its images
struct Geometry {
  int filter;
  int photo_cols, photo_rows;
  int cols, rows;   // the canvas
};

// the ray of canvas pixel (i, j).  eq: reproject::make_equirect_tables(cols, rows)
PF_LENS_FN void ray(const Geometry& g, int i, int j, const double* eq, double d[3]) {
  const double cl = eq[i], sl = eq[g.cols + i], cb = eq[2 * g.cols + j], sb = eq[2 * g.cols + g.rows + j];
  d[0] = cb * cl; d[1] = cb * sl; d[2] = sb;
}

// c = rot d; the outside exits; g of the model; the polynomial; the position; 256 * position + 1/2, floored.  A pixel the camera does
// not see, or whose position is no number within +-1e9, is outside: fx = 0, fy = INT32_MIN.
PF_LENS_FN void photo_fixed(const Geometry& g, const Lens& l, const double d[3], int* fx, int* fy) {
  *fx = 0; *fy = INT32_MIN;
  const double* R = l.rot;
  const double cx = (R[0] * d[0] + R[1] * d[1]) + R[2] * d[2];
  const double cy = (R[3] * d[0] + R[4] * d[1]) + R[5] * d[2];
  const double cz = (R[6] * d[0] + R[7] * d[1]) + R[8] * d[2];
  const double rho = sqrt(cy * cy + cz * cz);
  const double n = sqrt((cx * cx + cy * cy) + cz * cz);
  if (n == 0.0 || cx <= l.min_cos * n) return;
  double gr;
  if (l.model == kRectilinear) gr = rho / cx;
  else if (l.model == kEquidistant) gr = reproject::atan2_poly(rho, cx);
  else {
    const double m = n + cx;
    if (m <= 0.0) return;
    gr = (2.0 * rho) / (l.model == kStereographic ? m : sqrt((2.0 * n) * m));
  }
  const double r = l.focal_px * gr;
  const int side = g.photo_cols < g.photo_rows ? g.photo_cols : g.photo_rows;
  const double rn = r / (side * 0.5);
  const double s = ((l.a * rn + l.b) * rn + l.c) * rn + l.dd;
  const double r_src = r * s;
  const double k = rho == 0.0 ? 0.0 : r_src / rho;
  const double px = ((g.photo_cols * 0.5 - 0.5) + l.shift_x) + k * cy;
  const double py = ((g.photo_rows * 0.5 - 0.5) + l.shift_y) - k * cz;
  const double qx = 256.0 * px + 0.5, qy = 256.0 * py + 0.5;
  const bool number = qx >= -1.0e9 && qx <= 1.0e9 && qy >= -1.0e9 && qy <= 1.0e9;   // false for a NaN
  if (!number) return;
  *fx = reproject::floor_int(qx); *fy = reproject::floor_int(qy);
}

// within half a pixel of the photo, and within the image circle if there is one.  The differences are below 2^32 in magnitude, so the
// sum of their squares fits 64 unsigned bits.
PF_LENS_FN bool inside(const Geometry& g, const Lens& l, int fx, int fy) {
  if (fx < -128 || fx > 256 * (g.photo_cols - 1) + 128 || fy < -128 || fy > 256 * (g.photo_rows - 1) + 128) return false;
  if (l.crop_r256 <= 0) return true;
  const long long dx = (long long)fx - l.crop_cx256, dy = (long long)fy - l.crop_cy256;
  const unsigned long long ux = (unsigned long long)(dx < 0 ? -dx : dx), uy = (unsigned long long)(dy < 0 ? -dy : dy), ur = (unsigned long long)l.crop_r256;
  return ux * ux + uy * uy <= ur * ur;
}

#undef PF_LENS_FN

// ---- host only ----

// focal_px of a photo photo_cols wide that spans hfov_deg degrees across, by the model's own r(theta): f theta, f tan theta,
// 2 f tan(theta / 2), 2 f sin(theta / 2), with r = photo_cols / 2 at theta = hfov / 2
inline double focal(int model, int photo_cols, double hfov_deg) {
  const double hfov = (hfov_deg * reproject::kPi) / 180.0;
  switch (model) {
    case kRectilinear: return (photo_cols * 0.5) / tan(hfov * 0.5);
    case kEquidistant: return photo_cols / hfov;
    case kStereographic: return (photo_cols * 0.5) / (2.0 * tan(hfov * 0.25));
    case kEquisolid: return (photo_cols * 0.5) / (2.0 * sin(hfov * 0.25));
    default: return 0.0;
  }
}

// the rot of a camera posed by R = reproject::rotation(yaw, pitch, roll): its transpose (world -> camera)
inline void rotation(double yaw_deg, double pitch_deg, double roll_deg, double* rot) {
  double R[9];
  reproject::rotation(yaw_deg, pitch_deg, roll_deg, R);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) rot[3 * i + j] = R[3 * j + i];
}

}  // namespace lens
}  // namespace pf
