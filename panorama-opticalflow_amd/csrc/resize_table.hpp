// The resize passes' tables (kernels_resize.hip), host code: Pillow's precompute_coeffs and normalize_coeffs_8bpc restated.  For one axis
// of `in` source and `out` output samples, per output index the first source index and the tap count, and the taps as 22-bit
// fixed-point integers.  Doubles throughout, evaluated in Pillow's order (the translation units that include this are built without
// FMA contraction); HAMMING and LANCZOS go through the host's sin / cos, so their tables are this libm's.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

namespace resize_table {

enum { kLanczos = 1, kBilinear = 2, kBicubic = 3, kBox = 4, kHamming = 5 };   // Pillow's numbering (PF_RESIZE_* in panoflow.h)
constexpr int kPrecBits = 22;
// Largest table of one axis, in coefficients (rows() * out): 64 MiB of int32.  A LANCZOS downscale needs about 6 * in + out of them, an
// upscale 7 * out, so every axis up to 2.7 million source or 2.3 million output samples fits; beyond it the call is refused.
constexpr double kMaxCoefs = 16777216.0;

inline bool known(int filter) { return filter >= kLanczos && filter <= kHamming; }

inline double support_of(int filter) {
  switch (filter) {
    case kLanczos: return 3.0;
    case kBicubic: return 2.0;
    case kBox: return 0.5;
    default: return 1.0;   // BILINEAR, HAMMING
  }
}

inline double sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}

inline double weight(int filter, double x) {
  switch (filter) {
    case kBox: return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    case kBilinear:
      if (x < 0.0) x = -x;
      return x < 1.0 ? 1.0 - x : 0.0;
    case kHamming:
      if (x < 0.0) x = -x;
      if (x == 0.0) return 1.0;
      if (x >= 1.0) return 0.0;
      x = x * M_PI;
      return sin(x) / x * (0.54f + 0.46f * cos(x));   // Pillow's single-precision literals, widened
    case kBicubic: {
      const double a = -0.5;
      if (x < 0.0) x = -x;
      if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
      if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
      return 0.0;
    }
    default:   // LANCZOS
      return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0;
  }
}

// Pillow's ksize: an upper bound of every output's tap count, known before any table is made
inline double rows_bound(int in, int out, int filter) {
  const double scale = (double)in / out;
  return ceil(support_of(filter) * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}
inline bool fits(int in, int out, int filter) { return rows_bound(in, out, filter) * out <= kMaxCoefs; }

struct Table {
  int in = 0, out = 0, filter = 0;
  int rows = 0;              // the largest tap count of any output (>= 1)
  std::vector<int> bounds;   // out pairs: first source index, taps
  std::vector<int> k;        // rows x out, tap-major: k[t * out + index]; zero past an output's taps
};

inline void make(int in, int out, int filter, Table* t) {
  t->in = in; t->out = out; t->filter = filter;
  const double scale = (double)in / out, fs = scale < 1.0 ? 1.0 : scale, support = support_of(filter) * fs, ss = 1.0 / fs;
  t->bounds.assign(size_t(out) * 2, 0);
  int rows = 1;
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    t->bounds[2 * xx] = xmin; t->bounds[2 * xx + 1] = xmax - xmin;
    if (xmax - xmin > rows) rows = xmax - xmin;
  }
  t->rows = rows;
  t->k.assign(size_t(rows) * out, 0);
  std::vector<double> w(rows);
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    const int xmin = t->bounds[2 * xx], n = t->bounds[2 * xx + 1];
    double ww = 0.0;
    for (int x = 0; x < n; ++x) { w[x] = weight(filter, (x + xmin - center + 0.5) * ss); ww += w[x]; }
    for (int x = 0; x < n; ++x) {
      if (ww != 0.0) w[x] /= ww;
      t->k[size_t(x) * out + xx] = w[x] < 0 ? (int)(-0.5 + w[x] * (1 << kPrecBits)) : (int)(0.5 + w[x] * (1 << kPrecBits));
    }
  }
}

}  // namespace resize_table
