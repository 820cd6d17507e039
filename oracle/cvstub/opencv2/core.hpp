// =============================================================================================
// oracle/cvstub/opencv2/core.hpp  --  TEST INFRASTRUCTURE ONLY.
//
// A stand-in for the part of OpenCV's core module that the reference's PixFlow.hpp,
// OpticalFlow.hpp/.cpp, StitchTool.hpp/.cpp and util.hpp use, so that those files compile
// unmodified (oracle/Makefile, target refcore).  Own text: written from OpenCV's documented
// behaviour of each call, it holds nothing of OpenCV's or the reference's sources.
//
// What is here: value types (Point_, Size, Rect, Range, Scalar, Vec), a reference-counted Mat
// whose buffer is an exact-size zeroed heap block (host AddressSanitizer sees every access
// outside it), ROI views that remember their parent, and the few MatExpr forms the reference
// writes.  Every arithmetic body the stand-in supplies is listed in DESIGN.md section 6.
// =============================================================================================
#ifndef CVSTUB_OPENCV2_CORE_HPP
#define CVSTUB_OPENCV2_CORE_HPP

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

typedef unsigned char uchar;

// depth / type codes (documented values)
#define CV_8U 0
#define CV_32F 5
#define CV_64F 6
#define CV_CN_SHIFT 3
#define CV_MAKETYPE(depth, cn) ((depth) + (((cn) - 1) << CV_CN_SHIFT))
#define CV_8UC1 CV_MAKETYPE(CV_8U, 1)
#define CV_8UC3 CV_MAKETYPE(CV_8U, 3)
#define CV_8UC4 CV_MAKETYPE(CV_8U, 4)
#define CV_32FC1 CV_MAKETYPE(CV_32F, 1)
#define CV_32FC2 CV_MAKETYPE(CV_32F, 2)
#define CV_64FC1 CV_MAKETYPE(CV_64F, 1)

namespace cv {

[[noreturn]] inline void cvstub_die(const char* what) {
  std::fprintf(stderr, "cvstub: %s\n", what);
  std::abort();
}

// ---------------------------------------------------------------------------------------------
// value types.  Every constructor and operator takes its scalars BY VALUE (as OpenCV does): the
// reference passes static constexpr members, which must not be ODR-used under -std=c++11.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct Point_ {
  T x, y;
  Point_() : x(0), y(0) {}
  Point_(T x_, T y_) : x(x_), y(y_) {}
  T dot(const Point_& p) const { return T(x * p.x + y * p.y); }  // in T: float stays float
  Point_& operator+=(const Point_& b) { x = T(x + b.x); y = T(y + b.y); return *this; }
  Point_& operator-=(const Point_& b) { x = T(x - b.x); y = T(y - b.y); return *this; }
  Point_& operator*=(float a) { x = T(x * a); y = T(y * a); return *this; }
  Point_& operator/=(float a) { x = T(x / a); y = T(y / a); return *this; }
};
template <typename T> inline Point_<T> operator+(const Point_<T>& a, const Point_<T>& b) { return Point_<T>(T(a.x + b.x), T(a.y + b.y)); }
template <typename T> inline Point_<T> operator-(const Point_<T>& a, const Point_<T>& b) { return Point_<T>(T(a.x - b.x), T(a.y - b.y)); }
template <typename T> inline Point_<T> operator*(float a, const Point_<T>& b) { return Point_<T>(T(b.x * a), T(b.y * a)); }
template <typename T> inline Point_<T> operator*(const Point_<T>& b, float a) { return Point_<T>(T(b.x * a), T(b.y * a)); }
typedef Point_<float> Point2f;
typedef Point_<int> Point;
// documented: the L2 norm of a point is computed and returned in double
template <typename T> inline double norm(const Point_<T>& p) { return std::sqrt((double)p.x * p.x + (double)p.y * p.y); }

struct Size {
  int width, height;
  Size() : width(0), height(0) {}
  Size(int w, int h) : width(w), height(h) {}
  bool operator==(const Size& o) const { return width == o.width && height == o.height; }
  bool operator!=(const Size& o) const { return !(*this == o); }
};
struct Rect {
  int x, y, width, height;
  Rect() : x(0), y(0), width(0), height(0) {}
  Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {}
};
struct Range {
  int start, end;
  Range() : start(0), end(0) {}
  Range(int s, int e) : start(s), end(e) {}
};
struct Scalar {
  double val[4];
  Scalar(double a = 0, double b = 0, double c = 0, double d = 0) { val[0] = a; val[1] = b; val[2] = c; val[3] = d; }
  double operator[](int i) const { return val[i]; }
};
template <typename T, int N>
struct Vec {
  T val[N];
  Vec() { for (int i = 0; i < N; ++i) val[i] = T(0); }
  Vec(T a, T b) { static_assert(N == 2, "2 elements"); val[0] = a; val[1] = b; }
  Vec(T a, T b, T c) { static_assert(N == 3, "3 elements"); val[0] = a; val[1] = b; val[2] = c; }
  Vec(T a, T b, T c, T d) { static_assert(N == 4, "4 elements"); val[0] = a; val[1] = b; val[2] = c; val[3] = d; }
  T& operator[](int i) { return val[i]; }
  const T& operator[](int i) const { return val[i]; }
};
typedef Vec<uchar, 4> Vec4b;
typedef Vec<uchar, 3> Vec3b;
typedef Vec<float, 2> Vec2f;

// ---------------------------------------------------------------------------------------------
// Mat
// ---------------------------------------------------------------------------------------------
class Mat {
  struct Buf { uchar* p; int refs; };
  Buf* buf_;
  int type_;
  void retain() { if (buf_) ++buf_->refs; }
  void release() {
    if (buf_ && --buf_->refs == 0) { std::free(buf_->p); delete buf_; }
    buf_ = nullptr;
  }

 public:
  int rows, cols;
  size_t step;  // bytes between rows
  uchar* data;
  // the allocation this header looks into (a view keeps its parent's extent; own == whole otherwise)
  int wholeRows, wholeCols, ofsX, ofsY;

  Mat() : buf_(nullptr), type_(0), rows(0), cols(0), step(0), data(nullptr), wholeRows(0), wholeCols(0), ofsX(0), ofsY(0) {}
  Mat(int r, int c, int type) : Mat() { create(r, c, type); }
  Mat(Size s, int type) : Mat() { create(s.height, s.width, type); }
  Mat(int r, int c, int type, const Scalar& s) : Mat() { create(r, c, type); setTo(s); }
  Mat(const Mat& m)
      : buf_(m.buf_), type_(m.type_), rows(m.rows), cols(m.cols), step(m.step), data(m.data), wholeRows(m.wholeRows),
        wholeCols(m.wholeCols), ofsX(m.ofsX), ofsY(m.ofsY) { retain(); }
  Mat(const Mat& m, const Rect& r) : Mat(m) { narrow(r.y, r.y + r.height, r.x, r.x + r.width); }
  Mat& operator=(const Mat& m) {
    if (this != &m) {
      Buf* keep = m.buf_;
      if (keep) ++keep->refs;
      release();
      buf_ = keep; type_ = m.type_; rows = m.rows; cols = m.cols; step = m.step; data = m.data;
      wholeRows = m.wholeRows; wholeCols = m.wholeCols; ofsX = m.ofsX; ofsY = m.ofsY;
    }
    return *this;
  }
  ~Mat() { release(); }

  // a fresh, zero-filled, exact-size block (the reference reads `motion` before writing it)
  void create(int r, int c, int type) {
    if (r < 0 || c < 0) cvstub_die("Mat::create: negative size");
    release();
    type_ = type; rows = r; cols = c;
    step = (size_t)c * elemSize();
    const size_t n = step * (size_t)r;
    buf_ = new Buf{(uchar*)std::calloc(n ? n : 1, 1), 1};
    if (!buf_->p) cvstub_die("Mat::create: out of memory");
    data = buf_->p; wholeRows = r; wholeCols = c; ofsX = ofsY = 0;
  }
  static Mat zeros(Size s, int type) { return Mat(s, type); }
  static Mat zeros(int r, int c, int type) { return Mat(r, c, type); }

  int type() const { return type_; }
  int depth() const { return type_ & ((1 << CV_CN_SHIFT) - 1); }
  int channels() const { return (type_ >> CV_CN_SHIFT) + 1; }
  size_t elemSize1() const { return depth() == CV_8U ? 1 : depth() == CV_32F ? 4 : depth() == CV_64F ? 8 : (cvstub_die("unsupported depth"), 0); }
  size_t elemSize() const { return elemSize1() * channels(); }
  Size size() const { return Size(cols, rows); }
  bool empty() const { return data == nullptr || rows == 0 || cols == 0; }
  bool isContinuous() const { return step == (size_t)cols * elemSize() || rows <= 1; }
  const uchar* wholeData() const { return buf_ ? buf_->p : nullptr; }
  uchar* wholeData() { return buf_ ? buf_->p : nullptr; }

  template <typename T> T& at(int y, int x) { check_at(y, x, sizeof(T)); return *(T*)(data + (size_t)y * step + (size_t)x * sizeof(T)); }
  template <typename T> const T& at(int y, int x) const { check_at(y, x, sizeof(T)); return *(const T*)(data + (size_t)y * step + (size_t)x * sizeof(T)); }
  template <typename T> T* ptr(int y = 0) { return (T*)(data + (size_t)y * step); }
  template <typename T> const T* ptr(int y = 0) const { return (const T*)(data + (size_t)y * step); }

  Mat operator()(const Range& rr, const Range& cr) const { Mat v(*this); v.narrow(rr.start, rr.end, cr.start, cr.end); return v; }
  Mat operator()(const Rect& r) const { return Mat(*this, r); }

  Mat clone() const { Mat m; copyTo(m); return m; }
  // OpenCV's OutputArray binds to temporaries (the reference copies into Mat(m, Rect) rvalues): a destination of the
  // right size and type is written in place (a view stays a view), anything else is reallocated.
  void copyTo(const Mat& dst_) const {
    Mat& dst = const_cast<Mat&>(dst_);
    if (dst.data == data && dst.rows == rows && dst.cols == cols && dst.type_ == type_ && dst.step == step) return;
    if (dst.rows != rows || dst.cols != cols || dst.type_ != type_ || !dst.data) {
      Mat keep(*this);  // dst may be *this' own header
      dst.create(rows, cols, type_);
      keep.copyRowsTo(dst);
      return;
    }
    copyRowsTo(dst);
  }
  // only the conversions the reference performs; no scale (the MatExpr scalar forms below carry the scaling)
  void convertTo(Mat& dst, int rtype) const {
    const int ddepth = rtype < 0 ? depth() : (rtype & 7), cn = channels();
    Mat out(rows, cols, CV_MAKETYPE(ddepth, cn));
    for (int y = 0; y < rows; ++y)
      for (int i = 0; i < cols * cn; ++i) {
        if (depth() == CV_8U && ddepth == CV_32F) out.ptr<float>(y)[i] = (float)ptr<uchar>(y)[i];
        else if (depth() == CV_32F && ddepth == CV_32F) out.ptr<float>(y)[i] = ptr<float>(y)[i];
        else if (depth() == CV_8U && ddepth == CV_8U) out.ptr<uchar>(y)[i] = ptr<uchar>(y)[i];
        else cvstub_die("Mat::convertTo: conversion not provided by the stand-in");
      }
    dst = out;
  }
  // per-element product; only uchar (saturated), as StitchTool.cpp uses it
  Mat mul(const Mat& m) const {
    if (type_ != CV_8UC1 || m.type_ != CV_8UC1 || m.rows != rows || m.cols != cols) cvstub_die("Mat::mul: only equal-size CV_8UC1");
    Mat out(rows, cols, type_);
    for (int y = 0; y < rows; ++y)
      for (int x = 0; x < cols; ++x) {
        const int v = (int)at<uchar>(y, x) * (int)m.at<uchar>(y, x);
        out.at<uchar>(y, x) = (uchar)(v > 255 ? 255 : v);
      }
    return out;
  }
  void setTo(const Scalar& s) {
    const int cn = channels();
    for (int y = 0; y < rows; ++y)
      for (int x = 0; x < cols; ++x)
        for (int c = 0; c < cn; ++c) {
          const double v = s.val[c < 4 ? c : 3];
          if (depth() == CV_8U) ptr<uchar>(y)[x * cn + c] = (uchar)(v < 0 ? 0 : v > 255 ? 255 : std::lrint(v));
          else if (depth() == CV_32F) ptr<float>(y)[x * cn + c] = (float)v;
          else if (depth() == CV_64F) ptr<double>(y)[x * cn + c] = v;
        }
  }

 private:
  void narrow(int r0, int r1, int c0, int c1) {
    if (r0 < 0 || r1 > rows || r0 > r1 || c0 < 0 || c1 > cols || c0 > c1) cvstub_die("Mat: ROI outside its parent");
    data += (size_t)r0 * step + (size_t)c0 * elemSize();
    ofsX += c0; ofsY += r0; rows = r1 - r0; cols = c1 - c0;
  }
  void copyRowsTo(Mat& dst) const {
    const size_t n = (size_t)cols * elemSize();
    for (int y = 0; y < rows; ++y) std::memmove(dst.data + (size_t)y * dst.step, data + (size_t)y * step, n);
  }
  void check_at(int y, int x, size_t esz) const {
#ifdef CVSTUB_CHECK_AT
    // OpenCV's release build does not check; the sanitized driver does, because an access past the end of a ROW stays
    // inside the heap block and AddressSanitizer cannot see it.
    if (y < 0 || y >= rows || x < 0 || (size_t)(x + 1) * esz > (size_t)cols * elemSize()) cvstub_die("Mat::at outside the matrix");
#else
    (void)y; (void)x; (void)esz;
#endif
  }
};

// Mat_<T>(r, c) << a, b, c ...   (only to build the 3x3 shift matrix)
template <typename T> struct Mat_;
template <typename T>
struct MatCommaInitializer_ {
  Mat m; int n;
  MatCommaInitializer_(const Mat& m_) : m(m_), n(0) {}
  template <typename V> MatCommaInitializer_& operator,(V v) {
    if (n >= m.rows * m.cols) cvstub_die("Mat_ <<: too many elements");
    m.at<T>(n / m.cols, n % m.cols) = (T)v; ++n; return *this;
  }
  operator Mat() const { return m; }
};
template <typename T>
struct Mat_ : public Mat {
  Mat_(int r, int c) : Mat(r, c, sizeof(T) == 8 ? CV_64FC1 : sizeof(T) == 4 ? CV_32FC1 : CV_8UC1) {}
};
template <typename T, typename V>
inline MatCommaInitializer_<T> operator<<(const Mat_<T>& m, V v) { MatCommaInitializer_<T> ci(m); return (ci, v); }

// ---------------------------------------------------------------------------------------------
// The MatExpr forms the reference writes.  OpenCV evaluates `m * s`, `m *= s`, `m /= s` on CV_32F as convertTo with a
// scale: the double factor (1/s for a division) is narrowed to float, and each element becomes src * factor + 0.
// ---------------------------------------------------------------------------------------------
inline void cvstub_scale_f32(const Mat& src, Mat& dst, double factor) {
  if (src.depth() != CV_32F) cvstub_die("Mat scalar product: only CV_32F");
  const float a = (float)factor;
  const int cn = src.channels();
  Mat out(src.rows, src.cols, src.type());
  for (int y = 0; y < src.rows; ++y) {
    const float* s = src.ptr<float>(y); float* d = out.ptr<float>(y);
    for (int i = 0; i < src.cols * cn; ++i) d[i] = s[i] * a + 0.0f;
  }
  if (dst.rows == out.rows && dst.cols == out.cols && dst.type() == out.type() && dst.data) out.copyTo(dst);  // in place: views stay views
  else dst = out;
}
inline Mat operator*(const Mat& m, double s) { Mat out; cvstub_scale_f32(m, out, s); return out; }
inline Mat& operator*=(Mat& m, double s) { cvstub_scale_f32(m, m, s); return m; }
inline Mat& operator/=(Mat& m, double s) { cvstub_scale_f32(m, m, 1. / s); return m; }
// Mat + Mat, only CV_8UC1 (saturated)
inline Mat operator+(const Mat& a, const Mat& b) {
  if (a.type() != CV_8UC1 || b.type() != CV_8UC1 || a.rows != b.rows || a.cols != b.cols) cvstub_die("Mat + Mat: only equal-size CV_8UC1");
  Mat out(a.rows, a.cols, a.type());
  for (int y = 0; y < a.rows; ++y)
    for (int x = 0; x < a.cols; ++x) {
      const int v = (int)a.at<uchar>(y, x) + (int)b.at<uchar>(y, x);
      out.at<uchar>(y, x) = (uchar)(v > 255 ? 255 : v);
    }
  return out;
}

// channel split / merge (pure data movement)
inline void split(const Mat& m, std::vector<Mat>& mv) {
  const int cn = m.channels(); const size_t e1 = m.elemSize1();
  mv.assign(cn, Mat());
  for (int c = 0; c < cn; ++c) {
    mv[c].create(m.rows, m.cols, CV_MAKETYPE(m.depth(), 1));
    for (int y = 0; y < m.rows; ++y)
      for (int x = 0; x < m.cols; ++x) std::memcpy(mv[c].data + y * mv[c].step + x * e1, m.data + y * m.step + (x * cn + c) * e1, e1);
  }
}
inline void merge(const std::vector<Mat>& mv, Mat& dst) {
  if (mv.empty()) cvstub_die("merge: nothing to merge");
  const int cn = (int)mv.size(); const size_t e1 = mv[0].elemSize1();
  for (const Mat& m : mv)
    if (m.channels() != 1 || m.depth() != mv[0].depth() || m.rows != mv[0].rows || m.cols != mv[0].cols) cvstub_die("merge: planes differ");
  Mat out(mv[0].rows, mv[0].cols, CV_MAKETYPE(mv[0].depth(), cn));
  for (int c = 0; c < cn; ++c)
    for (int y = 0; y < out.rows; ++y)
      for (int x = 0; x < out.cols; ++x) std::memcpy(out.data + y * out.step + (x * cn + c) * e1, mv[c].data + y * mv[c].step + x * e1, e1);
  dst = out;
}

enum { NORM_MINMAX = 32 };
enum { BORDER_CONSTANT = 0, BORDER_REPLICATE = 1, BORDER_REFLECT_101 = 4, BORDER_DEFAULT = 4 };
// visualisers only: out of scope
inline void normalize(const Mat&, Mat&, double = 1, double = 0, int = NORM_MINMAX, int = -1) { cvstub_die("normalize: not provided (visualisers are out of scope)"); }

namespace detail {}

}  // namespace cv

#endif
