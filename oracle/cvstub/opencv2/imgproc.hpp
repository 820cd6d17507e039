// oracle/cvstub/opencv2/imgproc.hpp  --  TEST INFRASTRUCTURE ONLY (see core.hpp).
//
// The image primitives the reference calls.  Where the oracle (oracle/pixflow_oracle.cpp) already has a body, the call is
// delegated to its export, so the reference's own text and the oracle's restatement of it meet on the SAME primitive
// arithmetic; what is restated here is pure data movement or integer arithmetic.  DESIGN.md section 6 has the table.
// Anything the reference does not pass (another kernel size, border, interpolation, type) aborts with a message.
#ifndef CVSTUB_OPENCV2_IMGPROC_HPP
#define CVSTUB_OPENCV2_IMGPROC_HPP

#include <cstdint>

#include "opencv2/core.hpp"

extern "C" {
void orc_resize_cubic_u8(const uint8_t* src, int sw, int sh, int cn, uint8_t* dst, int dw, int dh);
void orc_resize_linear_f32(const float* src, int sw, int sh, int cn, float* dst, int dw, int dh);
void orc_resize_cubic_f32(const float* src, int sw, int sh, int cn, float* dst, int dw, int dh);
void orc_gaussian_blur_f32(const float* src, int w, int h, int cn, int ksize, double sigma, float* dst);
void orc_sobel1(const float* src, int w, int h, int dx, int dy, float* dst);
void orc_median5(const float* src, int w, int h, int cn, float* dst);
void orc_box_blur_roi(float* img, int w, int h, int x0, int y0, int rw, int rh, int k);
}

enum { CV_INTER_NN = 0, CV_INTER_LINEAR = 1, CV_INTER_CUBIC = 2 };
enum { CV_BGRA2GRAY = 10, CV_HSV2BGR = 54 };
enum { CV_THRESH_BINARY = 0 };
enum { CV_AA = 16 };

namespace cv {

enum { INTER_NEAREST = 0, INTER_LINEAR = 1, INTER_CUBIC = 2, WARP_INVERSE_MAP = 16 };
enum { THRESH_BINARY = 0 };
enum { COLOR_BGRA2GRAY = 10, COLOR_HSV2BGR = 54 };

// the driver's "pyramid sizes only" command switches the resize arithmetic off (the destination is still allocated)
inline bool& cvstub_resize_sizes_only() { static bool v = false; return v; }

inline Mat cvstub_packed(const Mat& m) { return m.isContinuous() ? m : m.clone(); }

inline void resize(const Mat& src_, Mat& dst, Size dsize, double fx = 0, double fy = 0, int interpolation = INTER_LINEAR) {
  if (fx != 0 || fy != 0 || dsize.width <= 0 || dsize.height <= 0) cvstub_die("resize: only an explicit, non-empty destination size");
  if (src_.empty()) cvstub_die("resize: empty source");
  const Mat src = cvstub_packed(src_);
  Mat out(dsize, src.type());
  const int cn = src.channels();
  if (cvstub_resize_sizes_only()) { dst = out; return; }
  if (src.depth() == CV_8U && interpolation == INTER_CUBIC)
    orc_resize_cubic_u8(src.data, src.cols, src.rows, cn, out.data, out.cols, out.rows);
  else if (src.depth() == CV_32F && interpolation == INTER_CUBIC)
    orc_resize_cubic_f32(src.ptr<float>(), src.cols, src.rows, cn, out.ptr<float>(), out.cols, out.rows);
  else if (src.depth() == CV_32F && interpolation == INTER_LINEAR)
    orc_resize_linear_f32(src.ptr<float>(), src.cols, src.rows, cn, out.ptr<float>(), out.cols, out.rows);
  else cvstub_die("resize: only cubic (8U, 32F) and linear (32F)");
  dst = out;
}

inline void GaussianBlur(const Mat& src_, Mat& dst, Size ksize, double sigmaX, double sigmaY = 0, int borderType = BORDER_DEFAULT) {
  if (src_.depth() != CV_32F || ksize.width != ksize.height || (ksize.width & 1) == 0 || sigmaX <= 0 || sigmaY != 0 || borderType != BORDER_DEFAULT)
    cvstub_die("GaussianBlur: only CV_32F, a square odd kernel, sigmaX > 0, sigmaY = 0, the default border");
  const Mat src = cvstub_packed(src_);
  Mat out(src.rows, src.cols, src.type());
  orc_gaussian_blur_f32(src.ptr<float>(), src.cols, src.rows, src.channels(), ksize.width, sigmaX, out.ptr<float>());
  dst = out;
}

inline void Sobel(const Mat& src_, Mat& dst, int ddepth, int dx, int dy, int ksize = 3, double scale = 1, double delta = 0, int borderType = BORDER_DEFAULT) {
  if (src_.type() != CV_32FC1 || ddepth != -1 || ksize != 1 || scale != 1 || delta != 0 || borderType != BORDER_REPLICATE || dx + dy != 1 || dx < 0 || dy < 0)
    cvstub_die("Sobel: only CV_32FC1, same depth, ksize 1, one first derivative, scale 1, delta 0, BORDER_REPLICATE");
  const Mat src = cvstub_packed(src_);
  Mat out(src.rows, src.cols, src.type());
  orc_sobel1(src.ptr<float>(), src.cols, src.rows, dx, dy, out.ptr<float>());
  dst = out;
}

inline void medianBlur(const Mat& src_, Mat& dst, int ksize) {
  if (src_.depth() != CV_32F || ksize != 5) cvstub_die("medianBlur: only CV_32F, ksize 5");
  const Mat src = cvstub_packed(src_);
  Mat out(src.rows, src.cols, src.type());
  orc_median5(src.ptr<float>(), src.cols, src.rows, src.channels(), out.ptr<float>());
  dst = out;
}

// blur(): the reference blurs in place, the whole image or a tile VIEW of it, and relies on OpenCV reading the pixels around
// a view from the parent image (a non-isolated ROI).  So the parent and the view's offset go to the oracle's body.
inline void blur(const Mat& src, Mat& dst, Size ksize) {
  if (src.type() != CV_32FC1 || dst.data != src.data || dst.rows != src.rows || dst.cols != src.cols) cvstub_die("blur: only CV_32FC1, in place");
  if (ksize.width != ksize.height || ksize.width <= 0) cvstub_die("blur: only a square kernel of positive width (OpenCV asserts on width 0)");
  if (src.empty()) return;
  orc_box_blur_roi((float*)dst.wholeData(), dst.wholeCols, dst.wholeRows, dst.ofsX, dst.ofsY, dst.cols, dst.rows, ksize.width);
}

// restated here: 8-bit BGR(A) -> grey in 14-bit fixed point, as OpenCV documents its 8U path (B 1868, G 9617, R 4899, round half up)
inline void cvtColor(const Mat& src, Mat& dst, int code) {
  if (code != COLOR_BGRA2GRAY || src.type() != CV_8UC4) cvstub_die("cvtColor: only BGRA2GRAY on CV_8UC4 (visualisers are out of scope)");
  Mat out(src.rows, src.cols, CV_8UC1);
  for (int y = 0; y < src.rows; ++y)
    for (int x = 0; x < src.cols; ++x) {
      const uchar* p = src.ptr<uchar>(y) + 4 * x;
      out.at<uchar>(y, x) = (uchar)((p[0] * 1868 + p[1] * 9617 + p[2] * 4899 + (1 << 13)) >> 14);
    }
  dst = out;
}

// restated here: dst = src > thresh ? maxval : 0 on CV_8UC1; may run in place
inline double threshold(const Mat& src, Mat& dst, double thresh, double maxval, int type) {
  if (type != THRESH_BINARY || src.type() != CV_8UC1) cvstub_die("threshold: only THRESH_BINARY on CV_8UC1");
  // OpenCV's 8U path compares against floor(thresh) and stores round(maxval), saturated
  const int it = (int)std::floor(thresh);
  long im = std::lrint(maxval); im = im < 0 ? 0 : im > 255 ? 255 : im;
  Mat out(src.rows, src.cols, CV_8UC1);
  for (int y = 0; y < src.rows; ++y)
    for (int x = 0; x < src.cols; ++x) out.at<uchar>(y, x) = (uchar)(src.at<uchar>(y, x) > it ? im : 0);
  if (dst.data == src.data && dst.rows == src.rows && dst.cols == src.cols) out.copyTo(dst); else dst = out;
  return thresh;
}

// restated here: only what the reference passes -- the forward map [1 0 tx; 0 1 0; 0 0 1] with an integer tx, nearest
// neighbour, a constant border.  dst(y, x) = src(y, x - tx), the border value where that leaves the source.
inline void warpPerspective(const Mat& src_, Mat& dst, const Mat& M, Size dsize, int flags = INTER_LINEAR, int borderMode = BORDER_CONSTANT,
                            const Scalar& borderValue = Scalar()) {
  if (M.type() != CV_64FC1 || M.rows != 3 || M.cols != 3) cvstub_die("warpPerspective: M must be 3x3 CV_64F");
  const double* m0 = M.ptr<double>(0); const double* m1 = M.ptr<double>(1); const double* m2 = M.ptr<double>(2);
  const double tx = m0[2];
  if (m0[0] != 1 || m0[1] != 0 || m1[0] != 0 || m1[1] != 1 || m1[2] != 0 || m2[0] != 0 || m2[1] != 0 || m2[2] != 1 || tx != std::floor(tx) ||
      flags != INTER_NEAREST || borderMode != BORDER_CONSTANT)
    cvstub_die("warpPerspective: only a pure integer x-translation with INTER_NEAREST and BORDER_CONSTANT");
  if (src_.depth() != CV_8U) cvstub_die("warpPerspective: only CV_8U");
  const Mat src(src_);  // dst may be the same header (StitchTool.cpp warps Map into Map): keep the source alive
  const int cn = src.channels(), t = (int)tx;
  Mat out(dsize, src.type());
  for (int y = 0; y < out.rows; ++y)
    for (int x = 0; x < out.cols; ++x)
      for (int c = 0; c < cn; ++c) {
        const int sx = x - t;
        const double b = borderValue.val[c < 4 ? c : 3];
        out.ptr<uchar>(y)[x * cn + c] = (sx >= 0 && sx < src.cols && y < src.rows) ? src.ptr<uchar>(y)[sx * cn + c] : (uchar)(b < 0 ? 0 : b > 255 ? 255 : std::lrint(b));
      }
  dst = out;
}

// visualisers only: out of scope
inline void line(Mat&, Point, Point, const Scalar&, int = 1, int = 8, int = 0) { cvstub_die("line: not provided (visualisers are out of scope)"); }

}  // namespace cv

#endif
