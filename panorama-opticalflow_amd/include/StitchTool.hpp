// Drop-in for the reference's CPU/StitchTool.hpp (:21-61).  Map / overlap masks / blend ramp / composite
// are computed by the StitchTool kernels through pf_stitch_prepare / pf_stitch_gather.
#ifndef StitchTool_hpp
#define StitchTool_hpp

#include <string>
#include <vector>

#include "util.hpp"

namespace stitch_tools {
using namespace panocv;

class Stitchtools {
 public:
  Mat ImageL, ImageR;
  Mat Blend;
  Mat OverlappedL, OverlappedR;
  Mat Mergedmiddle;  // merged image in the overlap
  Mat Map;           // ImageL only: 100; ImageR only: 50; overlap: 150
  Mat FinalResult;
  Mat MergedDis;

  Stitchtools() {}
  ~Stitchtools() {}

  // CPU/StitchTool.cpp:7-36.  One fused device pass (pf_stitch_prepare) = MatchImages() + the overlap masking + GenerateBlend(): nothing can
  // edit Map between them here, so the result is what calling the two public methods in sequence gives.
  void prepare(const Mat& colorImageL, const Mat& colorImageR) {
    if (colorImageL.type() != CV_8UC4 || colorImageR.type() != CV_8UC4 || colorImageL.rows != colorImageR.rows || colorImageL.cols != colorImageR.cols)
      throw util::VrCamException("Stitchtools::prepare: inputs must be two CV_8UC4 images of equal size");
    ImageL = colorImageL.clone();
    ImageR = colorImageR.clone();
    raw_ = Mat(); rawDis_ = Mat();
    const int r = ImageL.rows, c = ImageL.cols;
    Map = Mat(r, c, CV_8UC1); OverlappedL = Mat(r, c, CV_8UC4); OverlappedR = Mat(r, c, CV_8UC4);
    Blend = Mat(r, c, CV_32FC1); MergedDis = Mat(r, c, CV_32FC1);
    pano::check(pf_stitch_prepare(pano::context(), ImageL.data, ImageR.data, c, r, ImageL.step, Map.data, Map.step, OverlappedL.data, OverlappedR.data,
                                  Blend.ptr<float>(), Blend.step, MergedDis.ptr<float>()));
  }
  // CPU/StitchTool.cpp:38-50: Map from the two alpha channels (+ the overlap-masked copies prepare() derives from it, :17-33).
  void MatchImages() {
    if (ImageL.empty()) throw util::VrCamException("Stitchtools::MatchImages: prepare first");
    const int r = ImageL.rows, c = ImageL.cols;
    Map = Mat(r, c, CV_8UC1); OverlappedL = Mat(r, c, CV_8UC4); OverlappedR = Mat(r, c, CV_8UC4);
    pano::check(pf_stitch_match(pano::context(), ImageL.data, ImageR.data, c, r, ImageL.step, Map.data, Map.step, OverlappedL.data, OverlappedR.data));
  }
  // CPU/StitchTool.cpp:98-146: the blend ramp of the CURRENT Map member (a caller may have edited it since MatchImages(), as with the reference).
  void GenerateBlend() {
    if (Map.empty()) throw util::VrCamException("Stitchtools::GenerateBlend: MatchImages first");
    Blend = Mat(Map.rows, Map.cols, CV_32FC1); MergedDis = Mat(Map.rows, Map.cols, CV_32FC1);
    pano::check(pf_stitch_generate_blend(pano::context(), Map.data, Map.step, Map.cols, Map.rows, Blend.ptr<float>(), Blend.step, MergedDis.ptr<float>()));
  }
  // CPU/StitchTool.cpp:148-191.  x is in wrap-extended map coordinates (cols/5 columns were prepended, :102-111).
  // Like the reference it returns the RAW ratio minLdis / (minRdis + minLdis) of that pixel -- not the smoothed ramp --
  // and writes min(minLdis, minRdis) into MergedDis (:185-188).  The device evaluates the 8-direction search for the
  // whole image in one pass (pf_stitch_raw_blend); the result is cached until the next prepare().
  float countblend(const int x, const int y) {
    if (ImageL.empty()) throw util::VrCamException("Stitchtools::countblend: prepare first");
    if (raw_.empty()) {
      raw_ = Mat(ImageL.rows, ImageL.cols, CV_32FC1); rawDis_ = Mat(ImageL.rows, ImageL.cols, CV_32FC1);
      pano::check(pf_stitch_raw_blend(pano::context(), ImageL.data, ImageR.data, ImageL.cols, ImageL.rows, ImageL.step, raw_.ptr<float>(), raw_.step,
                                      rawDis_.ptr<float>()));
    }
    int sx = x - ImageL.cols / 5;
    if (sx < 0) sx += ImageL.cols; else if (sx >= ImageL.cols) sx -= ImageL.cols;
    if (MergedDis.empty()) MergedDis = Mat(ImageL.rows, ImageL.cols, CV_32FC1);
    MergedDis.at<float>(y, sx) = rawDis_.at<float>(y, sx);
    return raw_.at<float>(y, sx);
  }
  // CPU/StitchTool.cpp:52-96
  void Gather() {
    if (Mergedmiddle.empty() || Mergedmiddle.step != ImageL.step) throw util::VrCamException("Stitchtools::Gather: setMergedmiddle first");
    FinalResult = Mat(ImageL.rows, ImageL.cols, CV_8UC4);
    pano::check(pf_stitch_gather(pano::context(), ImageL.data, ImageR.data, Mergedmiddle.data, ImageL.step, Map.data, Map.step, ImageL.cols, ImageL.rows,
                                 FinalResult.data, FinalResult.step));
  }

  Mat getImageL() { return ImageL; }
  Mat getImageR() { return ImageR; }
  Mat getBlend() { return Blend; }
  Mat getMap() { return Map; }
  Mat getOverlappedL() { return OverlappedL; }
  Mat getOverlappedR() { return OverlappedR; }
  Mat getFinalResult() { return FinalResult; }
  void setMergedmiddle(const Mat& image) { Mergedmiddle = image.clone(); }

 private:
  Mat raw_, rawDis_;    // unsmoothed ramp / MergedDis for countblend(), computed on first use
};

// One whole iteration of the stitch loop (CPU/main.cpp:70-95) without leaving the device (pf_stitch_step).
// colorImageR == nullptr chains on the previous call's result, which stays resident in HBM (main.cpp:64-65).
static inline Mat stitchStep(const Mat& colorImageL, const Mat* colorImageR, const std::string& flowAlgName) {
  const int maxPct = pf_max_percentage_by_name(flowAlgName.c_str());
  if (maxPct < 0) throw util::VrCamException("unrecognized flow algorithm name: " + flowAlgName);
  if (colorImageL.type() != CV_8UC4 || (colorImageR && (colorImageR->type() != CV_8UC4 || colorImageR->rows != colorImageL.rows ||
                                                         colorImageR->cols != colorImageL.cols)))
    throw util::VrCamException("stitchStep: inputs must be CV_8UC4 images of equal size");
  std::vector<Mat> im = {colorImageL};
  if (colorImageR) im.push_back(*colorImageR);
  pano::shareStep(im);
  Mat out(colorImageL.rows, colorImageL.cols, CV_8UC4);
  pano::check(pf_stitch_step(pano::context(), im[0].data, colorImageR ? im[1].data : nullptr, colorImageL.cols, colorImageL.rows,
                             im[0].step, maxPct, out.data, out.step));
  return out;
}

// A stitch plan (pf_stitch_plan): the Map and the blend ramp of one step of a fixed rig, kept in HBM and reused for every frame whose
// alpha masks are the ones it was made from.  colorImageR == nullptr takes the R mask from the previous stitchStep's result in HBM.
// Owned by pano::context(); the object frees it (movable, not copyable).
class StitchPlan {
 public:
  StitchPlan() {}
  StitchPlan(const Mat& colorImageL, const Mat* colorImageR) {
    if (colorImageL.type() != CV_8UC4 || (colorImageR && (colorImageR->type() != CV_8UC4 || colorImageR->rows != colorImageL.rows ||
                                                           colorImageR->cols != colorImageL.cols)))
      throw util::VrCamException("StitchPlan: inputs must be CV_8UC4 images of equal size");
    std::vector<Mat> im = {colorImageL};
    if (colorImageR) im.push_back(*colorImageR);
    pano::shareStep(im);
    pano::check(pf_stitch_plan_create(pano::context(), im[0].data, colorImageR ? im[1].data : nullptr, colorImageL.cols, colorImageL.rows, im[0].step, &plan_));
  }
  ~StitchPlan() { reset(); }
  StitchPlan(const StitchPlan&) = delete;
  StitchPlan& operator=(const StitchPlan&) = delete;
  StitchPlan(StitchPlan&& o) noexcept : plan_(o.plan_) { o.plan_ = nullptr; }
  StitchPlan& operator=(StitchPlan&& o) noexcept {
    if (this != &o) { reset(); plan_ = o.plan_; o.plan_ = nullptr; }
    return *this;
  }
  void reset() {
    if (plan_) pf_stitch_plan_destroy(pano::context(), plan_);
    plan_ = nullptr;
  }
  bool empty() const { return plan_ == nullptr; }
  const pf_stitch_plan* get() const { return plan_; }
  int cols() const { int v = 0; if (plan_) pf_stitch_plan_info(plan_, &v, nullptr, nullptr); return v; }
  int rows() const { int v = 0; if (plan_) pf_stitch_plan_info(plan_, nullptr, &v, nullptr); return v; }
  long long overlapPixels() const { long long v = 0; if (plan_) pf_stitch_plan_info(plan_, nullptr, nullptr, &v); return v; }
  Mat getMap() const {
    Mat m(rows(), cols(), CV_8UC1);
    pano::check(pf_stitch_plan_download(pano::context(), plan_, m.data, m.step, nullptr, 0));
    return m;
  }
  Mat getBlend() const {
    Mat b(rows(), cols(), CV_32FC1);
    pano::check(pf_stitch_plan_download(pano::context(), plan_, nullptr, 0, b.ptr<float>(), b.step));
    return b;
  }

 private:
  pf_stitch_plan* plan_ = nullptr;
};

// A rig plan (pf_rig_plan): the StitchPlans of every step of one rig's chain, made from the top image and the chain's left images before
// any flow is solved (only alphas are read).  Owned by pano::context(); the object frees it (movable, not copyable).  step(i) is step
// i + 1's plan for stitchStep-like calls on the C interface; the rig owns it.
class RigPlan {
 public:
  RigPlan() {}
  RigPlan(const Mat& colorImageT, const std::vector<Mat>& colorImagesL) {
    std::vector<Mat> im = {colorImageT};
    for (const Mat& m : colorImagesL) {
      if (colorImageT.type() != CV_8UC4 || m.type() != CV_8UC4 || m.rows != colorImageT.rows || m.cols != colorImageT.cols)
        throw util::VrCamException("RigPlan: inputs must be CV_8UC4 images of equal size");
      im.push_back(m);
    }
    pano::shareStep(im);
    std::vector<const uint8_t*> l;
    for (size_t i = 1; i < im.size(); ++i) l.push_back(im[i].data);
    pano::check(pf_rig_plan_create(pano::context(), (int)l.size(), im[0].data, l.data(), colorImageT.cols, colorImageT.rows, im[0].step, &rig_));
  }
  ~RigPlan() { reset(); }
  RigPlan(const RigPlan&) = delete;
  RigPlan& operator=(const RigPlan&) = delete;
  RigPlan(RigPlan&& o) noexcept : rig_(o.rig_) { o.rig_ = nullptr; }
  RigPlan& operator=(RigPlan&& o) noexcept {
    if (this != &o) { reset(); rig_ = o.rig_; o.rig_ = nullptr; }
    return *this;
  }
  void reset() {
    if (rig_) pf_rig_plan_destroy(pano::context(), rig_);
    rig_ = nullptr;
  }
  bool empty() const { return rig_ == nullptr; }
  const pf_rig_plan* get() const { return rig_; }
  int steps() const { int v = 0; if (rig_) pf_rig_plan_info(rig_, &v, nullptr, nullptr); return v; }
  int cols() const { int v = 0; if (rig_) pf_rig_plan_info(rig_, nullptr, &v, nullptr); return v; }
  int rows() const { int v = 0; if (rig_) pf_rig_plan_info(rig_, nullptr, nullptr, &v); return v; }
  const pf_stitch_plan* step(int i) const {
    const pf_stitch_plan* p = pf_rig_plan_step(pano::context(), rig_, i);
    if (!p) throw util::VrCamException(std::string("panoflow: ") + pf_last_error(pano::context()));
    return p;
  }
  long long overlapPixels(int i) const { long long v = 0; pf_stitch_plan_info(step(i), nullptr, nullptr, &v); return v; }

 private:
  pf_rig_plan* rig_ = nullptr;
};

// stitchStep on a plan: the same bytes without recomputing the map and the ramp; throws if the frame's masks are not the plan's.
static inline Mat stitchStep(const StitchPlan& plan, const Mat& colorImageL, const Mat* colorImageR, const std::string& flowAlgName) {
  const int maxPct = pf_max_percentage_by_name(flowAlgName.c_str());
  if (maxPct < 0) throw util::VrCamException("unrecognized flow algorithm name: " + flowAlgName);
  if (colorImageL.type() != CV_8UC4 || (colorImageR && (colorImageR->type() != CV_8UC4 || colorImageR->rows != colorImageL.rows ||
                                                         colorImageR->cols != colorImageL.cols)))
    throw util::VrCamException("stitchStep: inputs must be CV_8UC4 images of equal size");
  std::vector<Mat> im = {colorImageL};
  if (colorImageR) im.push_back(*colorImageR);
  pano::shareStep(im);
  Mat out(colorImageL.rows, colorImageL.cols, CV_8UC4);
  pano::check(pf_stitch_step_planned(pano::context(), plan.get(), im[0].data, colorImageR ? im[1].data : nullptr, colorImageL.cols,
                                     colorImageL.rows, im[0].step, maxPct, out.data, out.step));
  return out;
}

}  // namespace stitch_tools

#endif /* StitchTool_hpp */
