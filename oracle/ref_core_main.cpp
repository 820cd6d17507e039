// =============================================================================================
// oracle/ref_core_main.cpp  --  TEST INFRASTRUCTURE ONLY.
//
// Command-line driver around the REFERENCE's own translation units (OpticalFlow.cpp, StitchTool.cpp and the headers they
// include), compiled unmodified against the OpenCV stand-in under oracle/cvstub and linked with the oracle for the primitive
// bodies (oracle/Makefile, target refcore).  PixFlow is a struct with public methods, so single steps are reachable as well as
// whole runs.  Reads and writes flat binary arrays (row-major, interleaved channels, native endianness).
//
//   pano_ref_core CMD PCT pyrScale smoothness vReg hReg stepSize  ARGS...
//     PCT is the PixFlow<MaxPercentage> instantiation (0 or 20); the five coefficients are its constructor arguments
//     (downscaleFactor 0.5, directionalRegularizationCoef 0).  `prepare` goes through the reference's factory, i.e. presets.
//   CMD ARGS:
//     pyramid        H WLO WHI  out.i32            buildPyramid sizes for every width WLO..WHI: n, then n (w, h) pairs
//     errfn          W H K  I0x I0y I1x I1y blurred cand  out     errorFunction at every pixel for K candidate planes
//     patcherr       W H N  I0 a0 I1 a1 pts.i32  out              computePatchError at N (i0x, i0y, i1x, i1y)
//     adjust         W H HINT  I0 I1 a0 a1  out                   adjustInitialFlow on a zero flow
//     level          W H HINT HASFLOW  I0 I1 a0 a1 [flow]  out    patchMatchPropagationAndSearch
//     diffusion      W H  a0 a1 flow  out                         lowAlphaFlowDiffusion
//     cof            COLS ROWS HINT  bgra0 bgra1  out             computeOpticalFlow
//     prepare        COLS ROWS  L R  outLtoR outRtoL              NovelViewGeneratorAsymmetricFlow::prepare
//     combine        COLS ROWS  L R fLtoR fRtoL blend  out        NovelViewUtil::combineNovelViews
//     stitch_prepare COLS ROWS  L R  map ovL ovR blend mergedDis  Stitchtools::prepare
//     gather         COLS ROWS  L R merged map  out               Stitchtools::Gather
// =============================================================================================
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "OpticalFlow.hpp"
#include "StitchTool.hpp"

using cv::Mat;
using optical_flow::OpticalFlowInterface;
using optical_flow::PixFlow;

namespace {

[[noreturn]] void die(const std::string& m) {
  std::fprintf(stderr, "pano_ref_core: %s\n", m.c_str());
  std::exit(2);
}

Mat load(const char* path, int rows, int cols, int type) {
  Mat m(rows, cols, type);
  FILE* f = std::fopen(path, "rb");
  if (!f) die(std::string("cannot open ") + path);
  const size_t n = (size_t)rows * m.step;
  const size_t got = std::fread(m.data, 1, n, f);
  const bool more = std::fgetc(f) != EOF;
  std::fclose(f);
  if (got != n || more) die(std::string("wrong size: ") + path);
  return m;
}

void store(const char* path, const Mat& m, int rows, int cols, int type) {
  if (m.rows != rows || m.cols != cols || m.type() != type) die(std::string("unexpected result shape or type for ") + path);
  FILE* f = std::fopen(path, "wb");
  if (!f) die(std::string("cannot create ") + path);
  const size_t n = (size_t)cols * m.elemSize();
  for (int y = 0; y < rows; ++y)
    if (std::fwrite(m.data + (size_t)y * m.step, 1, n, f) != n) die(std::string("short write: ") + path);
  std::fclose(f);
}

template <int P>
int run(const std::string& cmd, const float* k, int n, char** a) {
  auto need = [&](int want) { if (n != want) die(cmd + ": wrong number of arguments"); };
  auto I = [&](int i) { return std::atoi(a[i]); };
  PixFlow<P> pf(k[0], k[1], k[2], k[3], k[4], 0.5f, 0.0f);
  typedef OpticalFlowInterface::DirectionHint Hint;

  if (cmd == "pyramid") {
    need(4);
    const int h = I(0), wlo = I(1), whi = I(2);
    cv::cvstub_resize_sizes_only() = true;
    std::vector<int> out;
    for (int w = wlo; w <= whi; ++w) {
      std::vector<Mat> pyr = pf.buildPyramid(Mat(h, w, CV_32F));
      out.push_back((int)pyr.size());
      for (const Mat& m : pyr) { out.push_back(m.cols); out.push_back(m.rows); }
    }
    FILE* f = std::fopen(a[3], "wb");
    if (!f || std::fwrite(out.data(), 4, out.size(), f) != out.size()) die("pyramid: cannot write");
    std::fclose(f);
    return 0;
  }
  if (cmd == "errfn") {
    need(10);
    const int w = I(0), h = I(1), K = I(2);
    Mat I0x = load(a[3], h, w, CV_32FC1), I0y = load(a[4], h, w, CV_32FC1), I1x = load(a[5], h, w, CV_32FC1), I1y = load(a[6], h, w, CV_32FC1);
    Mat blurred = load(a[7], h, w, CV_32FC2), cand = load(a[8], K * h, w, CV_32FC2);
    Mat plane(h, w, CV_32FC1), flow(h, w, CV_32FC2), err(K * h, w, CV_32FC1);
    for (int c = 0; c < K; ++c)
      for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
          err.at<float>(c * h + y, x) = pf.errorFunction(plane, plane, plane, plane, I0x, I0y, I1x, I1y, x, y, flow, blurred, cand.at<cv::Point2f>(c * h + y, x));
    store(a[9], err, K * h, w, CV_32FC1);
    return 0;
  }
  if (cmd == "patcherr") {
    need(9);
    const int w = I(0), h = I(1), N = I(2);
    Mat i0 = load(a[3], h, w, CV_32FC1), a0 = load(a[4], h, w, CV_32FC1), i1 = load(a[5], h, w, CV_32FC1), a1 = load(a[6], h, w, CV_32FC1);
    Mat pts = load(a[7], N, 16, CV_8UC1), out(N, 1, CV_32FC1);
    for (int i = 0; i < N; ++i) {
      const int* p = pts.ptr<int>(i);
      out.at<float>(i, 0) = pf.computePatchError(i0, a0, p[0], p[1], i1, a1, p[2], p[3]);
    }
    store(a[8], out, N, 1, CV_32FC1);
    return 0;
  }
  if (cmd == "adjust") {
    need(8);
    const int w = I(0), h = I(1);
    Mat i0 = load(a[3], h, w, CV_32FC1), i1 = load(a[4], h, w, CV_32FC1), a0 = load(a[5], h, w, CV_32FC1), a1 = load(a[6], h, w, CV_32FC1);
    Mat flow = Mat::zeros(i0.size(), CV_32FC2);
    pf.adjustInitialFlow(i0, i1, a0, a1, flow, Hint(I(2)));
    store(a[7], flow, h, w, CV_32FC2);
    return 0;
  }
  if (cmd == "level") {
    const int w = I(0), h = I(1), has = I(3);
    need(has ? 10 : 9);
    Mat i0 = load(a[4], h, w, CV_32FC1), i1 = load(a[5], h, w, CV_32FC1), a0 = load(a[6], h, w, CV_32FC1), a1 = load(a[7], h, w, CV_32FC1);
    Mat flow;
    if (has) flow = load(a[8], h, w, CV_32FC2);
    pf.patchMatchPropagationAndSearch(i0, i1, a0, a1, flow, Hint(I(2)));
    store(a[has ? 9 : 8], flow, h, w, CV_32FC2);
    return 0;
  }
  if (cmd == "diffusion") {
    need(6);
    const int w = I(0), h = I(1);
    Mat a0 = load(a[2], h, w, CV_32FC1), a1 = load(a[3], h, w, CV_32FC1), flow = load(a[4], h, w, CV_32FC2);
    pf.lowAlphaFlowDiffusion(a0, a1, flow);
    store(a[5], flow, h, w, CV_32FC2);
    return 0;
  }
  if (cmd == "cof") {
    need(6);
    const int cols = I(0), rows = I(1);
    Mat b0 = load(a[3], rows, cols, CV_8UC4), b1 = load(a[4], rows, cols, CV_8UC4), flow;
    pf.computeOpticalFlow(b0, b1, flow, Hint(I(2)));
    store(a[5], flow, rows, cols, CV_32FC2);
    return 0;
  }
  if (cmd == "prepare") {
    need(6);
    const int cols = I(0), rows = I(1);
    Mat L = load(a[2], rows, cols, CV_8UC4), R = load(a[3], rows, cols, CV_8UC4);
    optical_flow::NovelViewGeneratorAsymmetricFlow g(P == 0 ? "pixflow_low" : "pixflow_search_20");
    g.prepare(L, R);
    store(a[4], g.getFlowLtoR(), rows, cols, CV_32FC2);
    store(a[5], g.getFlowRtoL(), rows, cols, CV_32FC2);
    return 0;
  }
  if (cmd == "combine") {
    need(8);
    const int cols = I(0), rows = I(1);
    Mat L = load(a[2], rows, cols, CV_8UC4), R = load(a[3], rows, cols, CV_8UC4), fLR = load(a[4], rows, cols, CV_32FC2),
        fRL = load(a[5], rows, cols, CV_32FC2), blend = load(a[6], rows, cols, CV_32FC1);
    store(a[7], optical_flow::NovelViewUtil::combineNovelViews(L, R, fLR, fRL, blend), rows, cols, CV_8UC4);
    return 0;
  }
  if (cmd == "stitch_prepare") {
    need(9);
    const int cols = I(0), rows = I(1);
    Mat L = load(a[2], rows, cols, CV_8UC4), R = load(a[3], rows, cols, CV_8UC4);
    stitch_tools::Stitchtools st;
    st.prepare(L, R);
    store(a[4], st.getMap(), rows, cols, CV_8UC1);
    store(a[5], st.getOverlappedL(), rows, cols, CV_8UC4);
    store(a[6], st.getOverlappedR(), rows, cols, CV_8UC4);
    store(a[7], st.getBlend(), rows, cols, CV_32FC1);
    store(a[8], st.MergedDis, rows, cols, CV_32FC1);
    return 0;
  }
  if (cmd == "gather") {
    need(7);
    const int cols = I(0), rows = I(1);
    stitch_tools::Stitchtools st;
    st.ImageL = load(a[2], rows, cols, CV_8UC4);
    st.ImageR = load(a[3], rows, cols, CV_8UC4);
    st.setMergedmiddle(load(a[4], rows, cols, CV_8UC4));
    st.Map = load(a[5], rows, cols, CV_8UC1);
    st.Gather();
    store(a[6], st.getFinalResult(), rows, cols, CV_8UC4);
    return 0;
  }
  die("unknown command " + cmd);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 8) die("usage: pano_ref_core CMD PCT pyrScale smoothness vReg hReg stepSize ARGS...  (see the head of ref_core_main.cpp)");
  const std::string cmd = argv[1];
  const int pct = std::atoi(argv[2]);
  float k[5];
  for (int i = 0; i < 5; ++i) k[i] = std::strtof(argv[3 + i], nullptr);
  if (pct == 0) return run<0>(cmd, k, argc - 8, argv + 8);
  if (pct == 20) return run<20>(cmd, k, argc - 8, argv + 8);
  die("PCT must be 0 or 20 (the instantiations the reference's factory makes)");
}
