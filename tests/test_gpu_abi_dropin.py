"""The C++ drop-in headers on wrapped memory: one program (built here with g++ against include/ and libpanoflow) runs the classes'
calls on Mats that wrap padded caller buffers, Mat(rows, cols, type, ext, ext_step).  Its outputs must equal those of the same program
on packed Mats, and the wrapped buffers (poisoned padding included) must come back unchanged.  Mode 2 mixes one padded with one packed
Mat where two images share a step argument of the C call: the headers copy the odd one out instead of throwing."""
import os
import subprocess

import numpy as np
import pytest

from abi_cases import ndiff
from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

PROGRAM = r'''
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "OpticalFlow.hpp"
#include "StitchTool.hpp"
using namespace panocv; using namespace util; using namespace optical_flow; using namespace stitch_tools;

// a Mat over a caller's buffer whose rows are `pad` bytes further apart than they are wide; the padding holds opaque pixels / large floats
struct Wrapped { std::vector<unsigned char> buf, copy; Mat m; };
static Wrapped wrap(const unsigned char* src, int rows, int cols, int type, size_t pad) {
  Wrapped w;
  const size_t row = size_t(cols) * Mat::elemSizeOf(type), step = row + pad;
  w.buf.resize(step * rows);
  for (int y = 0; y < rows; ++y) {
    unsigned char* d = w.buf.data() + size_t(y) * step;
    memcpy(d, src + size_t(y) * row, row);
    for (size_t i = 0; i < pad; i += 4) {
      if (type == CV_8UC4) { d[row + i] = (unsigned char)(37 * y + i); d[row + i + 1] = (unsigned char)(11 * y + 3 * i); d[row + i + 2] = (unsigned char)(y ^ i); d[row + i + 3] = 255; }
      else { const float v = (y & 1 ? -1.f : 1.f) * (100.f + float(i + y)); memcpy(d + row + i, &v, 4); }
    }
  }
  w.copy = w.buf;
  w.m = Mat(rows, cols, type, w.buf.data(), step);
  return w;
}
static FILE* out;
static void put(const Mat& m) { for (int y = 0; y < m.rows; ++y) fwrite(m.data + size_t(y) * m.step, m.elemSize(), m.cols, out); }

int main(int argc, char** argv) {
  const int rows = atoi(argv[1]), cols = atoi(argv[2]), mode = atoi(argv[5]);
  const size_t n = size_t(rows) * cols;
  std::vector<unsigned char> in(n * (4 * 3 + 4 + 8 * 2));
  FILE* f = fopen(argv[3], "rb");
  if (!f || fread(in.data(), 1, in.size(), f) != in.size()) return 2;
  fclose(f);
  const unsigned char *pL = in.data(), *pR = pL + n * 4, *pM = pR + n * 4, *pB = pM + n * 4, *pF0 = pB + n * 4, *pF1 = pF0 + n * 8;
  // mode 0: every Mat packed.  1: every Mat padded, the planes that share a step argument alike.  2: of each such pair one padded, one packed.
  const size_t a = mode ? 48 : 0, b = mode == 1 ? 48 : 0, fa = mode ? 40 : 0, fb = mode == 1 ? 40 : 0, bl = mode ? 24 : 0;
  Wrapped L = wrap(pL, rows, cols, CV_8UC4, a), R = wrap(pR, rows, cols, CV_8UC4, b), M = wrap(pM, rows, cols, CV_8UC4, mode ? 16 : 0),
          B = wrap(pB, rows, cols, CV_32FC1, bl), F0 = wrap(pF0, rows, cols, CV_32FC2, fa), F1 = wrap(pF1, rows, cols, CV_32FC2, fb);
  if (mode && (L.m.step == size_t(cols) * 4 || B.m.step == size_t(cols) * 4 || F0.m.step == size_t(cols) * 8)) return 3;
  out = fopen(argv[4], "wb");
  try {
    const std::string alg = "pixflow_search_20";
    Mat flow;
    std::unique_ptr<OpticalFlowInterface> of(makeOpticalFlowByName(alg));
    of->computeOpticalFlow(L.m, R.m, flow, OpticalFlowInterface::DirectionHint::LEFT);
    put(flow);
    NovelViewGeneratorAsymmetricFlow nv(alg);
    nv.prepare(L.m, R.m);
    nv.setBlend(B.m);
    Mat view;
    nv.generateNovelView(view);
    put(nv.getFlowLtoR()); put(nv.getFlowRtoL()); put(view);
    put(NovelViewUtil::combineNovelViews(L.m, R.m, F0.m, F1.m, B.m));
    Stitchtools st;
    st.prepare(L.m, R.m);
    put(st.getMap()); put(st.getOverlappedL()); put(st.getOverlappedR()); put(st.getBlend()); put(st.MergedDis);
    st.MatchImages();
    put(st.getMap());
    st.GenerateBlend();
    put(st.getBlend());
    st.setMergedmiddle(M.m);
    st.Gather();
    put(st.getFinalResult());
    put(stitchStep(L.m, &R.m, alg));
    StitchPlan plan(L.m, &R.m);
    put(plan.getMap()); put(plan.getBlend());
    put(stitchStep(plan, L.m, &R.m, alg));
    put(visualizeFlowAsGreyDisparity(F0.m)); put(visualizeFlowColorWheel(F0.m)); put(visualizeFlowAsVectorField(F0.m, L.m));
  } catch (const VrCamException& e) { fprintf(stderr, "%s\n", e.what()); return 4; }
  fclose(out);
  for (const Wrapped* w : {&L, &R, &M, &B, &F0, &F1}) if (w->buf != w->copy) return 5;   // a wrapped buffer, its padding included, was written
  return 0;
}
'''


def _same(got, want, what):
    assert np.array_equal(got, want), "%s: %d elements differ" % (what, ndiff(got, want))


def test_dropin_headers_on_wrapped_padded_mats(orc, tmp_path):
    src = tmp_path / "wrapped.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "wrapped")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(PKG, "include"), "-o", exe, str(src), "-L", PKG, "-lpanoflow", "-Wl,-rpath," + PKG], check=True)
    g = np.load(os.path.join(ROOT, "tests", "golden", "stitch_240x200.npz"))
    L, R, merged, blend = g["L"], g["R"], g["merged"], g["blend"]
    rows, cols = blend.shape
    r = np.random.default_rng(11)
    f0 = (r.standard_normal((rows, cols, 2)) * 4).astype(np.float32); f1 = (r.standard_normal((rows, cols, 2)) * 4).astype(np.float32)
    (tmp_path / "in.bin").write_bytes(b"".join(np.ascontiguousarray(a).tobytes() for a in (L, R, merged, blend, f0, f1)))
    outs = []
    for mode in (0, 1, 2):
        o = tmp_path / ("out%d.bin" % mode)
        p = subprocess.run([exe, str(rows), str(cols), str(tmp_path / "in.bin"), str(o), str(mode)], capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, "mode %d: exit %d (5 = a wrapped buffer was written): %s" % (mode, p.returncode, p.stderr)
        outs.append(np.frombuffer(o.read_bytes(), np.uint8))
    n = rows * cols
    names = [("flow", 8), ("nv flow L->R", 8), ("nv flow R->L", 8), ("novel view", 4), ("combineNovelViews", 4), ("Map", 1), ("OverlappedL", 4), ("OverlappedR", 4),
             ("Blend", 4), ("MergedDis", 4), ("Map after MatchImages", 1), ("Blend after GenerateBlend", 4), ("FinalResult", 4), ("stitchStep", 4), ("plan map", 1),
             ("plan blend", 4), ("planned stitchStep", 4), ("grey disparity", 1), ("colour wheel", 3), ("vector field", 4)]
    assert outs[0].size == n * sum(b for _, b in names)
    parts, at = {}, 0
    for name, b in names:
        for mode in (1, 2):
            _same(outs[mode][at:at + n * b], outs[0][at:at + n * b], "%s, mode %d vs packed Mats" % (name, mode))
        parts[name] = outs[0][at:at + n * b]
        at += n * b
    # the packed run is the oracle's: not three equal wrong answers
    mp, ovl, ovr, bl, md = orc.stitch_prepare(L, R, True)
    _same(parts["Map"].reshape(rows, cols), mp, "Map vs the oracle")
    _same(parts["Blend"].view(np.float32).reshape(rows, cols), bl, "Blend vs the oracle")
    _same(parts["FinalResult"].reshape(rows, cols, 4), g["final"], "FinalResult vs the oracle")
    _same(parts["combineNovelViews"].reshape(rows, cols, 4), orc.combine_novel_views(L, R, f0, f1, blend), "combineNovelViews vs the oracle")
    _same(parts["flow"].view(np.float32).reshape(rows, cols, 2), orc.compute_optical_flow(L, R, 20, 3), "computeOpticalFlow vs the oracle")
    w0, w1 = orc.flow_bidir(ovl, ovr, 20)
    _same(parts["stitchStep"].reshape(rows, cols, 4), orc.stitch_gather(L, R, orc.combine_novel_views(ovl, ovr, w0, w1, bl), mp), "stitchStep vs the oracle")
    _same(parts["planned stitchStep"], parts["stitchStep"], "planned stitchStep vs stitchStep")
