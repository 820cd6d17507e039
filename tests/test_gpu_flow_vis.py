"""GPU tier of the flow visualisers (pf_vis_*, pf_stitch_visualize; CPU/OpticalFlow.cpp:147-204, CPU/main.cpp:20-45): every kernel
output byte for byte against the serial host reference tests/cpp/flow_vis_ref.cpp (host libm atan2f, OpenCV-style LineAA drawn one
arrow at a time in the reference's order) -- oracle fixture flows, synthetic edge cases, sizes from 1x1 to 9000x4000."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT
from test_flow_vis import Ref, build_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return Ref(build_ref(tmp_path_factory.mktemp("flow_vis_ref_gpu")))


@pytest.fixture(scope="module")
def ctx(pf):
    c = pf.Context(0)
    yield c
    c.close()


def _image(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 4), dtype=np.uint8)


def _check_all(ctx, ref, flow, image, what=""):
    assert np.array_equal(ctx.vis_grey_disparity(flow), ref.grey(flow)), "grey " + what
    wg, wr = ctx.vis_color_wheel(flow), ref.wheel(flow)
    assert np.array_equal(wg, wr), "wheel %s: %d bytes differ" % (what, int((wg != wr).sum()))
    fg, fr = ctx.vis_vector_field(flow, image), ref.field(flow, image)
    assert np.array_equal(fg, fr), "field %s: %d bytes differ" % (what, int((fg != fr).sum()))
    pg = ctx.vis_panel(flow, image)
    assert np.array_equal(pg, ref.panel(flow, image)), "panel " + what
    return pg


def _synthetic(rows, cols, seed):
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((rows, cols, 2)) * 6).astype(np.float32)   # dense random vectors: neighbouring arrows overlap
    f[::5, ::7] = 0.0                                                  # zero vectors
    f[1::9, :, 1] = 0.0                                                # exact axis directions (hue 0 / pi: +-x)
    f[2::9, :, 0] = 0.0                                                # +-y
    f[3::11, :, 1] = -0.0                                              # atan2(-0, -x) = -pi: the other end of the hue range
    f[4::13] *= 8.0 * max(rows, cols) / 6                              # magnitudes up to 8x the image size
    return f


def test_fixture_flows(ctx, ref):
    d = np.load(os.path.join(ROOT, "tests", "golden", "flow_160x128.npz"))
    for alg in ("low", "s20"):
        _check_all(ctx, ref, d["flowLR_" + alg], d["L"], "flowLR_" + alg)
        _check_all(ctx, ref, d["flowRL_" + alg], d["R"], "flowRL_" + alg)


@pytest.mark.parametrize("rows,cols", [(1, 1), (7, 13), (25, 25), (4000, 24), (97, 131)])
def test_synthetic_sizes(ctx, ref, rows, cols):
    flow = _synthetic(rows, cols, rows * 1000 + cols)
    _check_all(ctx, ref, flow, _image(rows, cols, cols), "%dx%d" % (cols, rows))
    # a constant x component: all-zero disparity
    const = np.full((rows, cols, 2), 2.5, np.float32)
    assert (ctx.vis_grey_disparity(const) == 0).all()
    _check_all(ctx, ref, const, _image(rows, cols, 1), "constant %dx%d" % (cols, rows))


def test_panel_dev_full_size(pf, ctx, ref):
    import torch
    cols, rows = 9000, 4000
    g = torch.Generator(device="cuda").manual_seed(7)
    flow = torch.randn((rows, cols, 2), device="cuda", generator=g) * 6
    flow[::5, ::7] = 0.0
    flow[3::13] *= 2000.0
    img = torch.randint(0, 256, (rows, cols, 4), device="cuda", dtype=torch.uint8, generator=g)
    out = torch.empty((rows, 3 * cols, 4), device="cuda", dtype=torch.uint8)
    torch.cuda.synchronize()
    ctx.vis_panel_dev(flow.data_ptr(), img.data_ptr(), cols, rows, out.data_ptr())
    got = out.cpu().numpy(); f = flow.cpu().numpy(); im = img.cpu().numpy()
    exp = ref.panel(f, im)
    assert np.array_equal(got, exp), "9000x4000 panel: %d bytes differ" % int((got != exp).sum())
    # the host-buffer panel gives the same bytes
    assert np.array_equal(ctx.vis_panel(f, im), exp)


def test_stitch_visualize_chain(pf, synth):
    cols, rows, n = 480, 320, 3
    top, imgs = synth.make_stitch_set(cols, rows, 77, 5)
    top = top.numpy(); imgs = [im.numpy() for im in imgs[:n]]
    c = pf.Context(0)
    try:
        with pytest.raises(pf.PanoflowError):
            c.stitch_visualize((rows, cols))                   # no step has run
        outs, panels, inputs = [], [], []
        R = top
        for i in range(n):
            o = c.stitch_step(imgs[i], R if i == 0 else None, 20)
            panels.append(c.stitch_visualize())
            inputs.append((imgs[i], R))
            outs.append(o); R = o
        # a solve reuses the flow buffers: the step's panels are gone
        c.novel_view(imgs[0], top, 20, np.full((rows, cols), 0.5, np.float32), want_flows=False)
        with pytest.raises(pf.PanoflowError):
            c.stitch_visualize()
        # the chain without the visualiser calls: same composites
        c2 = pf.Context(0)
        R = top
        for i in range(n):
            o = c2.stitch_step(imgs[i], R if i == 0 else None, 20)
            assert np.array_equal(o, outs[i]), "step %d composite changed by pf_stitch_visualize" % i
            R = o
        # each step's panels equal pf_vis_panel of that step's flows (pf_flow_bidir on its overlapped images) over its inputs
        for i, ((L, Rin), (pl, pr)) in enumerate(zip(inputs, panels)):
            _, ovl, ovr = c2.stitch_match(L, Rin)
            f0, f1 = c2.flow_bidir(ovl, ovr, 20)
            assert np.array_equal(pl, c2.vis_panel(f0, L)), "step %d L->R panel" % i
            assert np.array_equal(pr, c2.vis_panel(f1, Rin)), "step %d R->L panel" % i
        c2.close()
    finally:
        c.close()


def test_rejects_bad_input(pf, ctx):
    import ctypes as C
    rows, cols = 30, 40
    img = _image(rows, cols, 3)
    for bad in (np.nan, np.inf, -np.inf):
        f = np.zeros((rows, cols, 2), np.float32); f[17, 5, 1] = bad
        for call in (lambda: ctx.vis_grey_disparity(f), lambda: ctx.vis_color_wheel(f), lambda: ctx.vis_vector_field(f, img),
                     lambda: ctx.vis_panel(f, img)):
            with pytest.raises(pf.PanoflowError):
                call()
    f = np.zeros((rows, cols, 2), np.float32)
    out = np.empty((rows, 3 * cols, 4), np.uint8)
    l = ctx.l
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert l.pf_vis_panel(ctx.h, None, C.c_size_t(cols * 8), p(img), C.c_size_t(cols * 4), cols, rows, p(out), C.c_size_t(cols * 12)) == -1
    assert l.pf_vis_panel(ctx.h, p(f), C.c_size_t(cols * 8), p(img), C.c_size_t(cols * 4), cols, rows, p(out), C.c_size_t(cols * 12 - 1)) == -1
    assert l.pf_vis_grey_disparity(ctx.h, p(f), C.c_size_t(cols * 8 - 4), cols, rows, p(out), C.c_size_t(cols)) == -1
    assert l.pf_vis_color_wheel(ctx.h, p(f), C.c_size_t(cols * 8), cols, rows, p(out), C.c_size_t(cols * 3 - 1)) == -1
    assert l.pf_vis_vector_field(ctx.h, p(f), C.c_size_t(cols * 8), p(img), C.c_size_t(cols * 4 - 1), cols, rows, p(out), C.c_size_t(cols * 4)) == -1
    assert l.pf_vis_panel_dev(ctx.h, None, None, cols, rows, None) == -1
    assert l.pf_stitch_visualize(None, None, None, C.c_size_t(0)) == -1


DROPIN = r'''
#include <cstdio>
#include <vector>
#include "OpticalFlow.hpp"
using namespace panocv; using namespace util; using namespace optical_flow;
int main(int argc, char** argv) {
  const int rows = atoi(argv[1]), cols = atoi(argv[2]);
  Mat flow(rows, cols, CV_32FC2), img(rows, cols, CV_8UC4);
  FILE* f = fopen(argv[3], "rb"); fread(flow.data, 8, size_t(rows) * cols, f); fread(img.data, 4, size_t(rows) * cols, f); fclose(f);
  Mat g = visualizeFlowAsGreyDisparity(flow), w = visualizeFlowColorWheel(flow), v = visualizeFlowAsVectorField(flow, img);
  if (g.type() != CV_8UC1 || w.type() != CV_8UC3 || v.type() != CV_8UC4) return 2;
  try { visualizeFlowAsVectorField(flow, w); return 3; } catch (const VrCamException&) {}
  try { visualizeFlowColorWheel(img); return 4; } catch (const VrCamException&) {}
  Mat gs = stackHorizontal(std::vector<Mat>({g, g})), ws = stackHorizontal(std::vector<Mat>({w, w})), vs = stackHorizontal(std::vector<Mat>({v, v}));
  f = fopen(argv[4], "wb");
  fwrite(g.data, 1, size_t(rows) * cols, f); fwrite(w.data, 3, size_t(rows) * cols, f); fwrite(v.data, 4, size_t(rows) * cols, f);
  fwrite(gs.data, 2, size_t(rows) * cols, f); fwrite(ws.data, 6, size_t(rows) * cols, f); fwrite(vs.data, 8, size_t(rows) * cols, f);
  fclose(f);
  return 0;
}
'''


def test_cpp_dropin(pf, ctx, tmp_path):
    src = tmp_path / "vis_dropin.cpp"; src.write_text(DROPIN)
    exe = str(tmp_path / "vis_dropin")
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(PKG, "include"), "-o", exe, str(src), "-L", PKG, "-lpanoflow",
                    "-Wl,-rpath," + PKG], check=True)
    rows, cols = 61, 83
    flow = (np.random.default_rng(5).standard_normal((rows, cols, 2)) * 4).astype(np.float32); img = _image(rows, cols, 9)
    (tmp_path / "in.bin").write_bytes(flow.tobytes() + img.tobytes())
    r = subprocess.run([exe, str(rows), str(cols), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    b = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.uint8)
    n = rows * cols
    g, w, v = b[:n].reshape(rows, cols), b[n:4 * n].reshape(rows, cols, 3), b[4 * n:8 * n].reshape(rows, cols, 4)
    o = 8 * n
    gs, ws, vs = b[o:o + 2 * n].reshape(rows, 2 * cols), b[o + 2 * n:o + 8 * n].reshape(rows, 2 * cols, 3), b[o + 8 * n:].reshape(rows, 2 * cols, 4)
    assert np.array_equal(g, ctx.vis_grey_disparity(flow)) and np.array_equal(w, ctx.vis_color_wheel(flow))
    assert np.array_equal(v, ctx.vis_vector_field(flow, img))
    assert np.array_equal(gs, np.concatenate([g, g], 1)) and np.array_equal(ws, np.concatenate([w, w], 1)) and np.array_equal(vs, np.concatenate([v, v], 1))


@pytest.mark.parametrize("fused", ["1", "0"])
def test_cli_visualize(pf, synth, tmp_path, fused):
    from PIL import Image
    exe = os.path.join(PKG, "tools", "pano_stitch")
    cols, rows, n = 480, 320, 2
    top, imgs = synth.make_stitch_set(cols, rows, 77, 5)
    top = top.numpy(); imgs = [im.numpy() for im in imgs[:n]]
    rgba = lambda a: np.ascontiguousarray(a[..., [2, 1, 0, 3]])
    Image.fromarray(rgba(top), "RGBA").save(tmp_path / "top.tif")
    for i, im in enumerate(imgs):
        Image.fromarray(rgba(im), "RGBA").save(tmp_path / ("%d.tif" % (i + 1)))
    base = [exe, "-test_dir", str(tmp_path), "-top_img", "top.tif", "--flow_alg=pixflow_search_20", "-steps", str(n), "-fused", fused]
    r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert not (tmp_path / "disparity").exists()
    r = subprocess.run(base + ["-visualize", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    c = pf.Context(0)
    try:
        R = top
        for i in range(n):
            _, ovl, ovr = c.stitch_match(imgs[i], R)
            f0, f1 = c.flow_bidir(ovl, ovr, 20)
            for name, f, im in (("LtoR", f0, imgs[i]), ("RtoL", f1, R)):
                got = np.array(Image.open(tmp_path / "disparity" / ("%s_pixflow_search_20_step%d.png" % (name, i + 1))))[..., [2, 1, 0, 3]]
                assert np.array_equal(got, c.vis_panel(f, im)), "%s step %d (fused %s)" % (name, i + 1, fused)
            R = c.stitch_step(imgs[i], R if i == 0 else None, 20)
    finally:
        c.close()
