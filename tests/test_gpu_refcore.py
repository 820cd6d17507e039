"""The HIP path against fixtures produced by THE REFERENCE'S OWN TEXT (tests/golden/refcore_*.npz, made by tests/golden/make_refcore_golden.py
from oracle/_ref/pano_ref_core: the reference's translation units compiled unmodified against the OpenCV stand-in).  No oracle call and no
oracle/_ref here: only the committed files.  Bit for bit (flows) and byte for byte (images), in the product library's two sweep forms.

Scope, as for every parity test of the blend: the fixtures' exp / tanhf are the libm's of the machine that made them.  The shapes are small
ones that still include a portrait level (45 x 61), a coarsest level with the patch search (150 x 131), the wrap pad with a truncated cols/20
and odd half sizes (203 x 131) and the tile blur with an even kernel (400 x 800)."""
import hashlib
import os

import numpy as np
import pytest

import refcore_cases as rc
from conftest import ROOT

pytestmark = pytest.mark.gpu

G = os.path.join(ROOT, "tests", "golden")


def load(name):
    return np.load(os.path.join(G, name))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    a = got.view(np.uint32) if got.dtype == np.float32 else got
    b = want.view(np.uint32) if want.dtype == np.float32 else want
    n = int((a != b).sum())
    assert n == 0, "%s: %d of %d elements differ from the reference's fixture" % (what, n, a.size)


@pytest.fixture(scope="module", params=[0, 2], ids=["latency_form", "throughput_form"])
def ctx(request, pf):
    c = pf.Context(0, sweep_wide=request.param)
    yield c
    c.close()


@pytest.mark.parametrize("hint", [1, 2, 3, 4])
def test_adjust_initial_flow(ctx, hint):
    g = load("refcore_adjust_29x26.npz")
    got = ctx.stage_adjust_initial_flow(rc.img_f32(g["I0"]), rc.img_f32(g["I1"]), rc.img_f32(g["a0"]), rc.img_f32(g["a1"]), hint, 20)
    same(got, g["flow_h%d" % hint], "adjustInitialFlow, hint %d" % hint)
    assert got.any()


@pytest.mark.parametrize("w,h", [(61, 45), (45, 61)])
def test_level_with_an_incoming_flow(ctx, w, h):
    g = load("refcore_level_%dx%d.npz" % (w, h))
    I0, I1, a0, a1, fin = rc.decode_level(g)
    assert I0.shape == (h, w)
    got = ctx.stage_level(I0, I1, a0, a1, fin, 0, 0)
    same(got, g["flow"], "level %dx%d" % (w, h))
    assert not np.array_equal(got, fin)


def test_level_with_tied_proposals(ctx):
    """Different proposals of exactly equal error (tests/refcore_cases.py::tie_case_q, smoothnessCoef 0): the one input on which the order of
    a sweep's two proposals and the strict '<' of proposeFlowUpdate decide the bits."""
    g = load("refcore_level_ties_61x45.npz")
    I0, I1, a0, a1, fin = rc.decode_level(g)
    keys = ("pyr_scale_factor", "smoothness_coef", "vertical_regularization_coef", "horizontal_regularization_coef", "gradient_step_size")
    ctx.set_solver_params(**dict(zip(keys, (float(v) for v in g["params"]))))
    try:
        got = ctx.stage_level(I0, I1, a0, a1, fin, 0, 0)
    finally:
        ctx.set_solver_params()
    same(got, g["flow"], "level with tied proposals")
    assert not np.array_equal(got, fin)


def test_coarsest_level_with_search(ctx):
    g = load("refcore_level_150x131_coarsest.npz")
    got = ctx.stage_level(rc.img_f32(g["I0"]), rc.img_f32(g["I1"]), rc.img_f32(g["a0"]), rc.img_f32(g["a1"]), None, 3, 20)
    same(got, g["flow"], "coarsest level 150x131, hint LEFT, 20 %")
    assert got.any()


@pytest.mark.parametrize("name,pct", [("low", 0), ("s20", 20)])
@pytest.mark.parametrize("cols,rows", [(160, 128), (203, 131)])
def test_flows_and_novel_view(ctx, synth, cols, rows, name, pct):
    g = load("refcore_pair_%dx%d_%s.npz" % (cols, rows, name))
    L, R, blend = synth.make_pair_np(cols, rows, int(g["seed"]))
    assert np.array_equal(sha(L, R, blend), g["in_sha"]), "the synthetic inputs are not the ones the fixture was made from"
    f0, f1 = ctx.flow_bidir(L, R, pct)
    same(f0, g["flowLR"], "flowLtoR"); same(f1, g["flowRL"], "flowRtoL")
    out, n0, n1 = ctx.novel_view(L, R, pct, blend)
    same(n0, g["flowLR"], "novel_view flowLtoR"); same(n1, g["flowRL"], "novel_view flowRtoL")
    same(out, g["merged"], "novel view")
    assert f0.any() and not np.array_equal(out, L)


def test_one_stitch_step(ctx, synth):
    g = load("refcore_stitch_400x800.npz")
    L, R, _ = rc.canvas(synth, "tall_even")
    assert np.array_equal(sha(L, R), g["in_sha"]), "the synthetic canvas is not the one the fixture was made from"
    y0, x0 = 300, 168       # make_refcore_golden.CROP
    out = ctx.stitch_step(L, R, 20)
    assert np.array_equal(sha(out), g["final_sha"]), "composite differs; bytes differing inside the crop: %d" % int((out[y0:y0 + 64, x0:x0 + 64] != g["final_crop"]).sum())
    same(out[y0:y0 + 64, x0:x0 + 64], g["final_crop"], "composite crop")
    mp, ovl, ovr, bl, md = ctx.stitch_prepare(L, R)
    same(mp, g["map"], "Map"); same(bl, g["blend"], "blend ramp")
    plan = ctx.stitch_plan(L, R)
    pm, pb = plan.download()
    same(pm, g["map"], "planned Map"); same(pb, g["blend"], "planned blend ramp")
    again = ctx.stitch_step(L, R, 20, plan=plan)
    assert np.array_equal(sha(again), g["final_sha"]), "planned composite differs"
    plan.close()
    assert not np.array_equal(out, L) and ((g["blend"] > 0) & (g["blend"] < 1)).any()
