"""The oracle against the REFERENCE'S OWN TEXT.

oracle/_ref/pano_ref_core is the reference's PixFlow.hpp, OpticalFlow.hpp/.cpp, StitchTool.hpp/.cpp and util.hpp, compiled unmodified
against the OpenCV stand-in under oracle/cvstub (make -C oracle refcore), with the primitive bodies (resize, Gaussian, Sobel, median, box
blur) delegated to the oracle.  Both sides therefore run the same primitive arithmetic under the same compiler flags and the same libm, and
every comparison here is bit for bit: what is held is every line the reference's authors wrote -- sizing, tie order, NaN losers, proposal
order, clamps, truncations, decision tables.  The arithmetic inside the OpenCV primitives stays unpinned.

Inputs stay outside the four regimes where the reference reads out of bounds or does not terminate and the oracle deliberately defines a
result (|flow * t| >= cols, step < 1, a zero blur width, Gather probes that leave the canvas); the host-AddressSanitizer run below shows it."""
import os
import subprocess

import numpy as np
import pytest

import refcore
import refcore_cases as rc
from conftest import ROOT

G = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def ref():
    if not refcore.available():
        if refcore.sources_present():
            pytest.fail("oracle/_ref/pano_ref_core is missing although the reference's sources are here: run `%s`" % refcore.BUILD_CMD)
        pytest.skip("neither oracle/_ref/pano_ref_core nor the reference's sources are on this machine")
    refcore.use_exe(None)
    refcore.reset_params()
    yield refcore
    refcore.reset_params()


@pytest.fixture()
def both(ref, orc):
    """(reference driver, oracle), with a setter that gives both the same PixFlow constructor arguments."""
    def set_params(p):
        if p is None:
            ref.reset_params(); orc.reset_params()
        else:
            ref.set_params(*p); orc.set_params(*p)
    yield ref, orc, set_params
    ref.reset_params(); orc.reset_params()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    n = int((bits(a) != bits(b)).sum())
    assert n == 0, "%s: %d of %d elements differ bitwise" % (what, n, a.size)


# ---------------------------------------------------------------------------------------------------------------------------------
# pyramid sizing (float arithmetic of PixFlow.hpp:140-145)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [0.9, 0.5, 0.75, 0.95])
def test_pyramid_size_lists(both, scale):
    ref, orc, set_params = both
    set_params((scale, 0.001, 0.01, 0.01, 0.5))
    levels = 0
    for h in (30, 101, 256):
        got = ref.pyramid_sizes_range(h, 25, 2000)
        for w, sizes in zip(range(25, 2001), got):
            assert sizes == orc.pyramid_sizes(w, h), (scale, w, h)
            levels = max(levels, len(sizes))
    assert levels > 1      # the lists are not just their input


# ---------------------------------------------------------------------------------------------------------------------------------
# errorFunction
# ---------------------------------------------------------------------------------------------------------------------------------
def _errfn_planes(orc, w, h):
    r = np.random.default_rng(100 + w)
    g0 = np.stack(orc.gradients(r.random((h, w)).astype(np.float32)), -1)
    g1 = np.stack(orc.gradients(r.random((h, w)).astype(np.float32)), -1)
    blurred = (r.standard_normal((h, w, 2)) * 1.5).astype(np.float32)
    x = np.arange(w, dtype=np.float32)[None, :]; y = np.arange(h, dtype=np.float32)[:, None]
    c = np.zeros((10, h, w, 2), np.float32)
    c[0:3] = (r.standard_normal((3, h, w, 2)) * 1.5)                     # lands inside the image
    c[3, ..., 0] = (w - 2) - x; c[3, ..., 1] = (h - 2) - y               # lands exactly on the w-2 / h-2 clamp
    c[3, ::2, :, 0] += 0.5; c[3, :, ::3, 1] -= 0.25                      # ... and just beside it
    far = np.float32(1000.0)
    c[4, :h // 2, :, 0] = -far; c[4, h // 2:, :, 0] = far                # far outside: left / right
    c[4, :, :w // 2, 1] = -far; c[4, :, w // 2:, 1] = far                #              above / below
    c[5] = (r.standard_normal((h, w, 2)) * 1.5)                          # the operands test_sweep_operands_outside_fast_math_range plants
    c[5, 3::11, 2::7, 1] = np.float32(1e-33)
    c[5, 5::13, 1::9, 0] = np.float32(-3e-39)                            # denormal
    c[5, 7::17, 4::10, :] = np.float32(1e31)
    c[5, 1::6, 5::12, :] = 0.0
    blurred[2::9, 3::8, :] = c[5, 2::9, 3::8, :] + np.float32(1e-20)
    g0[1::6, 5::12, :] = g1[1::6, 5::12, :] + np.float32(1e-25)
    c[6:10] = r.uniform(-w, 2 * w, (4, h, w, 2))                          # anywhere, inside and out
    return g0, g1, blurred, c


@pytest.mark.parametrize("pset", [None, rc.SET_POW2, rc.SET_ODD], ids=["preset", "step_pow2", "step_odd"])
@pytest.mark.parametrize("w,h", [(40, 27), (27, 40)])
def test_error_function(both, w, h, pset):
    ref, orc, set_params = both
    g0, g1, blurred, c = _errfn_planes(orc, w, h)
    assert c.shape[0] * w * h >= 10000
    set_params(pset)
    got = ref.error_function(g0[..., 0], g0[..., 1], g1[..., 0], g1[..., 1], blurred, c)
    want = np.stack([orc.error_function(g0[..., 0], g0[..., 1], g1[..., 0], g1[..., 1], blurred, c[k]) for k in range(c.shape[0])])
    same(got, want, "errorFunction")
    assert not np.array_equal(got, c[..., 0]) and np.isfinite(got[:5]).all()


def test_compute_patch_error(ref, orc):
    w, h = 29, 26
    q = rc.adjust_case_q(w, h, 3)
    I0, I1, a0, a1 = rc.img_f32(q["I0"]), rc.img_f32(q["I1"]), rc.img_f32(q["a0"]), rc.img_f32(q["a1"])
    r = np.random.default_rng(4)
    pts = np.stack([r.integers(0, w, 4000), r.integers(0, h, 4000), r.integers(-3, w + 3, 4000), r.integers(-3, h + 3, 4000)], -1).astype(np.int32)
    got = ref.patch_error(I0, a0, I1, a1, pts, 20)
    same(got, orc.patch_error(I0, a0, I1, a1, pts, 20), "computePatchError")
    assert np.isnan(got).any() or np.isinf(got).any()      # sum(alpha) = 0 occurs
    assert np.isfinite(got).any() and (got[np.isfinite(got)] > 0).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# adjustInitialFlow
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hint", [1, 2, 3, 4])
@pytest.mark.parametrize("w,h", [(26, 29), (29, 26), (40, 27)])
def test_adjust_initial_flow(ref, orc, w, h, hint):
    q = rc.adjust_case_q(w, h, 7 * w + h)
    I0, I1, a0, a1 = rc.img_f32(q["I0"]), rc.img_f32(q["I1"]), rc.img_f32(q["a0"]), rc.img_f32(q["a1"])
    got = ref.adjust_initial_flow(I0, I1, a0, a1, hint, 20)
    same(got, orc.adjust_initial_flow(I0, I1, a0, a1, hint, 20), "adjustInitialFlow hint %d" % hint)
    assert got.any()                                        # differs from the zero flow it starts from
    # the inputs do hold what they are meant to: ties, and whole patches without alpha
    assert len(np.unique(q["I0"])) == 5
    hole = (q["a1"] == 0)
    assert hole[h // 3 + 4:h // 3 + 8, w // 4 + 4:w // 4 + 10].all()


# ---------------------------------------------------------------------------------------------------------------------------------
# patchMatchPropagationAndSearch, one level
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pct", [0, 20])
@pytest.mark.parametrize("hint", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("w,h", [(61, 45), (45, 61)])
def test_level_with_an_empty_flow(ref, orc, w, h, hint, pct):
    I0, I1, a0, a1, _ = rc.decode_level(rc.level_case_q(w, h, 11 + w))
    got = ref.level(I0, I1, a0, a1, None, hint, pct)
    same(got, orc.level(I0, I1, a0, a1, None, hint, pct), "level, empty flow")
    assert got.any()


@pytest.mark.parametrize("w,h,gate,pset", [(61, 45, "rects", None), (45, 61, "rects", None), (150, 131, "rects", None), (61, 45, "empty", None),
                                           (45, 61, "one", None), (61, 45, "rects", rc.SET_ODD), (150, 131, "rects", rc.SET_POW2)])
def test_level_with_an_incoming_flow(both, w, h, gate, pset):
    ref, orc, set_params = both
    I0, I1, a0, a1, fin = rc.decode_level(rc.level_case_q(w, h, 23 + h, gate))
    gated = int(((a0 > np.float32(0.9)) & (a1 > np.float32(0.9))).sum())
    assert gated == {"empty": 0, "one": 1}.get(gate, gated) and (gate != "rects" or gated > w * h // 4)
    set_params(pset)
    got = ref.level(I0, I1, a0, a1, fin, 0, 0)
    same(got, orc.level(I0, I1, a0, a1, fin, 0, 0), "level, incoming flow")
    assert not np.array_equal(got, fin)


@pytest.mark.parametrize("w,h", [(61, 45), (45, 61)])
def test_level_proposal_order_and_strict_comparison(both, w, h):
    """On ordinary data two different proposals never have exactly the same error, so neither the order of a sweep's two proposals
    (PixFlow.hpp:319-320, :332-333) nor the strict '<' of proposeFlowUpdate (:358) can be seen.  rc.tie_case_q makes such ties common."""
    ref, orc, set_params = both
    I0, I1, a0, a1, fin = rc.decode_level(rc.tie_case_q(w, h, 61 + w))
    set_params(rc.SET_TIES)
    # the ties are there: gated pixels whose left and upper neighbours carry different flows of exactly equal error, better than their own
    g0 = orc.gradients(I0); g1 = orc.gradients(I1)
    bl = orc.gaussian_blur(fin, 15, 8.0)
    err = lambda cand: orc.error_function(g0[0], g0[1], g1[0], g1[1], bl, np.ascontiguousarray(cand))
    left = np.roll(fin, 1, axis=1); up = np.roll(fin, 1, axis=0)
    e, el, eu = err(fin), err(left), err(up)
    gated = (a0 > np.float32(0.9)) & (a1 > np.float32(0.9))
    ties = gated & (el == eu) & (el < e) & (left != up).any(-1)
    assert int(ties[1:, 1:].sum()) >= 20
    assert int((gated & (el == e) & (left != fin).any(-1))[1:, 1:].sum()) >= 20      # a proposal exactly as good as the pixel's own flow
    got = ref.level(I0, I1, a0, a1, fin, 0, 0)
    same(got, orc.level(I0, I1, a0, a1, fin, 0, 0), "level with tied proposals")
    assert not np.array_equal(got, fin)


def test_level_fuzz(ref, orc):
    """12 seeded cases after the recipe of test_gpu_stages.py::test_level_fuzz_alpha_patterns."""
    r = np.random.default_rng(777)
    for case in range(12):
        w, h = int(r.integers(26, 180)), int(r.integers(26, 180))
        I0 = r.random((h, w)).astype(np.float32); I1 = np.roll(I0, int(r.integers(-3, 4)), axis=1) + 0.03 * r.random((h, w)).astype(np.float32)
        A0 = np.zeros((h, w), np.float32); A1 = np.zeros((h, w), np.float32)
        for A in (A0, A1):
            for _ in range(int(r.integers(0, 3)) + (case % 4 != 0)):
                x0, y0 = int(r.integers(0, w)), int(r.integers(0, h))
                A[y0:int(r.integers(y0, h)) + 1, x0:int(r.integers(x0, w)) + 1] = float(r.choice([1.0, 0.95, 0.6]))
        fin = (r.standard_normal((h, w, 2)) * 1.2).astype(np.float32)
        got = ref.level(I0, I1, A0, A1, fin, 0, 0)
        same(got, orc.level(I0, I1, A0, A1, fin, 0, 0), "fuzz case %d (%dx%d)" % (case, w, h))
        assert not np.array_equal(got, fin)


def test_diffusion(ref, orc):
    w, h = 64, 80
    r = np.random.default_rng(5)
    a0 = np.ones((h, w), np.float32); a1 = np.ones((h, w), np.float32)
    a0[10:30, 5:40] = 0.0; a1[25:60, 30:64] = 0.0; a1[70:, :10] = 0.0
    flow = (r.standard_normal((h, w, 2)) * 2).astype(np.float32)
    got = ref.diffusion(a0, a1, flow)
    same(got, orc.diffusion(a0, a1, flow), "lowAlphaFlowDiffusion")
    assert not np.array_equal(got, flow) and np.array_equal(got[40:60, :25], flow[40:60, :25])   # alpha 1 x 1: kept


# ---------------------------------------------------------------------------------------------------------------------------------
# whole runs
# ---------------------------------------------------------------------------------------------------------------------------------
SMALLEST_TWO_LEVEL = (56, 56)     # half size 28 x 28: int(28 * 0.9f + 0.5f) = 25 > 24, int(27 * 0.9f + 0.5f) = 24 is not


def test_smallest_two_level_size(orc):
    orc.reset_params()
    assert len(orc.pyramid_sizes(28, 28)) == 2 and len(orc.pyramid_sizes(27, 28)) == 1 and len(orc.pyramid_sizes(28, 27)) == 1


@pytest.fixture(scope="module")
def pairs(synth):
    return {s: synth.make_pair_np(s[0], s[1], 40 + s[0]) for s in [(301, 203), (320, 256), SMALLEST_TWO_LEVEL, (203, 131)]}


@pytest.mark.parametrize("hint", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("pct", [0, 20])
@pytest.mark.parametrize("size", [(301, 203), (320, 256), SMALLEST_TWO_LEVEL])
def test_compute_optical_flow(ref, orc, pairs, size, pct, hint):
    L, R, _ = pairs[size]
    got = ref.compute_optical_flow(L, R, pct, hint)
    same(got, orc.compute_optical_flow(L, R, pct, hint), "computeOpticalFlow")
    assert got.any()


def test_compute_optical_flow_non_preset(both, pairs):
    ref, orc, set_params = both
    L, R, _ = pairs[(301, 203)]
    preset = ref.compute_optical_flow(L, R, 20, 3)
    set_params(rc.SET_ODD)
    got = ref.compute_optical_flow(L, R, 20, 3)
    same(got, orc.compute_optical_flow(L, R, 20, 3), "computeOpticalFlow, non-preset")
    assert not np.array_equal(got, preset)


@pytest.mark.parametrize("pct", [0, 20])
@pytest.mark.parametrize("size", [(320, 256), (203, 131)])     # 203 / 20 = 10 (truncated) -> padded 223, half size 111 x 65 (both odd)
def test_prepare_both_flows(ref, orc, pairs, size, pct):
    L, R, _ = pairs[size]
    g0, g1 = ref.flow_bidir(L, R, pct)
    w0, w1 = orc.flow_bidir(L, R, pct)
    same(g0, w0, "flowLtoR"); same(g1, w1, "flowRtoL")
    assert g0.any() and g1.any() and not np.array_equal(g0, g1)


def test_combine_novel_views(ref, orc, synth):
    L, R, f0, f1, blend = rc.combine_case(synth)
    got = ref.combine_novel_views(L, R, f0, f1, blend)
    same(got, orc.combine_novel_views(L, R, f0, f1, blend), "combineNovelViews")
    assert not np.array_equal(got, L) and not np.array_equal(got, R)
    assert (got[..., 3] == 0).any() and (got[..., 3] == 255).any()
    assert (blend == 0).any() and (blend == 1).any()


# ---------------------------------------------------------------------------------------------------------------------------------
# StitchTool
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stitched(ref, synth):
    """name -> (L, R, hole, the reference's prepare outputs): computed once, shared by the prepare and the Gather cases."""
    out = {}
    for name in rc.CANVASES:
        L, R, hole = rc.canvas(synth, name)
        out[name] = (L, R, hole, ref.stitch_prepare(L, R))
    return out


@pytest.mark.parametrize("name", list(rc.CANVASES))
def test_stitch_prepare(stitched, orc, name):
    L, R, _, (mp, ovl, ovr, bl, md) = stitched[name]
    rows, cols = mp.shape
    assert min(cols, rows) >= 200
    assert (rows // 130) % 2 == (name != "tall_even") and (rows // 400 >= 2) == name.startswith("tall") and (cols <= rows) == (name != "wide_seam")
    wmp, wovl, wovr, wbl, wmd = orc.stitch_prepare(L, R, True)
    same(mp, wmp, "Map"); same(ovl, wovl, "OverlappedL"); same(ovr, wovr, "OverlappedR"); same(md, wmd, "MergedDis"); same(bl, wbl, "Blend")
    assert set(np.unique(mp)) == {0, 50, 100, 150} and not np.array_equal(ovl, L)
    ramp = bl[mp == 150]
    assert ((ramp > 0) & (ramp < 1)).any() and (md > min(cols, rows) // 200).any()        # a ramp, and tiles that get smoothed
    if name == "wide_seam":
        assert (mp[:, 0] == 150).any() and (mp[:, -1] == 150).any()                       # the overlap does cross the seam
    if name == "tall_even":
        assert (mp[380:430, 170:200] == 50).all()                                          # the notch: L is missing there


@pytest.mark.parametrize("name", list(rc.CANVASES))
def test_stitch_gather(ref, stitched, orc, name):
    L, R, hole, (mp, ovl, ovr, bl, md) = stitched[name]
    merged = rc.crafted_merged(mp, ovl, hole)
    gmap = rc.gather_map(mp, merged)
    assert (gmap == 150).sum() > 0 and rc.n150_near_border(gmap) == 0
    got = ref.stitch_gather(L, R, merged, mp)
    same(got, orc.stitch_gather(L, R, merged, mp), "Gather")
    assert not np.array_equal(got, L) and not np.array_equal(got, merged)
    # of the hole's pixels some find L, some R, by the 8-direction search
    hb = got[hole[1]:hole[3], hole[0]:hole[2]]
    assert (hb == L[hole[1]:hole[3], hole[0]:hole[2]]).all(-1).any() or (hb == R[hole[1]:hole[3], hole[0]:hole[2]]).all(-1).any()


def chain_inputs(synth):
    """top and two images on a 420 x 420 canvas; every overlap stays 100 px clear of the borders, so no Gather probe can leave the canvas."""
    cols = rows = 420
    top, l1 = rc.rect_canvas(synth, cols, rows, 51, [(60, 40, 360, 180)], [(110, 120, 310, 300)])
    l2, _ = rc.rect_canvas(synth, cols, rows, 52, [(130, 240, 290, 400)], [])
    return top, [l1, l2]


def run_chain(m, top, Ls, pct, stitch_prepare):
    """main.cpp's loop (CPU/main.cpp:60-96) over the module m (refcore or orc)."""
    R = top
    steps = []
    for L in Ls:
        mp, ovl, ovr, bl, md = stitch_prepare(L, R)
        f0, f1 = m.flow_bidir(ovl, ovr, pct)
        merged = m.combine_novel_views(ovl, ovr, f0, f1, bl)
        R = m.stitch_gather(L, R, merged, mp)
        steps.append((mp, bl, merged, R))
    return steps


def test_two_step_chain(ref, orc, synth):
    top, Ls = chain_inputs(synth)
    got = run_chain(ref, top, Ls, 20, ref.stitch_prepare)
    want = run_chain(orc, top, Ls, 20, lambda L, R: orc.stitch_prepare(L, R, True))
    for i, (g, w) in enumerate(zip(got, want)):
        for a, b, what in zip(g, w, ("Map", "Blend", "merged", "FinalResult")):
            same(a, b, "step %d %s" % (i + 1, what))
        assert rc.n150_near_border(rc.gather_map(g[0], g[2])) == 0
    assert not np.array_equal(got[1][3], got[0][3]) and not np.array_equal(got[0][3], top)


# ---------------------------------------------------------------------------------------------------------------------------------
# host AddressSanitizer: the same driver as one stand-alone sanitized program (oracle source rebuilt sanitized and linked in; no preload,
# no Python in the sanitized process; Mat::at checks its indices).  One case of each command: a clean exit shows that the inputs above stay
# outside the reference's out-of-bounds regimes, so no bit-equality above rests on an undefined read.
# ---------------------------------------------------------------------------------------------------------------------------------
def test_host_asan_pass(ref, orc, synth, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("refcore_asan") / "pano_ref_core_asan")
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "refcore_asan", "ASAN_OUT=" + exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    ref.use_exe(exe)
    try:
        assert ref.pyramid_sizes_range(101, 25, 400)[-1] == orc.pyramid_sizes(400, 101)
        g0, g1, blurred, c = _errfn_planes(orc, 40, 27)
        same(ref.error_function(g0[..., 0], g0[..., 1], g1[..., 0], g1[..., 1], blurred, c[3:6]),
             np.stack([orc.error_function(g0[..., 0], g0[..., 1], g1[..., 0], g1[..., 1], blurred, c[k]) for k in (3, 4, 5)]), "asan errfn")
        q = rc.adjust_case_q(29, 26, 3)
        I0, I1, a0, a1 = rc.img_f32(q["I0"]), rc.img_f32(q["I1"]), rc.img_f32(q["a0"]), rc.img_f32(q["a1"])
        pts = np.array([[0, 0, -3, -3], [28, 25, 31, 28], [5, 5, 7, 12], [14, 13, 12, 13]], np.int32)
        same(ref.patch_error(I0, a0, I1, a1, pts, 20), orc.patch_error(I0, a0, I1, a1, pts, 20), "asan patcherr")
        same(ref.adjust_initial_flow(I0, I1, a0, a1, 3, 20), orc.adjust_initial_flow(I0, I1, a0, a1, 3, 20), "asan adjust")
        I0, I1, a0, a1, fin = rc.decode_level(rc.level_case_q(61, 45, 23 + 45))
        same(ref.level(I0, I1, a0, a1, fin, 0, 0), orc.level(I0, I1, a0, a1, fin, 0, 0), "asan level")
        same(ref.level(I0, I1, a0, a1, None, 1, 20), orc.level(I0, I1, a0, a1, None, 1, 20), "asan level, empty flow")
        same(ref.diffusion(a0, a1, fin), orc.diffusion(a0, a1, fin), "asan diffusion")
        L, R, _ = synth.make_pair_np(203, 131, 40 + 203)
        same(ref.compute_optical_flow(L, R, 20, 2), orc.compute_optical_flow(L, R, 20, 2), "asan computeOpticalFlow")
        f0, f1 = ref.flow_bidir(L, R, 20)
        w0, w1 = orc.flow_bidir(L, R, 20)
        same(f0, w0, "asan prepare"); same(f1, w1, "asan prepare")
        cL, cR, c0, c1, cb = rc.combine_case(synth)
        same(ref.combine_novel_views(cL, cR, c0, c1, cb), orc.combine_novel_views(cL, cR, c0, c1, cb), "asan combine")
        L, R, hole = rc.canvas(synth, "small")
        mp, ovl, ovr, bl, md = ref.stitch_prepare(L, R)
        same(bl, orc.stitch_prepare(L, R, True)[3], "asan stitch prepare")
        merged = rc.crafted_merged(mp, ovl, hole)
        same(ref.stitch_gather(L, R, merged, mp), orc.stitch_gather(L, R, merged, mp), "asan Gather")
    finally:
        ref.use_exe(None)


# ---------------------------------------------------------------------------------------------------------------------------------
# the committed fixtures tests/golden/refcore_*.npz (made by tests/golden/make_refcore_golden.py from the DRIVER, not the oracle): the
# driver must keep reproducing them.  tests/test_gpu_refcore.py holds the HIP path to the same files.
# ---------------------------------------------------------------------------------------------------------------------------------
def test_driver_reproduces_the_committed_fixtures(ref, synth):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_refcore_golden", os.path.join(G, "make_refcore_golden.py"))
    mk = importlib.util.module_from_spec(spec); spec.loader.exec_module(mk)
    made = mk.make(synth)
    assert made, "no fixtures"
    for fname, arrays in made.items():
        path = os.path.join(G, fname)
        assert os.path.exists(path), "%s is not committed: run python tests/golden/make_refcore_golden.py" % fname
        have = np.load(path)
        assert sorted(have.files) == sorted(arrays), fname
        for k, v in arrays.items():
            v = np.asarray(v)
            assert have[k].dtype == v.dtype and have[k].shape == v.shape, (fname, k)
            assert np.array_equal(bits(have[k]), bits(v)) if v.dtype == np.float32 else np.array_equal(have[k], v), (fname, k)
        assert os.path.getsize(path) < (1 << 20), fname
