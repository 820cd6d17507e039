"""Every row-step argument of every host-buffer entry point of the core (include/panoflow.h: solver, stitch, plans, rig plans,
visualisers).  Each entry point gets ONE call whose step arguments are all padded and all different, on inputs whose padding is poison
(opaque pixels, region codes, large finite floats: asserted on the CPU to change what a reader with any other step of the call would
see) and outputs whose padding is 0xEE before and after.  Results equal the oracle's on the packed images, or the packed call's where
the oracle has no such function.  Then each step argument in turn is passed one byte below its row width: PF_ERR_ARG "row step too
small" before any work (no kernel family in the profile, outputs still filled, chains undisturbed).  Where the header lets planes share a
step (L and R, the two flows, a rig's images; overlapped_l/r at the input step) the layouts below pin it."""
import ctypes as C
import os

import numpy as np
import pytest

from abi_cases import In, Out, Run, Steps, ndiff, ptrs
from conftest import ROOT
from rig_cases import rig_codes
from test_flow_vis import Ref, build_ref

pytestmark = pytest.mark.gpu

PCT = 20
HINT_LEFT = 3
G = os.path.join(ROOT, "tests", "golden")
SC, SR = 240, 200    # the stitch fixture's canvas
VC, VR = 160, 128    # the flow fixture's


def _noop():
    pass


def _same(got, want, what):
    assert np.array_equal(got, want), "%s: %d elements differ" % (what, ndiff(got, want))


class Solver:
    """one solver shape: the pair, the blend weights and the oracle's results on the packed images"""

    def __init__(self, orc, synth, cols, rows):
        self.cols, self.rows = cols, rows
        self.L, self.R, self.blend = synth.make_pair_np(cols, rows, 9 + cols)
        self.flow = orc.compute_optical_flow(self.L, self.R, PCT, HINT_LEFT)
        self.f0, self.f1 = orc.flow_bidir(self.L, self.R, PCT)
        self.view = orc.combine_novel_views(self.L, self.R, self.f0, self.f1, self.blend)
        # pf_blend's flows are its caller's: any finite field will do, and one unlike the solve's shows a swap of the two
        r = np.random.default_rng(cols)
        self.g0 = (r.standard_normal((rows, cols, 2)) * 3).astype(np.float32)
        self.g1 = (r.standard_normal((rows, cols, 2)) * 3).astype(np.float32)
        self.blended = orc.combine_novel_views(self.L, self.R, self.g0, self.g1, self.blend)


@pytest.fixture(scope="module", params=[(52, 52), (61, 53)], ids=["52x52", "61x53"])
def solver(request, orc, synth):
    return Solver(orc, synth, *request.param)


class Stitch:
    """the stitch fixture's pair with the oracle's planes of one step, and a seeded chain of the same size for the chained entry points"""

    def __init__(self, orc, synth):
        g = np.load(os.path.join(G, "stitch_240x200.npz"))
        self.L, self.R, self.merged_in, self.final_of_merged = g["L"], g["R"], g["merged"], g["final"]
        self.map, self.ovl, self.ovr, self.blend, self.md = orc.stitch_prepare(self.L, self.R, True)
        _, _, _, self.raw, self.raw_md = orc.stitch_prepare(self.L, self.R, False)
        f0, f1 = orc.flow_bidir(self.ovl, self.ovr, PCT)
        self.final = orc.stitch_gather(self.L, self.R, orc.combine_novel_views(self.ovl, self.ovr, f0, f1, self.blend), self.map)
        top, imgs = synth.make_stitch_set(SC, SR, 31, 3)
        self.top, self.Ls = top.numpy(), [im.numpy() for im in imgs]
        # frames of the same rig (the masks of make_stitch_set do not depend on the seed)
        self.frames = [(self.top, self.Ls)]
        for seed in (32, 33):
            t, ims = synth.make_stitch_set(SC, SR, seed, 3)
            self.frames.append((t.numpy(), [im.numpy() for im in ims]))
        assert all(np.array_equal(t[..., 3] > 0, self.top[..., 3] > 0) for t, _ in self.frames)


@pytest.fixture(scope="module")
def stitch(orc, synth):
    return Stitch(orc, synth)


@pytest.fixture(scope="module")
def chains(pf, stitch):
    """the packed pf_stitch_step chains of the three frames: what the chained, batched and rig entry points must give from padded rows"""
    c = pf.Context(0)
    ref = [[c.stitch_step(L, top if i == 0 else None, PCT) for i, L in enumerate(Ls)] for top, Ls in stitch.frames]
    c.close()
    return ref


@pytest.fixture(scope="module")
def vis(tmp_path_factory):
    class V:
        pass
    v = V()
    g = np.load(os.path.join(G, "flow_160x128.npz"))
    v.flow, v.image = g["flowLR_s20"], g["L"]
    v.ref = Ref(build_ref(tmp_path_factory.mktemp("flow_vis_ref_abi")))
    return v


@pytest.fixture()
def ctx(pf):
    c = pf.Context(0)
    yield c
    c.close()


# ---- the calls: run_*(ctx, data, short=None, arm=_noop) -> Run.  arm() runs right before the entry point under test. ----

def run_flow(c, s, short=None, arm=_noop):
    st = Steps(short, step=(s.cols * 4, 12), fstep=(s.cols * 8, 40))
    i0, i1 = In(s.L, st["step"], 1), In(s.R, st["step"], 2)
    o = Out((s.rows, s.cols, 2), np.float32, st["fstep"])
    arm()
    rc = c.l.pf_flow(c.h, i0.ptr, i1.ptr, s.cols, s.rows, st.arg("step"), PCT, HINT_LEFT, o.ptr, st.arg("fstep"))
    return Run(rc, [i0, i1], {"flow": o}, st)


def run_flow_bidir(c, s, short=None, arm=_noop):
    st = Steps(short, step=(s.cols * 4, 20), fstep=(s.cols * 8, 8))
    l, r = In(s.L, st["step"], 1), In(s.R, st["step"], 2)
    o0, o1 = Out((s.rows, s.cols, 2), np.float32, st["fstep"]), Out((s.rows, s.cols, 2), np.float32, st["fstep"])
    arm()
    rc = c.l.pf_flow_bidir(c.h, l.ptr, r.ptr, s.cols, s.rows, st.arg("step"), PCT, o0.ptr, o1.ptr, st.arg("fstep"))
    return Run(rc, [l, r], {"flow_l2r": o0, "flow_r2l": o1}, st)


def run_blend(c, s, short=None, arm=_noop):
    st = Steps(short, step=(s.cols * 4, 12), fstep=(s.cols * 8, 16), bstep=(s.cols * 4, 20), ostep=(s.cols * 4, 28))
    l, r = In(s.L, st["step"], 1), In(s.R, st["step"], 2)
    f0, f1, b = In(s.g0, st["fstep"], 3), In(s.g1, st["fstep"], 4), In(s.blend, st["bstep"], 5)
    o = Out((s.rows, s.cols, 4), np.uint8, st["ostep"])
    arm()
    rc = c.l.pf_blend(c.h, l.ptr, r.ptr, st.arg("step"), f0.ptr, f1.ptr, st.arg("fstep"), b.ptr, st.arg("bstep"), s.cols, s.rows, o.ptr, st.arg("ostep"))
    return Run(rc, [l, r, f0, f1, b], {"out": o}, st)


def run_novel_view(c, s, short=None, arm=_noop):
    st = Steps(short, step=(s.cols * 4, 8), bstep=(s.cols * 4, 24), ostep=(s.cols * 4, 36), fstep=(s.cols * 8, 24))
    l, r, b = In(s.L, st["step"], 1), In(s.R, st["step"], 2), In(s.blend, st["bstep"], 3)
    o = Out((s.rows, s.cols, 4), np.uint8, st["ostep"])
    o0, o1 = Out((s.rows, s.cols, 2), np.float32, st["fstep"]), Out((s.rows, s.cols, 2), np.float32, st["fstep"])
    arm()
    rc = c.l.pf_novel_view(c.h, l.ptr, r.ptr, s.cols, s.rows, st.arg("step"), PCT, b.ptr, st.arg("bstep"), o.ptr, st.arg("ostep"), o0.ptr, o1.ptr,
                           st.arg("fstep"))
    return Run(rc, [l, r, b], {"out": o, "flow_l2r": o0, "flow_r2l": o1}, st)


def run_prepare(c, s, short=None, arm=_noop):
    st = Steps(short, step=(SC * 4, 16), mstep=(SC, 7), bstep=(SC * 4, 44))
    l, r = In(s.L, st["step"], 1), In(s.R, st["step"], 2)
    outs = {"map": Out((SR, SC), np.uint8, st["mstep"]), "overlapped_l": Out((SR, SC, 4), np.uint8, st["step"]),
            "overlapped_r": Out((SR, SC, 4), np.uint8, st["step"]), "blend": Out((SR, SC), np.float32, st["bstep"]),
            "merged_dis": Out((SR, SC), np.float32, SC * 4)}
    arm()
    rc = c.l.pf_stitch_prepare(c.h, l.ptr, r.ptr, SC, SR, st.arg("step"), outs["map"].ptr, st.arg("mstep"), outs["overlapped_l"].ptr, outs["overlapped_r"].ptr,
                               outs["blend"].ptr, st.arg("bstep"), outs["merged_dis"].ptr)
    return Run(rc, [l, r], outs, st)


def run_match(c, s, short=None, arm=_noop):
    st = Steps(short, step=(SC * 4, 28), mstep=(SC, 13))
    l, r = In(s.L, st["step"], 1), In(s.R, st["step"], 2)
    outs = {"map": Out((SR, SC), np.uint8, st["mstep"]), "overlapped_l": Out((SR, SC, 4), np.uint8, st["step"]),
            "overlapped_r": Out((SR, SC, 4), np.uint8, st["step"])}
    arm()
    rc = c.l.pf_stitch_match(c.h, l.ptr, r.ptr, SC, SR, st.arg("step"), outs["map"].ptr, st.arg("mstep"), outs["overlapped_l"].ptr, outs["overlapped_r"].ptr)
    return Run(rc, [l, r], outs, st)


def run_generate_blend(c, s, short=None, arm=_noop):
    st = Steps(short, mstep=(SC, 5), bstep=(SC * 4, 12))
    m = In(s.map, st["mstep"], 1)
    outs = {"blend": Out((SR, SC), np.float32, st["bstep"]), "merged_dis": Out((SR, SC), np.float32, SC * 4)}
    arm()
    rc = c.l.pf_stitch_generate_blend(c.h, m.ptr, st.arg("mstep"), SC, SR, outs["blend"].ptr, st.arg("bstep"), outs["merged_dis"].ptr)
    return Run(rc, [m], outs, st)


def run_raw_blend(c, s, short=None, arm=_noop):
    st = Steps(short, step=(SC * 4, 4), bstep=(SC * 4, 8))
    l, r = In(s.L, st["step"], 1), In(s.R, st["step"], 2)
    outs = {"raw_blend": Out((SR, SC), np.float32, st["bstep"]), "merged_dis": Out((SR, SC), np.float32, SC * 4)}
    arm()
    rc = c.l.pf_stitch_raw_blend(c.h, l.ptr, r.ptr, SC, SR, st.arg("step"), outs["raw_blend"].ptr, st.arg("bstep"), outs["merged_dis"].ptr)
    return Run(rc, [l, r], outs, st)


def run_gather(c, s, short=None, arm=_noop):
    st = Steps(short, step=(SC * 4, 20), mstep=(SC, 3), ostep=(SC * 4, 32))
    l, r, g, m = In(s.L, st["step"], 1), In(s.R, st["step"], 2), In(s.merged_in, st["step"], 3), In(s.map, st["mstep"], 4)
    o = Out((SR, SC, 4), np.uint8, st["ostep"])
    arm()
    rc = c.l.pf_stitch_gather(c.h, l.ptr, r.ptr, g.ptr, st.arg("step"), m.ptr, st.arg("mstep"), SC, SR, o.ptr, st.arg("ostep"))
    return Run(rc, [l, r, g, m], {"out": o}, st)


def run_step(c, s, short=None, arm=_noop, plan=None, L=None, R=None, chained=False):
    """pf_stitch_step (plan: pf_stitch_step_planned) of L over R (default: the fixture's pair); chained: r_bgra == NULL"""
    st = Steps(short, step=(SC * 4, 24), ostep=(SC * 4, 12))
    l = In(s.L if L is None else L, st["step"], 1)
    r = None if chained else In(s.R if R is None else R, st["step"], 2)
    o = Out((SR, SC, 4), np.uint8, st["ostep"])
    arm()
    if plan is None:
        rc = c.l.pf_stitch_step(c.h, l.ptr, None if chained else r.ptr, SC, SR, st.arg("step"), PCT, o.ptr, st.arg("ostep"))
    else:
        rc = c.l.pf_stitch_step_planned(c.h, plan.h, l.ptr, None if chained else r.ptr, SC, SR, st.arg("step"), PCT, o.ptr, st.arg("ostep"))
    return Run(rc, [l] + ([] if chained else [r]), {"out": o}, st)


def run_step_batch(c, s, short=None, arm=_noop, plan=None, pairs=None, in_flight=2):
    """pf_stitch_step_batch (plan: pf_stitch_step_batch_planned); pairs: [(L, R or None), ...]"""
    st = Steps(short, step=(SC * 4, 36), ostep=(SC * 4, 4))
    ls = [In(L, st["step"], 10 + k) for k, (L, _) in enumerate(pairs)]
    rs = [None if R is None else In(R, st["step"], 20 + k) for k, (_, R) in enumerate(pairs)]
    outs = [Out((SR, SC, 4), np.uint8, st["ostep"]) for _ in pairs]
    arm()
    if plan is None:
        rc = c.l.pf_stitch_step_batch(c.h, len(pairs), ptrs(ls), ptrs(rs), SC, SR, st.arg("step"), PCT, ptrs(outs), st.arg("ostep"), in_flight)
    else:
        rc = c.l.pf_stitch_step_batch_planned(c.h, plan.h, len(pairs), ptrs(ls), ptrs(rs), SC, SR, st.arg("step"), PCT, ptrs(outs), st.arg("ostep"), in_flight)
    return Run(rc, ls + [r for r in rs if r is not None], {"out %d" % k: o for k, o in enumerate(outs)}, st)


def run_plan_create(c, s, short=None, arm=_noop):
    """pf_stitch_plan_create, then (unless the creation was to be refused) pf_stitch_plan_download of it with padded planes of its own"""
    st = Steps(short, step=(SC * 4, 40), mstep=(SC, 9), bstep=(SC * 4, 16))
    l, r = In(s.L, st["step"], 1), In(s.R, st["step"], 2)
    outs = {"map": Out((SR, SC), np.uint8, st["mstep"]), "blend": Out((SR, SC), np.float32, st["bstep"])}
    h = C.c_void_p(None)
    if short != "step":
        assert c.l.pf_stitch_plan_create(c.h, l.ptr, r.ptr, SC, SR, C.c_size_t(st["step"]), C.byref(h)) == 0, c.l.pf_last_error(c.h).decode()
        arm()
        rc = c.l.pf_stitch_plan_download(c.h, h, outs["map"].ptr, st.arg("mstep"), outs["blend"].ptr, st.arg("bstep"))
    else:
        arm()
        rc = c.l.pf_stitch_plan_create(c.h, l.ptr, r.ptr, SC, SR, st.arg("step"), C.byref(h))
        assert h.value is None, "a refused creation handed out a plan"
    return Run(rc, [l, r], outs, st)


def run_rig_create(c, s, short=None, arm=_noop):
    st = Steps(short, step=(SC * 4, 52))
    top = In(s.top, st["step"], 1)
    ls = [In(L, st["step"], 2 + i) for i, L in enumerate(s.Ls)]
    h = C.c_void_p(None)
    arm()
    rc = c.l.pf_rig_plan_create(c.h, len(ls), top.ptr, ptrs(ls), SC, SR, st.arg("step"), C.byref(h))
    run = Run(rc, [top] + ls, {}, st)
    run.rig = h
    return run


def run_rig_stitch(c, s, rig, frames, short=None, arm=_noop, in_flight=1, lone=False):
    """pf_rig_stitch_batch of `frames` (lone: pf_rig_stitch of frames[0]), every composite asked for"""
    st = Steps(short, step=(SC * 4, 8), ostep=(SC * 4, 60))
    tops = [In(t, st["step"], 30 + k) for k, (t, _) in enumerate(frames)]
    ls = [In(L, st["step"], 40 + 8 * k + i) for k, (_, Ls) in enumerate(frames) for i, L in enumerate(Ls)]
    outs = [Out((SR, SC, 4), np.uint8, st["ostep"]) for _ in ls]
    arm()
    if lone:
        rc = c.l.pf_rig_stitch(c.h, rig.h, tops[0].ptr, ptrs(ls), SC, SR, st.arg("step"), PCT, ptrs(outs), st.arg("ostep"))
    else:
        rc = c.l.pf_rig_stitch_batch(c.h, rig.h, len(frames), ptrs(tops), ptrs(ls), SC, SR, st.arg("step"), PCT, ptrs(outs), st.arg("ostep"), in_flight)
    return Run(rc, tops + ls, {"out %d" % k: o for k, o in enumerate(outs)}, st)


def run_vis_grey(c, v, short=None, arm=_noop):
    st = Steps(short, fstep=(VC * 8, 24), ostep=(VC, 11))
    f, o = In(v.flow, st["fstep"], 1), Out((VR, VC), np.uint8, st["ostep"])
    arm()
    rc = c.l.pf_vis_grey_disparity(c.h, f.ptr, st.arg("fstep"), VC, VR, o.ptr, st.arg("ostep"))
    return Run(rc, [f], {"out": o}, st)


def run_vis_wheel(c, v, short=None, arm=_noop):
    st = Steps(short, fstep=(VC * 8, 8), ostep=(VC * 3, 7))
    f, o = In(v.flow, st["fstep"], 1), Out((VR, VC, 3), np.uint8, st["ostep"])
    arm()
    rc = c.l.pf_vis_color_wheel(c.h, f.ptr, st.arg("fstep"), VC, VR, o.ptr, st.arg("ostep"))
    return Run(rc, [f], {"out": o}, st)


def run_vis_field(c, v, short=None, arm=_noop):
    st = Steps(short, fstep=(VC * 8, 16), istep=(VC * 4, 12), ostep=(VC * 4, 20))
    f, im, o = In(v.flow, st["fstep"], 1), In(v.image, st["istep"], 2), Out((VR, VC, 4), np.uint8, st["ostep"])
    arm()
    rc = c.l.pf_vis_vector_field(c.h, f.ptr, st.arg("fstep"), im.ptr, st.arg("istep"), VC, VR, o.ptr, st.arg("ostep"))
    return Run(rc, [f, im], {"out": o}, st)


def run_vis_panel(c, v, short=None, arm=_noop):
    st = Steps(short, fstep=(VC * 8, 32), istep=(VC * 4, 4), ostep=(VC * 12, 28))
    f, im, o = In(v.flow, st["fstep"], 1), In(v.image, st["istep"], 2), Out((VR, 3 * VC, 4), np.uint8, st["ostep"])
    arm()
    rc = c.l.pf_vis_panel(c.h, f.ptr, st.arg("fstep"), im.ptr, st.arg("istep"), VC, VR, o.ptr, st.arg("ostep"))
    return Run(rc, [f, im], {"out": o}, st)


def run_stitch_visualize(c, s, short=None, arm=_noop):
    """both panels of the last pf_stitch_step; the two share the call's one step"""
    st = Steps(short, step=(SC * 12, 44))
    outs = {"l2r": Out((SR, 3 * SC, 4), np.uint8, st["step"]), "r2l": Out((SR, 3 * SC, 4), np.uint8, st["step"])}
    arm()
    rc = c.l.pf_stitch_visualize(c.h, outs["l2r"].ptr, outs["r2l"].ptr, st.arg("step"))
    return Run(rc, [], outs, st)


def _armed(c):
    """arm() for a refusal: the profile on and empty right before the call under test"""
    def arm():
        c.profile_enable(1)
        c.profile_reset()
    return arm


def _refusals(c, run, data, names, **kw):
    for name in names:
        r = run(c, data, short=name, arm=_armed(c), **kw)
        r.assert_refused(c)
        c.profile_enable(0)


# ---- solver ----

def test_flow(ctx, solver):
    r = run_flow(ctx, solver)
    r.assert_padded_ok(ctx)
    _same(r.outs["flow"].plane(), solver.flow, "pf_flow vs the oracle")
    _refusals(ctx, run_flow, solver, ("step", "fstep"))


def test_flow_bidir(ctx, solver):
    r = run_flow_bidir(ctx, solver)
    r.assert_padded_ok(ctx)
    _same(r.outs["flow_l2r"].plane(), solver.f0, "pf_flow_bidir L->R vs the oracle")
    _same(r.outs["flow_r2l"].plane(), solver.f1, "pf_flow_bidir R->L vs the oracle")
    _refusals(ctx, run_flow_bidir, solver, ("step", "fstep"))


def test_blend(ctx, solver):
    r = run_blend(ctx, solver)
    r.assert_padded_ok(ctx)
    _same(r.outs["out"].plane(), solver.blended, "pf_blend vs the oracle")
    _refusals(ctx, run_blend, solver, ("step", "fstep", "bstep", "ostep"))


def test_novel_view(ctx, solver):
    r = run_novel_view(ctx, solver)
    r.assert_padded_ok(ctx)
    _same(r.outs["flow_l2r"].plane(), solver.f0, "pf_novel_view L->R vs the oracle")
    _same(r.outs["flow_r2l"].plane(), solver.f1, "pf_novel_view R->L vs the oracle")
    _same(r.outs["out"].plane(), solver.view, "pf_novel_view vs the oracle")
    _refusals(ctx, run_novel_view, solver, ("step", "bstep", "ostep", "fstep"))


def test_null_optional_planes_with_step_0_stay_accepted(ctx, solver, stitch):
    s, z = solver, C.c_size_t(0)
    l, r, b = In(s.L, s.cols * 4 + 4, 1), In(s.R, s.cols * 4 + 4, 2), In(s.blend, s.cols * 4 + 8, 3)
    o = Out((s.rows, s.cols, 4), np.uint8, s.cols * 4 + 12)
    f = Out((s.rows, s.cols, 2), np.float32, s.cols * 8 + 16)
    step = C.c_size_t(l.step)
    # no flows wanted: fstep 0; no view wanted: bstep and ostep 0 (what pf_flow_bidir passes); one flow only
    assert ctx.l.pf_novel_view(ctx.h, l.ptr, r.ptr, s.cols, s.rows, step, PCT, b.ptr, C.c_size_t(b.step), o.ptr, C.c_size_t(o.step), None, None, z) == 0
    _same(o.plane(), s.view, "pf_novel_view without flows")
    assert ctx.l.pf_novel_view(ctx.h, l.ptr, r.ptr, s.cols, s.rows, step, PCT, None, z, None, z, None, f.ptr, C.c_size_t(f.step)) == 0
    _same(f.plane(), s.f1, "pf_novel_view, R->L flow only")
    assert f.padding_kept() and o.padding_kept()
    t = stitch
    tl, tr = In(t.L, SC * 4 + 4, 1), In(t.R, SC * 4 + 4, 2)
    assert ctx.l.pf_stitch_prepare(ctx.h, tl.ptr, tr.ptr, SC, SR, C.c_size_t(tl.step), None, z, None, None, None, z, None) == 0
    assert ctx.l.pf_stitch_match(ctx.h, tl.ptr, tr.ptr, SC, SR, C.c_size_t(tl.step), None, z, None, None) == 0
    assert ctx.l.pf_stitch_step(ctx.h, tl.ptr, tr.ptr, SC, SR, C.c_size_t(tl.step), PCT, None, z) == 0
    assert ctx.l.pf_stitch_step_batch(ctx.h, 1, ptrs([tl]), ptrs([tr]), SC, SR, C.c_size_t(tl.step), PCT, None, z, 1) == 0
    plan = ctx.stitch_plan(t.L, t.R)
    assert ctx.l.pf_stitch_plan_download(ctx.h, plan.h, None, z, None, z) == 0


# ---- stitch ----

def test_stitch_prepare(ctx, stitch):
    r = run_prepare(ctx, stitch)
    r.assert_padded_ok(ctx)
    for name, want in (("map", stitch.map), ("overlapped_l", stitch.ovl), ("overlapped_r", stitch.ovr), ("blend", stitch.blend), ("merged_dis", stitch.md)):
        _same(r.outs[name].plane(), want, "pf_stitch_prepare %s vs the oracle" % name)
    _refusals(ctx, run_prepare, stitch, ("step", "mstep", "bstep"))


def test_stitch_match(ctx, stitch):
    r = run_match(ctx, stitch)
    r.assert_padded_ok(ctx)
    for name, want in (("map", stitch.map), ("overlapped_l", stitch.ovl), ("overlapped_r", stitch.ovr)):
        _same(r.outs[name].plane(), want, "pf_stitch_match %s vs the oracle" % name)
    _refusals(ctx, run_match, stitch, ("step", "mstep"))


def test_stitch_generate_blend(ctx, stitch):
    r = run_generate_blend(ctx, stitch)
    r.assert_padded_ok(ctx)
    _same(r.outs["blend"].plane(), stitch.blend, "pf_stitch_generate_blend ramp vs the oracle")
    _same(r.outs["merged_dis"].plane(), stitch.md, "pf_stitch_generate_blend MergedDis vs the oracle")
    _refusals(ctx, run_generate_blend, stitch, ("mstep", "bstep"))


def test_stitch_raw_blend(ctx, stitch):
    r = run_raw_blend(ctx, stitch)
    r.assert_padded_ok(ctx)
    ov = stitch.map == 150   # countblend is defined in the overlap; outside it the ramp is 0 / 1 / 0.5 by region code, as the oracle's
    _same(r.outs["raw_blend"].plane()[ov], stitch.raw[ov], "pf_stitch_raw_blend vs the oracle, overlap")
    _same(r.outs["raw_blend"].plane(), stitch.raw, "pf_stitch_raw_blend vs the oracle")
    _same(r.outs["merged_dis"].plane(), stitch.raw_md, "pf_stitch_raw_blend MergedDis vs the oracle")
    _refusals(ctx, run_raw_blend, stitch, ("step", "bstep"))


def test_stitch_gather(ctx, stitch):
    r = run_gather(ctx, stitch)
    r.assert_padded_ok(ctx)
    _same(r.outs["out"].plane(), stitch.final_of_merged, "pf_stitch_gather vs the oracle")
    _refusals(ctx, run_gather, stitch, ("step", "mstep", "ostep"))


def test_stitch_step(ctx, stitch, chains):
    r = run_step(ctx, stitch)
    r.assert_padded_ok(ctx)
    _same(r.outs["out"].plane(), stitch.final, "pf_stitch_step vs the oracle's prepare / flows / blend / gather")
    # a chain from padded rows, with a refusal of either step between its steps: the next chained call gives the undisturbed chain's bytes
    top, Ls = stitch.frames[0]
    r = run_step(ctx, stitch, L=Ls[0], R=top)
    r.assert_padded_ok(ctx)
    _same(r.outs["out"].plane(), chains[0][0], "step 1 of the chain vs the packed call")
    _refusals(ctx, run_step, stitch, ("step", "ostep"), L=Ls[1], chained=True)
    r = run_step(ctx, stitch, L=Ls[1], chained=True)
    r.assert_padded_ok(ctx)
    _same(r.outs["out"].plane(), chains[0][1], "step 2 of the chain, after two refused calls, vs the packed chain")


def test_stitch_prefetch_and_the_step_that_consumes_it(ctx, stitch, chains):
    top, Ls = stitch.frames[0]
    st = Steps(None, step=(SC * 4, 24), pstep=(SC * 4, 48))
    nxt = In(Ls[1], st["pstep"], 7)   # the announced image lives at a step of its own
    nxt.assert_poison_seen([SC * 4, st["step"]])
    assert ctx.l.pf_stitch_prefetch(ctx.h, nxt.ptr, SC, SR, C.c_size_t(st["pstep"])) == 0
    r = run_step(ctx, stitch, L=Ls[0], R=top)        # uploads nxt beside its own kernels
    r.assert_padded_ok(ctx)
    _same(r.outs["out"].plane(), chains[0][0], "step 1 with a prefetch announced")
    o = Out((SR, SC, 4), np.uint8, SC * 4 + 12)
    assert ctx.l.pf_stitch_step(ctx.h, nxt.ptr, None, SC, SR, C.c_size_t(st["pstep"]), PCT, o.ptr, C.c_size_t(o.step)) == 0
    assert o.padding_kept()
    _same(o.plane(), chains[0][1], "step 2 from the prefetched copy vs the packed chain")
    # a short step is refused in the words of the other entry points, announces nothing, and leaves the chain as it is
    ctx.profile_enable(1); ctx.profile_reset()
    assert ctx.l.pf_stitch_prefetch(ctx.h, nxt.ptr, SC, SR, C.c_size_t(SC * 4 - 1)) == -1
    assert "row step too small" in ctx.l.pf_last_error(ctx.h).decode()
    assert not [k for k, (_, n) in ctx.profile().items() if n]
    ctx.profile_enable(0)
    r = run_step(ctx, stitch, L=Ls[2], chained=True)
    r.assert_padded_ok(ctx)
    _same(r.outs["out"].plane(), chains[0][2], "step 3 after a refused prefetch vs the packed chain")


def test_stitch_step_batch(ctx, stitch, chains):
    (t0, l0), (t1, l1) = stitch.frames[0], stitch.frames[1]
    r = run_step_batch(ctx, stitch, pairs=[(stitch.L, stitch.R), (l0[0], t0), (l1[0], t1)])
    r.assert_padded_ok(ctx)
    _same(r.outs["out 0"].plane(), stitch.final, "frame 0 vs the oracle")
    _same(r.outs["out 1"].plane(), chains[0][0], "frame 1 vs the packed pf_stitch_step")
    _same(r.outs["out 2"].plane(), chains[1][0], "frame 2 vs the packed pf_stitch_step")
    # the slots chain; a refused call between two chained ones leaves them as they were
    r = run_step_batch(ctx, stitch, pairs=[(l0[0], t0), (l1[0], t1)])
    r.assert_padded_ok(ctx)
    _refusals(ctx, run_step_batch, stitch, ("step", "ostep"), pairs=[(l0[1], None), (l1[1], None)])
    r = run_step_batch(ctx, stitch, pairs=[(l0[1], None), (l1[1], None)])
    r.assert_padded_ok(ctx)
    _same(r.outs["out 0"].plane(), chains[0][1], "slot 0, step 2 after two refused calls")
    _same(r.outs["out 1"].plane(), chains[1][1], "slot 1, step 2 after two refused calls")


# ---- stitch plans ----

def test_stitch_plan_create_and_download(ctx, stitch):
    r = run_plan_create(ctx, stitch)
    r.assert_padded_ok(ctx)
    _same(r.outs["map"].plane(), stitch.map, "plan map vs the oracle")
    _same(r.outs["blend"].plane(), stitch.blend, "plan ramp vs the oracle")
    _refusals(ctx, run_plan_create, stitch, ("step", "mstep", "bstep"))


def test_stitch_step_planned_and_batch_planned(ctx, stitch):
    plan = ctx.stitch_plan(stitch.L, stitch.R)
    r = run_step(ctx, stitch, plan=plan)
    r.assert_padded_ok(ctx)
    _same(r.outs["out"].plane(), stitch.final, "pf_stitch_step_planned vs the oracle")
    _refusals(ctx, run_step, stitch, ("step", "ostep"), plan=plan)
    r = run_step_batch(ctx, stitch, plan=plan, pairs=[(stitch.L, stitch.R)] * 3)
    r.assert_padded_ok(ctx)
    for k in range(3):
        _same(r.outs["out %d" % k].plane(), stitch.final, "pf_stitch_step_batch_planned frame %d vs the oracle" % k)
    _refusals(ctx, run_step_batch, stitch, ("step", "ostep"), plan=plan, pairs=[(stitch.L, stitch.R)] * 2)


# ---- rig plans ----

def test_rig_plan_create(pf, ctx, stitch):
    r = run_rig_create(ctx, stitch)
    r.assert_padded_ok(ctx)
    rig = pf.RigPlan(ctx, r.rig.value)
    packed = ctx.rig_plan(stitch.top, stitch.Ls)
    codes = rig_codes(stitch.top, stitch.Ls)
    for i in range(3):
        mp, ramp = rig.steps[i].download()
        _same(mp, codes[i], "step %d map vs the region codes of the masks" % (i + 1))
        _same(ramp, packed.steps[i].download()[1], "step %d ramp vs the packed creation" % (i + 1))
    _same(rig.steps[0].download()[0], ctx.stitch_prepare(stitch.Ls[0], stitch.top)[0], "step 1 map vs pf_stitch_prepare")
    _refusals(ctx, run_rig_create, stitch, ("step",))


def test_rig_stitch(ctx, stitch, chains):
    rig = ctx.rig_plan(stitch.top, stitch.Ls)
    r = run_rig_stitch(ctx, stitch, rig, stitch.frames[1:2], lone=True)
    r.assert_padded_ok(ctx)
    for i in range(3):
        _same(r.outs["out %d" % i].plane(), chains[1][i], "pf_rig_stitch step %d vs the packed pf_stitch_step chain" % (i + 1))
    _refusals(ctx, lambda c, s, **kw: run_rig_stitch(c, s, rig, stitch.frames[1:2], lone=True, **kw), stitch, ("step", "ostep"))


@pytest.mark.parametrize("overlap", [1, 0])
def test_rig_stitch_batch_of_three_waves(ctx, stitch, chains, overlap):
    """three frames at in_flight 1: wave 3 goes up a second time, beside wave 2's compute on the copy stream (1) or between the waves (0)"""
    ctx.rig_set_upload_overlap(overlap)
    rig = ctx.rig_plan(stitch.top, stitch.Ls)
    r = run_rig_stitch(ctx, stitch, rig, stitch.frames, in_flight=1)
    r.assert_padded_ok(ctx)
    for k in range(3):
        for i in range(3):
            _same(r.outs["out %d" % (3 * k + i)].plane(), chains[k][i], "frame %d step %d vs the packed pf_stitch_step chain" % (k, i + 1))
    _refusals(ctx, lambda c, s, **kw: run_rig_stitch(c, s, rig, stitch.frames, in_flight=1, **kw), stitch, ("step", "ostep"))


# ---- visualisers ----

@pytest.mark.parametrize("run,ref,names", [(run_vis_grey, lambda v: v.ref.grey(v.flow), ("fstep", "ostep")),
                                           (run_vis_wheel, lambda v: v.ref.wheel(v.flow), ("fstep", "ostep")),
                                           (run_vis_field, lambda v: v.ref.field(v.flow, v.image), ("fstep", "istep", "ostep")),
                                           (run_vis_panel, lambda v: v.ref.panel(v.flow, v.image), ("fstep", "istep", "ostep"))],
                         ids=["grey_disparity", "color_wheel", "vector_field", "panel"])
def test_visualisers(ctx, vis, run, ref, names):
    r = run(ctx, vis)
    r.assert_padded_ok(ctx)
    _same(r.outs["out"].plane(), ref(vis), "vs the host reference")
    _refusals(ctx, run, vis, names)


def test_stitch_visualize(ctx, stitch):
    ctx.stitch_step(stitch.L, stitch.R, PCT, want_out=False)
    want = ctx.stitch_visualize((SR, SC))
    r = run_stitch_visualize(ctx, stitch)
    r.assert_padded_ok(ctx)
    _same(r.outs["l2r"].plane(), want[0], "L->R panel vs the packed call")
    _same(r.outs["r2l"].plane(), want[1], "R->L panel vs the packed call")
    _same(want[0], ctx.vis_panel(ctx.flow_bidir(stitch.ovl, stitch.ovr, PCT)[0], stitch.L), "L->R panel vs pf_vis_panel of the step's flow")
    ctx.stitch_step(stitch.L, stitch.R, PCT, want_out=False)   # (the solve above reused the step's flow buffers)
    _refusals(ctx, run_stitch_visualize, stitch, ("step",))
    got = ctx.stitch_visualize((SR, SC))
    _same(got[0], want[0], "the panels after a refused call")
