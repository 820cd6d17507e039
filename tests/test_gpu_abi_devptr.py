"""Caller-owned device pointers of the device forms (include/panoflow.h: "device-resident entry points").  The contract is the element's
natural alignment (BGRA and float planes 4 bytes, flows 8) and no output inside an input or another output of the call.
Equality: every caller-owned pointer placed at exactly that alignment inside a larger allocation (+4 / +8) gives the bytes the same call
gives on allocation-aligned pointers (and the oracle's, for the solver forms), and the allocation around the plane keeps its 0xEE.
Refusals: a pointer below the alignment, or an overlapping output, is PF_ERR_ARG before any work (no kernel family in the profile, every
output still filled).  DESIGN.md 8.9 holds the audit of the kernels behind these pointers."""
import ctypes as C

import numpy as np
import pytest

from abi_cases import FILL, ndiff
from test_gpu_abi_steps import PCT, SC, SR, Solver, Stitch

pytestmark = pytest.mark.gpu

COLS, ROWS = 61, 53   # the smallest odd solver shape of the suite: both sweep forms run at any size when the context asks for one


class Dev:
    """a caller-owned device plane `off` bytes into an allocation of its own; every other byte of the allocation holds FILL"""

    def __init__(self, pool, nbytes, off, data=None):
        self.c, self.n, self.off = pool.c, int(nbytes), int(off)
        self.total = self.off + self.n + 64
        self.base = self.c.dev_alloc(self.total)
        pool.devs.append(self)
        host = np.full(self.total, FILL, np.uint8)
        if data is not None:
            host[self.off:self.off + self.n] = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        self.c.upload(self.base, host)
        self.ptr = self.base + self.off

    def _host(self):
        return self.c.download(np.empty(self.total, np.uint8), self.base)

    def get(self, shape, dtype):
        h = self._host()
        assert (h[:self.off] == FILL).all() and (h[self.off + self.n:] == FILL).all(), "the allocation around the plane was written"
        return h[self.off:self.off + self.n].copy().view(dtype).reshape(shape)

    def untouched(self):
        return bool((self._host() == FILL).all())


class Pool:
    def __init__(self, c):
        self.c, self.devs = c, []

    def plane(self, data, off):
        data = np.ascontiguousarray(data)
        return Dev(self, data.nbytes, off, data)

    def out(self, nbytes, off):
        return Dev(self, nbytes, off)

    def free(self):
        for d in self.devs:
            self.c.dev_free(d.base)
        self.devs = []


@pytest.fixture(scope="module")
def pair(orc, synth):
    return Solver(orc, synth, COLS, ROWS)


@pytest.fixture(scope="module")
def stitch(orc, synth):
    return Stitch(orc, synth)


@pytest.fixture()
def ctx(pf):
    c = pf.Context(0)
    pool = Pool(c)
    c.pool = pool
    yield c
    pool.free()
    c.close()


def _same(got, want, what):
    assert np.array_equal(got, want), "%s: %d elements differ" % (what, ndiff(got, want))


N = COLS * ROWS
IMG, FLOW = (ROWS, COLS, 4), (ROWS, COLS, 2)


# ---- equality: the solver forms ----

def _flow_bidir(c, s, o4, o8):
    p = c.pool
    l, r, f0, f1 = p.plane(s.L, o4), p.plane(s.R, o4), p.out(N * 8, o8), p.out(N * 8, o8)
    c.flow_bidir_dev(l.ptr, r.ptr, COLS, ROWS, PCT, f0.ptr, f1.ptr)
    return f0.get(FLOW, np.float32), f1.get(FLOW, np.float32)


def _blend(c, s, o4, o8):
    p = c.pool
    l, r, g0, g1, b, o = p.plane(s.L, o4), p.plane(s.R, o4), p.plane(s.g0, o8), p.plane(s.g1, o8), p.plane(s.blend, o4), p.out(N * 4, o4)
    c.blend_dev(l.ptr, r.ptr, g0.ptr, g1.ptr, b.ptr, COLS, ROWS, o.ptr)
    return (o.get(IMG, np.uint8),)


def _novel_view(c, s, o4, o8):
    p = c.pool
    l, r, b, o, f0, f1 = p.plane(s.L, o4), p.plane(s.R, o4), p.plane(s.blend, o4), p.out(N * 4, o4), p.out(N * 8, o8), p.out(N * 8, o8)
    c.novel_view_dev(l.ptr, r.ptr, COLS, ROWS, PCT, b.ptr, o.ptr, f0.ptr, f1.ptr)
    return o.get(IMG, np.uint8), f0.get(FLOW, np.float32), f1.get(FLOW, np.float32)


def _novel_view_batch(c, s, o4, o8, n=3, in_flight=2):
    """pairs 0 and 2 are the fixture's, pair 1 is it mirrored: a batch of two and a lone pair behind it (two groups)"""
    p = c.pool
    flip = lambda a: np.ascontiguousarray(a[:, ::-1])
    src = [(s.L, s.R, s.blend), (flip(s.L), flip(s.R), flip(s.blend)), (s.L, s.R, s.blend)][:n]
    d = [dict(l=p.plane(L, o4), r=p.plane(R, o4), b=p.plane(b, o4), o=p.out(N * 4, o4), f0=p.out(N * 8, o8), f1=p.out(N * 8, o8)) for L, R, b in src]
    col = lambda k: [x[k].ptr for x in d]
    c.novel_view_batch_dev(col("l"), col("r"), COLS, ROWS, PCT, col("b"), col("o"), col("f0"), col("f1"), in_flight=in_flight)
    return tuple(a for x in d for a in (x["o"].get(IMG, np.uint8), x["f0"].get(FLOW, np.float32), x["f1"].get(FLOW, np.float32)))


def test_flow_bidir_dev_and_blend_dev_at_the_natural_alignment(ctx, pair):
    got, want = _flow_bidir(ctx, pair, 4, 8), _flow_bidir(ctx, pair, 0, 0)
    for g, w, o, name in zip(got, want, (pair.f0, pair.f1), ("L->R", "R->L")):
        _same(g, w, "pf_flow_bidir_dev %s, planes at +4 / +8 vs allocation-aligned" % name)
        _same(g, o, "pf_flow_bidir_dev %s vs the oracle" % name)
    got, want = _blend(ctx, pair, 4, 8), _blend(ctx, pair, 0, 0)
    _same(got[0], want[0], "pf_blend_dev, planes at +4 / +8 vs allocation-aligned")
    _same(got[0], pair.blended, "pf_blend_dev vs the oracle")


@pytest.mark.parametrize("sweep_wide", [0, 2])
def test_novel_view_dev_lone_and_batched_at_the_natural_alignment(pf, pair, sweep_wide):
    c = pf.Context(0, sweep_wide=sweep_wide)
    c.pool = Pool(c)
    try:
        got, want = _novel_view(c, pair, 4, 8), _novel_view(c, pair, 0, 0)
        for g, w, o, name in zip(got, want, (pair.view, pair.f0, pair.f1), ("view", "L->R", "R->L")):
            _same(g, w, "pf_novel_view_dev %s, sweep form %d, planes at +4 / +8 vs allocation-aligned" % (name, sweep_wide))
            _same(g, o, "pf_novel_view_dev %s, sweep form %d, vs the oracle" % (name, sweep_wide))
        got, want = _novel_view_batch(c, pair, 4, 8), _novel_view_batch(c, pair, 0, 0)
        for k, (g, w) in enumerate(zip(got, want)):
            _same(g, w, "pf_novel_view_batch_dev pair %d %s, sweep form %d, planes at +4 / +8 vs allocation-aligned" % (k // 3, ("view", "L->R", "R->L")[k % 3], sweep_wide))
        for k in (0, 6):   # pairs 0 and 2 are the fixture's own
            for g, o in zip(got[k:k + 3], (pair.view, pair.f0, pair.f1)):
                _same(g, o, "pf_novel_view_batch_dev pair %d, sweep form %d, vs the oracle" % (k // 3, sweep_wide))
    finally:
        c.pool.free()
        c.close()


# ---- equality: the stitch, plan, rig and panel device forms ----

NB = SC * SR * 4
CANVAS = (SR, SC, 4)


def _stitch_batch(c, s, off, plan=None):
    p = c.pool
    pairs = [(s.L, s.R)] * 3 if plan is not None else [(s.L, s.R), (s.Ls[0], s.top), (s.frames[1][1][0], s.frames[1][0])]
    d = [(p.plane(L, off), p.plane(R, off), p.out(NB, off)) for L, R in pairs]
    c.stitch_step_batch_dev([x[0].ptr for x in d], [x[1].ptr for x in d], SC, SR, PCT, [x[2].ptr for x in d], in_flight=2, plan=plan)
    return [x[2].get(CANVAS, np.uint8) for x in d]


def test_stitch_step_batch_dev_and_planned_dev_at_plus_4(ctx, stitch):
    got, want = _stitch_batch(ctx, stitch, 4), _stitch_batch(ctx, stitch, 0)
    for k in range(3):
        _same(got[k], want[k], "pf_stitch_step_batch_dev frame %d, planes at +4 vs allocation-aligned" % k)
    _same(got[0], stitch.final, "pf_stitch_step_batch_dev frame 0 vs the oracle")
    plan = ctx.stitch_plan(stitch.L, stitch.R)
    got, want = _stitch_batch(ctx, stitch, 4, plan), _stitch_batch(ctx, stitch, 0, plan)
    for k in range(3):
        _same(got[k], want[k], "pf_stitch_step_batch_planned_dev frame %d, planes at +4 (the match's 4-byte path) vs allocation-aligned" % k)
        _same(got[k], stitch.final, "pf_stitch_step_batch_planned_dev frame %d vs the oracle" % k)


def test_stitch_plan_create_dev_at_plus_4(ctx, stitch):
    p = ctx.pool
    for off in (4, 0):
        l, r = p.plane(stitch.L, off), p.plane(stitch.R, off)
        mp, ramp = ctx.stitch_plan_dev(l.ptr, r.ptr, SC, SR).download()
        _same(mp, stitch.map, "plan map, images at +%d, vs the oracle" % off)
        _same(ramp, stitch.blend, "plan ramp, images at +%d, vs the oracle" % off)
        l.get(CANVAS, np.uint8), r.get(CANVAS, np.uint8)   # (the allocations around the inputs)


def _rig(c, s, off, frames, lone=False):
    """the rig's plan from device images, then its chain of `frames` with every composite in the caller's buffers"""
    p = c.pool
    top, ls = p.plane(s.top, off), [p.plane(L, off) for L in s.Ls]
    rig = c.rig_plan_dev(top.ptr, [x.ptr for x in ls], SC, SR)
    plans = [st.download() for st in rig.steps]
    d = [(p.plane(t, off), [p.plane(L, off) for L in Ls], [p.out(NB, off) for _ in Ls]) for t, Ls in frames]
    if lone:
        t, Ls, outs = d[0]
        arr = lambda v: (C.c_void_p * len(v))(*[C.c_void_p(x.ptr) for x in v])
        c._chk(c.l.pf_rig_stitch_dev(c.h, rig.h, C.c_void_p(t.ptr), arr(Ls), SC, SR, PCT, arr(outs)))
    else:
        c.rig_stitch_batch_dev(rig, [x[0].ptr for x in d], [[y.ptr for y in x[1]] for x in d], PCT, [[y.ptr for y in x[2]] for x in d], in_flight=2)
    return plans, [[o.get(CANVAS, np.uint8) for o in x[2]] for x in d]


@pytest.mark.parametrize("lone", [True, False], ids=["pf_rig_stitch_dev", "pf_rig_stitch_batch_dev"])
def test_rig_device_forms_at_plus_4(ctx, stitch, lone):
    frames = stitch.frames[:1] if lone else stitch.frames
    (gp, got), (wp, want) = _rig(ctx, stitch, 4, frames, lone), _rig(ctx, stitch, 0, frames, lone)
    for i in range(3):
        _same(gp[i][0], wp[i][0], "rig plan step %d map, images at +4 vs allocation-aligned" % (i + 1))
        _same(gp[i][1], wp[i][1], "rig plan step %d ramp, images at +4 vs allocation-aligned" % (i + 1))
    for k in range(len(frames)):
        for i in range(3):
            _same(got[k][i], want[k][i], "frame %d step %d, planes at +4 vs allocation-aligned" % (k, i + 1))
    chain = [ctx.stitch_step(L, stitch.top if i == 0 else None, PCT) for i, L in enumerate(stitch.Ls)]
    for i in range(3):
        _same(got[0][i], chain[i], "frame 0 step %d vs the pf_stitch_step chain" % (i + 1))


def test_vis_panel_dev_at_the_natural_alignment(ctx, stitch):
    r = np.random.default_rng(5)
    flow = (r.standard_normal((SR, SC, 2)) * 5).astype(np.float32)
    outs = []
    for o4, o8 in ((4, 8), (0, 0)):
        f, im, o = ctx.pool.plane(flow, o8), ctx.pool.plane(stitch.L, o4), ctx.pool.out(NB * 3, o4)
        ctx.vis_panel_dev(f.ptr, im.ptr, SC, SR, o.ptr)
        outs.append(o.get((SR, 3 * SC, 4), np.uint8))
    _same(outs[0], outs[1], "pf_vis_panel_dev, planes at +4 / +8 vs allocation-aligned")
    _same(outs[0], ctx.vis_panel(flow, stitch.L), "pf_vis_panel_dev vs the host form")


# ---- refusals ----

def _refused(pf, c, call, outs, words):
    c.profile_enable(1)
    c.profile_reset()
    with pytest.raises(pf.PanoflowError, match=r"error -1: .*" + words):
        call()
    ran = sorted(k for k, (_, n) in c.profile().items() if n)
    c.profile_enable(0)
    assert not ran, "kernels ran before the refusal: %r" % ran
    for o in outs:
        assert o.untouched(), "an output was written by a refused call"


def _solver_form_refusals(pf, c, names, aligns, out_names, make_call, planes):
    """names: the pointer arguments in order; aligns[name]: 4 or 8; every argument once below its alignment, every output once on top of
    (or one row into) every input and every later output"""
    outs = [planes[n] for n in out_names]
    base = {n: planes[n].ptr for n in names}
    for n in names:
        bad = dict(base); bad[n] += aligns[n] // 2 if aligns[n] == 8 else 1    # a flow at +4 is aligned for floats, not for (dx, dy) pairs
        _refused(pf, c, make_call(bad), outs, "%s is not %d-byte aligned" % (n, aligns[n]))
    k = 0
    for o in out_names:
        for other in names:
            if other == o or (other in out_names and out_names.index(other) < out_names.index(o)):
                continue
            bad = dict(base); bad[o] = base[other] + (0 if k % 2 == 0 else 8 * COLS); k += 1
            _refused(pf, c, make_call(bad), outs, "overlaps")


def test_core_device_forms_refuse_misaligned_and_overlapping_planes(pf, ctx, pair):
    p, s = ctx.pool, pair
    pl = dict(d_l=p.plane(s.L, 0), d_r=p.plane(s.R, 0), d_blend=p.plane(s.blend, 0), g0=p.plane(s.g0, 0), g1=p.plane(s.g1, 0),
              d_out=p.out(N * 4, 0), f0=p.out(N * 8, 0), f1=p.out(N * 8, 0))
    a4 = dict(d_l=4, d_r=4, d_blend=4, d_out=4)
    # pf_flow_bidir_dev
    planes = dict(d_l=pl["d_l"], d_r=pl["d_r"], d_flow_l2r=pl["f0"], d_flow_r2l=pl["f1"])
    _solver_form_refusals(pf, ctx, list(planes), dict(d_l=4, d_r=4, d_flow_l2r=8, d_flow_r2l=8), ["d_flow_l2r", "d_flow_r2l"],
                          lambda b: lambda: ctx.flow_bidir_dev(b["d_l"], b["d_r"], COLS, ROWS, PCT, b["d_flow_l2r"], b["d_flow_r2l"]), planes)
    # pf_blend_dev: the flows are inputs
    planes = dict(d_l=pl["d_l"], d_r=pl["d_r"], d_flow_l2r=pl["g0"], d_flow_r2l=pl["g1"], d_blend=pl["d_blend"], d_out=pl["d_out"])
    _solver_form_refusals(pf, ctx, list(planes), dict(a4, d_flow_l2r=8, d_flow_r2l=8), ["d_out"],
                          lambda b: lambda: ctx.blend_dev(b["d_l"], b["d_r"], b["d_flow_l2r"], b["d_flow_r2l"], b["d_blend"], COLS, ROWS, b["d_out"]), planes)
    # pf_novel_view_dev
    planes = dict(d_l=pl["d_l"], d_r=pl["d_r"], d_blend=pl["d_blend"], d_out=pl["d_out"], d_flow_l2r=pl["f0"], d_flow_r2l=pl["f1"])
    _solver_form_refusals(pf, ctx, list(planes), dict(a4, d_flow_l2r=8, d_flow_r2l=8), ["d_out", "d_flow_l2r", "d_flow_r2l"],
                          lambda b: lambda: ctx.novel_view_dev(b["d_l"], b["d_r"], COLS, ROWS, PCT, b["d_blend"], b["d_out"], b["d_flow_l2r"], b["d_flow_r2l"]), planes)
    # after all of them the forms still work on these very planes
    ctx.novel_view_dev(pl["d_l"].ptr, pl["d_r"].ptr, COLS, ROWS, PCT, pl["d_blend"].ptr, pl["d_out"].ptr, pl["f0"].ptr, pl["f1"].ptr)
    _same(pl["d_out"].get(IMG, np.uint8), s.view, "pf_novel_view_dev after the refusals vs the oracle")


def test_novel_view_batch_dev_refuses_across_its_pairs(pf, ctx, pair):
    p, s = ctx.pool, pair
    d = [dict(l=p.plane(s.L, 0), r=p.plane(s.R, 0), b=p.plane(s.blend, 0), o=p.out(N * 4, 0), f0=p.out(N * 8, 0), f1=p.out(N * 8, 0)) for _ in range(3)]
    outs = [x[k] for x in d for k in ("o", "f0", "f1")]

    def call(edit):
        cols = {k: [x[k].ptr for x in d] for k in ("l", "r", "b", "o", "f0", "f1")}
        edit(cols)
        return lambda: ctx.novel_view_batch_dev(cols["l"], cols["r"], COLS, ROWS, PCT, cols["b"], cols["o"], cols["f0"], cols["f1"], in_flight=2)

    def put(k, i, v):
        def edit(cols):
            cols[k][i] = v(cols)
        return edit
    for k, i, delta, words in (("l", 1, 1, "d_l 1 is not 4-byte aligned"), ("r", 2, 2, "d_r 2 is not 4-byte aligned"), ("b", 0, 3, "d_blend 0 is not 4-byte aligned"),
                               ("o", 2, 1, "d_out 2 is not 4-byte aligned"), ("f0", 0, 4, "d_flow_l2r 0 is not 8-byte aligned"), ("f1", 1, 4, "d_flow_r2l 1 is not 8-byte aligned")):
        _refused(pf, ctx, call(put(k, i, lambda cols, k=k, i=i, delta=delta: cols[k][i] + delta)), outs, words)
    # 32 bytes into a plane of its own size, an output stays inside that plane's allocation: the pair the refusal names is the one meant
    for k, i, src, j, words in (("o", 1, "l", 0, "d_out 1 overlaps d_l 0"), ("o", 0, "o", 2, "d_out 0 overlaps d_out 2"), ("f1", 1, "f0", 1, "d_flow_l2r 1 overlaps d_flow_r2l 1"),
                                ("f0", 2, "f1", 0, "d_flow_r2l 0 overlaps d_flow_l2r 2"), ("o", 2, "b", 0, "d_out 2 overlaps d_blend 0"), ("o", 2, "r", 2, "d_out 2 overlaps d_r 2")):
        _refused(pf, ctx, call(put(k, i, lambda cols, src=src, j=j: cols[src][j] + 32)), outs, words)


def test_stitch_rig_and_panel_device_forms_refuse_planes_below_4_bytes(pf, ctx, stitch):
    p, s = ctx.pool, stitch
    L, R, o = [p.plane(s.L, 0) for _ in range(2)], [p.plane(s.R, 0) for _ in range(2)], [p.out(NB, 0) for _ in range(2)]
    plan = ctx.stitch_plan(s.L, s.R)
    ptr = lambda v: [x.ptr for x in v]
    for pl in (None, plan):
        for which, delta in ((0, 1), (1, 2), (2, 3)):
            a = [ptr(L), ptr(R), ptr(o)]
            a[which][1] += delta
            _refused(pf, ctx, lambda: ctx.stitch_step_batch_dev(a[0], a[1], SC, SR, PCT, a[2], in_flight=2, plan=pl), o, "is not 4-byte aligned")
    _refused(pf, ctx, lambda: ctx.stitch_plan_dev(L[0].ptr + 2, R[0].ptr, SC, SR), o, "is not 4-byte aligned")
    _refused(pf, ctx, lambda: ctx.stitch_plan_dev(L[0].ptr, R[0].ptr + 1, SC, SR), o, "is not 4-byte aligned")
    top, ls = p.plane(s.top, 0), [p.plane(x, 0) for x in s.Ls]
    _refused(pf, ctx, lambda: ctx.rig_plan_dev(top.ptr + 1, ptr(ls), SC, SR), o, "is not 4-byte aligned")
    _refused(pf, ctx, lambda: ctx.rig_plan_dev(top.ptr, [ls[0].ptr, ls[1].ptr + 2, ls[2].ptr], SC, SR), o, "is not 4-byte aligned")
    rig = ctx.rig_plan_dev(top.ptr, ptr(ls), SC, SR)
    ro = [p.out(NB, 0) for _ in range(3)]
    _refused(pf, ctx, lambda: ctx.rig_stitch_batch_dev(rig, [top.ptr + 3], [ptr(ls)], PCT, [ptr(ro)], in_flight=1), ro, "is not 4-byte aligned")
    _refused(pf, ctx, lambda: ctx.rig_stitch_batch_dev(rig, [top.ptr], [[ls[0].ptr, ls[1].ptr, ls[2].ptr + 1]], PCT, [ptr(ro)], in_flight=1), ro, "is not 4-byte aligned")
    _refused(pf, ctx, lambda: ctx.rig_stitch_batch_dev(rig, [top.ptr], [ptr(ls)], PCT, [[ro[0].ptr, ro[1].ptr + 2, ro[2].ptr]], in_flight=1), ro, "is not 4-byte aligned")
    # the panel: flow 8, image and panel 4, the panel inside neither input
    flow = p.plane(np.zeros((SR, SC, 2), np.float32), 0)
    po = p.out(NB * 3, 0)
    for f, im, out, words in ((4, 0, 0, "d_flow is not 8-byte aligned"), (0, 1, 0, "d_image is not 4-byte aligned"), (0, 0, 2, "d_out is not 4-byte aligned")):
        _refused(pf, ctx, lambda: ctx.vis_panel_dev(flow.ptr + f, L[0].ptr + im, SC, SR, po.ptr + out), [po], words)
    _refused(pf, ctx, lambda: ctx.vis_panel_dev(flow.ptr, L[0].ptr, SC, SR, flow.ptr + 16), [po], "d_out overlaps d_flow")
    _refused(pf, ctx, lambda: ctx.vis_panel_dev(flow.ptr, L[0].ptr, SC, SR, L[0].ptr), [po], "d_out overlaps d_image")
