"""pf_set_solver_params across its accepted range (include/panoflow.h: "bit-identical to the reference's arithmetic for every accepted set"):
the cases of tests/solver_param_cases.py through the HIP path against the oracle, bit for bit on view(np.uint32).  tests/test_solver_param_cases.py
holds the cases themselves to what they claim (level counts, finite results, pixels on both sides of the range guard) with the oracle alone.

  1. the fast gradient step (one fused multiply-add) at the ends of its power-of-two window, 2^-16 and 2^16; just outside it (2^-17, 2^17,
     49152 = 1.5 * 2^15), where every step takes the IEEE sequence; step sizes 0 and 2^-140 (a denormal)
  2. the sweep's range guard under coefficients that move the operands across 2^-95 and the energies across 2^99 from pixel to pixel
  3. level counts the 0.9 pyramid never produces: 1, 2 (4x upsample), 3, 77, 96; 10 and 11 on either side of the fine / coarse split; 97 refused
  4. 0.98f: the reference's pyramid does not end there (1000 levels), so every solve refuses it; the float below matches the oracle
  5. coefficients that overflow every energy: element classes (finite, +inf, -inf, NaN) as the oracle's, finite elements bit for bit"""
import numpy as np
import pytest

import solver_param_cases as sp

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what=""):
    g, w = bits(got), bits(want)
    assert np.array_equal(g, w), "%s: %d of %d elements differ" % (what, int((g != w).sum()), w.size)


@pytest.fixture(scope="module")
def ctxs(pf):
    """One context per sweep form, made on first use: the latency form, the throughput form, and the lab build's independent v1 kernel."""
    made = {}

    def get(form):
        if form not in made:
            made[form] = pf.Context(0, **sp.SWEEP_FORMS[form])
        return made[form]
    get.made = made
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(autouse=True)
def presets_again(ctxs, orc):
    yield
    orc.reset_params()
    for c in ctxs.made.values():
        c.set_solver_params()


_want = {}


def oracle_flows(orc, synth, key, cols, rows, max_pct, pset):
    """The oracle's two flows of a whole-solve case, computed once per module run; the oracle is left with the presets."""
    if key not in _want:
        L, R, _ = synth.make_pair_np(cols, rows, sp.SEED)
        orc.set_params(*pset)
        _want[key] = orc.flow_bidir(L, R, max_pct)
        orc.reset_params()
    return _want[key]


def solve_and_compare(ctx, orc, synth, name, case):
    cols, rows, max_pct, pset, _ = case
    want = oracle_flows(orc, synth, name, cols, rows, max_pct, pset)
    L, R, blend = synth.make_pair_np(cols, rows, sp.SEED)
    ctx.set_solver_params(**sp.kw(pset))
    got = ctx.flow_bidir(L, R, max_pct)
    same(got[0], want[0], name + " flowLtoR"); same(got[1], want[1], name + " flowRtoL")
    return L, R, blend, want


# ---- 1. the step window ----
@pytest.mark.parametrize("name", list(sp.STEP_CASES))
def test_step_window_whole_solves(ctxs, orc, synth, name):
    solve_and_compare(ctxs("latency"), orc, synth, name, sp.STEP_CASES[name])


@pytest.mark.parametrize("form", list(sp.SWEEP_FORMS))
@pytest.mark.parametrize("name", list(sp.LEVEL_STEP_SETS))
def test_step_window_one_level_in_every_sweep_form(ctxs, orc, synth, name, form):
    """One level (blurred flow, two sweeps, two medians, diffusion) on explicit planes at both ends of the window, where the fast form's
    product is exact, and at 49152, where it is not and the guard must send every step through the IEEE sequence."""
    planes = sp.level_planes(orc, synth)
    pset = sp.LEVEL_STEP_SETS[name]
    orc.set_params(*pset)
    want = orc.level(*planes, 0, 0)
    c = ctxs(form)
    c.set_solver_params(**sp.kw(pset))
    same(c.stage_level(*planes, 0, 0), want, "%s %s" % (name, form))


# ---- 2. the range guard under coefficients ----
@pytest.mark.parametrize("form", list(sp.SWEEP_FORMS))
@pytest.mark.parametrize("w,h", sp.GUARD_SIZES)
@pytest.mark.parametrize("name", list(sp.GUARD_SETS))
def test_range_guard_under_coefficients_one_sweep(ctxs, orc, name, w, h, form):
    """Ordinary flows, nothing planted: the coefficient alone puts a regulariser operand below 2^-95 at one gated pixel in eight (straddle), or
    the energy above 2^99 at one in nine (large), so fast and IEEE steps alternate inside the sweep.  Both band orientations, forward and backward."""
    g0, g1, blurred, a0, a1, flow = sp.sweep_planes(orc, w, h)
    pset = sp.GUARD_SETS[name]
    orc.set_params(*pset)
    c = ctxs(form)
    c.set_solver_params(**sp.kw(pset))
    for fwd in (1, 0):
        want = orc.sweep(g0[..., 0], g0[..., 1], g1[..., 0], g1[..., 1], blurred, a0, a1, flow, fwd)
        assert np.isfinite(want).all()
        same(c.stage_sweep(g0, g1, blurred, a0, a1, flow, fwd), want, "%s %dx%d %s forward %d" % (name, w, h, form, fwd))


@pytest.mark.parametrize("name", list(sp.COEF_CASES))
def test_range_guard_under_coefficients_whole_solves(ctxs, orc, synth, name):
    solve_and_compare(ctxs("latency"), orc, synth, name, sp.COEF_CASES[name])


# ---- 3. level counts ----
@pytest.mark.parametrize("name", list(sp.LEVEL_CASES))
def test_level_counts_whole_solves(ctxs, orc, synth, name):
    """The solve's orchestration by level count: no upsample at all (1), a 4x upsample on the path without a fine / coarse split (2), 3, the two
    counts on either side of the split (10: every gradient in one launch; 11: three launches and both event waits), 77, and a full level table (96)."""
    ctx = ctxs("latency")
    case = sp.LEVEL_CASES[name]
    L, R, blend, want = solve_and_compare(ctx, orc, synth, name, case)
    cols, rows, max_pct, pset, _ = case
    if name == "levels_2":
        out, f0, f1 = ctx.novel_view(L, R, max_pct, blend)
        same(f0, want[0], "novel_view flowLtoR"); same(f1, want[1], "novel_view flowRtoL")
        assert np.array_equal(out, orc.combine_novel_views(L, R, want[0], want[1], blend))
    if name == "levels_3":
        orc.set_params(*pset)
        same(ctx.flow(L, R, max_pct, 3), orc.compute_optical_flow(L, R, max_pct, 3), "one direction with a hint")


def _refused(pf, call, levels):
    with pytest.raises(pf.PanoflowError) as ei:
        call()
    text = str(ei.value)
    assert "error -1:" in text and "%d pyramid levels" % levels in text, text      # PF_ERR_ARG, naming the count
    return text


@pytest.mark.parametrize("name", list(sp.REFUSED_CASES))
def test_more_than_96_levels_are_refused_lone_and_batched(pf, ctxs, orc, synth, name):
    """97 levels (0.975 on 606x566) and the 1000 of 0.98f, where a side of 25 no longer shrinks and the reference goes on to its level limit:
    PF_ERR_ARG naming the count, from the lone solve and -- before any lane exists or any plane is touched -- from the batched entry point; the
    context then solves the presets' pair to the presets' bits, and the largest usable scale on the same pair to the oracle's."""
    ctx = ctxs("throughput")
    cols, rows, max_pct, pset, levels = sp.REFUSED_CASES[name]
    L, R, blend = synth.make_pair_np(cols, rows, sp.SEED)
    ctx.set_solver_params(**sp.kw(pset))
    _refused(pf, lambda: ctx.flow_bidir(L, R, max_pct), levels)
    _refused(pf, lambda: ctx.novel_view(L, R, max_pct, blend), levels)
    n = cols * rows
    fill = np.full((rows, cols, 4), 0xA5, np.uint8)
    d = {k: ctx.dev_alloc(n * 4) for k in ("L", "R", "b", "o0", "o1")}
    ctx.upload(d["L"], L); ctx.upload(d["R"], R); ctx.upload(d["b"], blend); ctx.upload(d["o0"], fill); ctx.upload(d["o1"], fill)
    text = _refused(pf, lambda: ctx.novel_view_batch_dev([d["L"]] * 2, [d["R"]] * 2, cols, rows, max_pct, [d["b"]] * 2, [d["o0"], d["o1"]], in_flight=2), levels)
    assert "lane" not in text, text                                                # refused by the entry point, not by a lane's solve
    for k in ("o0", "o1"):
        assert np.array_equal(ctx.download(np.empty_like(fill), d[k]), fill)
    for p in d.values():
        ctx.dev_free(p)
    ctx.set_solver_params()
    orc.reset_params()
    same_pair = oracle_flows(orc, synth, "presets_%dx%d" % (cols, rows), cols, rows, max_pct, sp.PRESETS)
    got = ctx.flow_bidir(L, R, max_pct)
    same(got[0], same_pair[0], "presets after the refusal"); same(got[1], same_pair[1], "presets after the refusal")
    if name == "levels_1000":
        solve_and_compare(ctx, orc, synth, "below_098_200x160", (cols, rows, max_pct, sp.pyr(sp.PYR_BELOW_098), 53))


@pytest.mark.parametrize("scale", [0.25, 0.97])
def test_pyramid_scales_in_the_throughput_form_and_in_batches(pf, orc, synth, scale):
    """Three pairs of 420x360 through the batch entry point, every sweep launch in the throughput form: 2 levels with a 4x upsample, and 67 levels
    (the lanes fuse the upsample into the next level's Gaussian on small levels: k_gauss15_fused with the context's ratio, not 1 / 0.9)."""
    cols, rows, mp = 420, 360, 0
    pset = sp.pyr(scale)
    pairs = [synth.make_pair_np(cols, rows, 500 + i) for i in range(3)]
    orc.set_params(*pset)
    want = []
    for L, R, blend in pairs:
        f0, f1 = orc.flow_bidir(L, R, mp)
        want.append((f0, f1, orc.combine_novel_views(L, R, f0, f1, blend)))
    c = pf.Context(0, sweep_wide=2)
    try:
        c.set_solver_params(**sp.kw(pset))
        n = cols * rows
        d = [{"L": c.dev_alloc(n * 4), "R": c.dev_alloc(n * 4), "b": c.dev_alloc(n * 4), "o": c.dev_alloc(n * 4), "f0": c.dev_alloc(n * 8), "f1": c.dev_alloc(n * 8)} for _ in pairs]
        for k, (L, R, blend) in zip(d, pairs):
            c.upload(k["L"], L); c.upload(k["R"], R); c.upload(k["b"], blend)
        for in_flight in (3, 1):
            c.novel_view_batch_dev([k["L"] for k in d], [k["R"] for k in d], cols, rows, mp, [k["b"] for k in d], [k["o"] for k in d], [k["f0"] for k in d], [k["f1"] for k in d], in_flight=in_flight)
            for i, (k, w) in enumerate(zip(d, want)):
                same(c.download(np.empty((rows, cols, 2), np.float32), k["f0"]), w[0], "in_flight %d pair %d flowLtoR" % (in_flight, i))
                same(c.download(np.empty((rows, cols, 2), np.float32), k["f1"]), w[1], "in_flight %d pair %d flowRtoL" % (in_flight, i))
                assert np.array_equal(c.download(np.empty((rows, cols, 4), np.uint8), k["o"]), w[2])
    finally:
        c.close()


def test_presized_context_regrows_its_arena_for_a_finer_pyramid(pf, orc, synth):
    """pf_create sizes the arena for max_cols x max_rows with the 0.9 geometry; at nextafter(0.98f, 0) the pyramid planes of the same image hold
    about three times the pixels (77 levels instead of 16).  The solve must regrow them -- and still give the presets' bits afterwards."""
    name = "levels_77"
    cols, rows, max_pct, pset, _ = sp.LEVEL_CASES[name]
    c = pf.Context(0, max_cols=cols, max_rows=rows)
    try:
        L, R, _, _ = solve_and_compare(c, orc, synth, name, sp.LEVEL_CASES[name])
        preset = oracle_flows(orc, synth, "presets_%dx%d" % (cols, rows), cols, rows, max_pct, sp.PRESETS)
        c.set_solver_params()
        got = c.flow_bidir(L, R, max_pct)
        same(got[0], preset[0], "presets again"); same(got[1], preset[1], "presets again")
    finally:
        c.close()


def test_one_stitch_step_under_a_non_preset_set(ctxs, orc, synth):
    """pf_stitch_step solves its overlap with the context's parameters: the reference's call sequence (prepare, both flows, the novel view,
    Gather) with the oracle, as tests/test_gpu_e2e.py composes it, under a set with another pyramid scale and step size 2^-3."""
    cols, rows = 640, 420
    L, R = synth.make_canvas_pair(cols, rows, 21)
    L, R = L.numpy(), R.numpy()
    mp, ovl, ovr, blend, _ = orc.stitch_prepare(L, R, True)
    preset = orc.stitch_gather(L, R, orc.combine_novel_views(ovl, ovr, *orc.flow_bidir(ovl, ovr, 20), blend), mp)
    orc.set_params(*sp.STITCH_SET)
    fLR, fRL = orc.flow_bidir(ovl, ovr, 20)
    final = orc.stitch_gather(L, R, orc.combine_novel_views(ovl, ovr, fLR, fRL, blend), mp)
    assert not np.array_equal(final, preset)
    ctx = ctxs("latency")
    ctx.set_solver_params(**sp.kw(sp.STITCH_SET))
    assert np.array_equal(ctx.stitch_step(L, R, 20), final)
    ctx.set_solver_params()
    assert np.array_equal(ctx.stitch_step(L, R, 20), preset)


# ---- 5. overflow ----
@pytest.mark.parametrize("form", ["latency", "throughput"])
def test_coefficients_that_overflow_every_energy(ctxs, orc, synth, form):
    """(0.9, 1e20, 1e25, 1e28, 0.5): every energy is +inf or NaN and the oracle's flow is finite nowhere.  "Bit-identical" then means: every
    element is of the oracle's class (finite, +inf, -inf, NaN), and finite elements have its bits; a NaN's sign and payload are not compared
    (they depend on which operand an instruction propagates, which IEEE 754 leaves open)."""
    cols, rows, max_pct, pset, _ = sp.OVERFLOW_CASE
    want = oracle_flows(orc, synth, "overflow", cols, rows, max_pct, pset)
    L, R, _ = synth.make_pair_np(cols, rows, sp.SEED)
    ctx = ctxs(form)
    ctx.set_solver_params(**sp.kw(pset))
    got = ctx.flow_bidir(L, R, max_pct)
    for d in range(2):
        gc, wc = sp.float_class(got[d]), sp.float_class(want[d])
        assert np.array_equal(gc, wc), "direction %d: %d elements of another class; oracle %s, got %s" % (d, int((gc != wc).sum()), np.bincount(wc.ravel(), minlength=4), np.bincount(gc.ravel(), minlength=4))
        fin = wc == 0
        assert np.array_equal(bits(got[d])[fin], bits(want[d])[fin])
