"""Stitch plans (pf_stitch_plan_*, pf_stitch_step_planned, pf_stitch_step_batch_planned*): a plan holds what the oracle's
stitch_prepare derives from the masks, a planned step gives the bytes of the unplanned one, and a frame whose masks are not the
plan's fails the call.  Seed A makes the plans; seeds B..E are the frames."""
import ctypes as C

import numpy as np
import pytest

PCT = 20   # pixflow_search_20
COLS, ROWS = 523, 261   # odd both ways: rows no multiple of 4 or 64, pixels no multiple of 4 (the verifying match's scalar tail runs)
SEED_A, SEEDS = 1234, (1235, 1236, 1237, 1238)
RAMP_FAMILIES = ("countblend", "tile_blur", "box_blur")


def _ndiff(a, b):
    return int((a != b).sum())


def _rig(synth, cols, rows, seed, n=5):
    top, imgs = synth.make_stitch_set(cols, rows, seed, n)
    return top.numpy(), [im.numpy() for im in imgs]


def _chain(c, top, imgs, plans=None, planned_steps=range(5)):
    outs = []
    for i, L in enumerate(imgs):
        plan = plans[i] if plans is not None and i in planned_steps else None
        outs.append(c.stitch_step(L, top if i == 0 else None, PCT, plan=plan))
    return outs


@pytest.fixture(scope="module")
def rig_a(synth, pf):
    return _rig(synth, COLS, ROWS, SEED_A)


@pytest.fixture(scope="module")
def rigs(synth, pf):
    return [_rig(synth, COLS, ROWS, s) for s in SEEDS]


@pytest.fixture(scope="module")
def chain_a(pf, rig_a):
    c = pf.Context(0)
    ref = _chain(c, *rig_a)
    c.close()
    return ref


@pytest.fixture(scope="module")
def chains(pf, rigs):
    """the unplanned pf_stitch_step chains of seeds B..E: the reference of every planned result below"""
    c = pf.Context(0)
    ref = [_chain(c, top, imgs) for top, imgs in rigs]
    c.close()
    return ref


def _plans(c, rig_a, chain_a, steps=5):
    top, imgs = rig_a
    return [c.stitch_plan(imgs[i], top if i == 0 else chain_a[i - 1]) for i in range(steps)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["240x200", "523x261"])
def test_plan_equals_oracle_prepare(pf, orc, synth, rig_a, size):
    if size == "240x200":
        L, R = (t.numpy() for t in synth.make_canvas_pair(240, 200))
    else:
        L, R = rig_a[1][0], rig_a[0]
    rows, cols = L.shape[:2]
    mp, _, _, blend, _ = orc.stitch_prepare(L, R, True)
    c = pf.Context(0)
    plan = c.stitch_plan(L, R)
    assert (plan.cols, plan.rows) == (cols, rows)
    assert plan.overlap_px == int((mp == 150).sum()) and plan.overlap_px > 0
    got_mp, got_blend = plan.download()
    assert np.array_equal(got_mp, mp), "%d map codes differ from the oracle's" % _ndiff(got_mp, mp)
    assert np.array_equal(got_blend.view(np.uint32), blend.view(np.uint32)), "%d ramp values differ from the oracle's" % _ndiff(got_blend, blend)
    # the device form makes the same plan
    nb = cols * rows * 4
    dl, dr = c.dev_alloc(nb), c.dev_alloc(nb)
    c.upload(dl, L); c.upload(dr, R)
    plan2 = c.stitch_plan_dev(dl, dr, cols, rows)
    mp2, blend2 = plan2.download()
    assert plan2.overlap_px == plan.overlap_px and np.array_equal(mp2, mp) and np.array_equal(blend2.view(np.uint32), blend.view(np.uint32))
    c.dev_free(dl); c.dev_free(dr)
    plan.close(); plan2.close()
    c.close()


@pytest.mark.gpu
def test_planned_chain_equals_unplanned(pf, orc, rig_a, chain_a, rigs, chains):
    top, imgs = rigs[0]
    ref = chains[0]
    c = pf.Context(0)
    plans = _plans(c, rig_a, chain_a)
    # all five steps planned, with the next left image announced: the prefetch is honoured and changes nothing
    outs = []
    for i, L in enumerate(imgs):
        if i + 1 < len(imgs):
            c.stitch_prefetch(imgs[i + 1])
        outs.append(c.stitch_step(L, top if i == 0 else None, PCT, plan=plans[i]))
    for i in range(5):
        assert np.array_equal(outs[i], ref[i]), "planned step %d: %d bytes differ from pf_stitch_step's" % (i + 1, _ndiff(outs[i], ref[i]))
    panels = c.stitch_visualize()
    c.stitch_step(imgs[4], ref[3], PCT)
    want = c.stitch_visualize()
    assert np.array_equal(panels[0], want[0]) and np.array_equal(panels[1], want[1]), "the visualiser's panels after a planned step differ"
    # steps 1, 3, 5 planned and 2, 4 unplanned share one chain state
    mixed = _chain(c, top, imgs, plans, planned_steps=(0, 2, 4))
    for i in range(5):
        assert np.array_equal(mixed[i], ref[i]), "mixed chain step %d: %d bytes differ" % (i + 1, _ndiff(mixed[i], ref[i]))
    # a plan made from the chained composite in HBM (r = NULL) is the plan made from its host copy
    c.stitch_step(rig_a[1][0], rig_a[0], PCT, want_out=False)
    p2 = c.stitch_plan(rig_a[1][1], None)
    a, b = p2.download(), plans[1].download()
    assert p2.overlap_px == plans[1].overlap_px and np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    c.close()
    # step 1 of seed B against the oracle's composite
    L, R = imgs[0], top
    mp, ovl, ovr, blend, _ = orc.stitch_prepare(L, R, True)
    f0, f1 = orc.flow_bidir(ovl, ovr, PCT)
    want = orc.stitch_gather(L, R, orc.combine_novel_views(ovl, ovr, f0, f1, blend), mp)
    assert np.array_equal(outs[0], want), "planned step 1: %d bytes differ from the oracle chain" % _ndiff(outs[0], want)


@pytest.mark.gpu
def test_planned_step_with_active_smoothing(pf, synth):
    """1003x800: step 4, tile window rows/130 = 6 and box blur rows/400 = 2, so the plan's ramp went through tiles that do work and
    through the box blur.  GPU against GPU, no oracle.
    The streamed form of the tile smoothing cannot be had at a size a test may use: plan creation takes ramp_geom()'s form, as
    pf_stitch_step does, and that is the streamed one only where the tile window exceeds the 160 KiB of LDS (canvases beyond
    24000x12000); forcing a form is pf_stage_tile_blur's business (tests/test_gpu_tile_blur_streamed.py), not an argument of a plan."""
    cols, rows = 1003, 800
    top_a, imgs_a = _rig(synth, cols, rows, SEED_A, 1)
    top_b, imgs_b = _rig(synth, cols, rows, SEEDS[0], 1)
    c = pf.Context(0)
    plan = c.stitch_plan(imgs_a[0], top_a)
    _, ramp = plan.download()
    raw, md = c.stitch_raw_blend(imgs_a[0], top_a)
    step = min(cols, rows) // 200
    assert int((md[0:rows - step:step, 0:cols - step:step] > step).sum()) >= 100, "too few active tiles for the case to mean anything"
    assert not np.array_equal(ramp, raw), "the smoothing changed nothing"
    want = c.stitch_step(imgs_b[0], top_b, PCT)
    got = c.stitch_step(imgs_b[0], top_b, PCT, plan=plan)
    assert np.array_equal(got, want), "%d bytes differ" % _ndiff(got, want)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("in_flight", [1, 3, 4])
def test_planned_batches(pf, rig_a, chain_a, rigs, chains, in_flight):
    c = pf.Context(0)
    plans = _plans(c, rig_a, chain_a, 2)
    tops = [top for top, _ in rigs]
    # host form: two chained calls, the second on the slots the first left
    for i in range(2):
        outs = c.stitch_step_batch([imgs[i] for _, imgs in rigs], tops if i == 0 else None, PCT, in_flight=in_flight, plan=plans[i])
        for k in range(4):
            assert np.array_equal(outs[k], chains[k][i]), "host form, frame %d step %d: %d bytes differ" % (k, i + 1, _ndiff(outs[k], chains[k][i]))
    # the planned and the unplanned host form share the slots: an unplanned step 2 after a planned step 1
    c.stitch_step_batch([imgs[0] for _, imgs in rigs], tops, PCT, in_flight=in_flight, plan=plans[0], want_out=False)
    outs = c.stitch_step_batch([imgs[1] for _, imgs in rigs], None, PCT, in_flight=in_flight)
    for k in range(4):
        assert np.array_equal(outs[k], chains[k][1]), "unplanned step 2 after a planned step 1, frame %d: %d bytes differ" % (k, _ndiff(outs[k], chains[k][1]))
    # device form
    nb = COLS * ROWS * 4
    bufs = [c.dev_alloc(nb) for _ in range(12)]
    try:
        dl, dr, dout = bufs[0:4], bufs[4:8], bufs[8:12]
        for k, (top, imgs) in enumerate(rigs):
            c.upload(dl[k], imgs[0]); c.upload(dr[k], top)
        c.stitch_step_batch_dev(dl, dr, COLS, ROWS, PCT, dout, in_flight=in_flight, plan=plans[0])
        for k in range(4):
            got = c.download(np.empty((ROWS, COLS, 4), np.uint8), dout[k])
            assert np.array_equal(got, chains[k][0]), "device form, frame %d: %d bytes differ" % (k, _ndiff(got, chains[k][0]))
    finally:
        for p in bufs:
            c.dev_free(p)
        c.close()


@pytest.mark.gpu
def test_planned_batch_throughput_sweep_form(pf, rig_a, chain_a, rigs, chains):
    c = pf.Context(0, sweep_wide=2)
    plan = _plans(c, rig_a, chain_a, 1)[0]
    outs = c.stitch_step_batch([imgs[0] for _, imgs in rigs], [top for top, _ in rigs], PCT, in_flight=4, plan=plan)
    for k in range(4):
        assert np.array_equal(outs[k], chains[k][0]), "sweep_wide 2, frame %d: %d bytes differ" % (k, _ndiff(outs[k], chains[k][0]))
    c.close()


def _changed(L, R, where, change):
    """copies of (L, R) with ONE pixel's alpha changed in whichever image has the starting alpha there"""
    rows, cols = L.shape[:2]
    y, x = {"first": (0, 0), "last": (rows - 1, cols - 1), "inner": (rows // 2 + 3, cols // 10 + 1)}[where]
    src, dst = change
    L, R = L.copy(), R.copy()
    img = L if L[y, x, 3] == src else R
    assert img[y, x, 3] == src, "neither image has alpha %d at %s" % (src, where)
    img[y, x, 3] = dst
    return L, R


@pytest.mark.gpu
@pytest.mark.parametrize("change", [(255, 0), (0, 255), (0, 1)], ids=["255to0", "0to255", "0to1"])
@pytest.mark.parametrize("where,frame", [("inner", 1), ("first", 0), ("last", 2)])
def test_frame_off_the_plan_fails_the_call(pf, rig_a, chain_a, rigs, chains, where, frame, change):
    c = pf.Context(0)
    plan = _plans(c, rig_a, chain_a, 1)[0]
    Ls = [imgs[0] for _, imgs in rigs[:3]]
    Rs = [top for top, _ in rigs[:3]]
    c.stitch_step_batch(Ls, Rs, PCT, in_flight=3, plan=plan, want_out=False)   # something to chain on
    Ls[frame], Rs[frame] = _changed(Ls[frame], Rs[frame], where, change)
    outs = [np.full((ROWS, COLS, 4), 7, np.uint8) for _ in range(3)]
    with pytest.raises(pf.PanoflowError, match=r"error -1: .*frame %d differs from the stitch plan in 1 pixels" % frame):
        c.stitch_step_batch(Ls, Rs, PCT, in_flight=3, plan=plan, out=outs)
    assert all((o == 7).all() for o in outs), "a failed call delivered a composite"
    with pytest.raises(pf.PanoflowError, match="error -1: .*chain"):
        c.stitch_step_batch([imgs[1] for _, imgs in rigs[:3]], None, PCT, in_flight=3)
    # the lone step: the same refusal, and nothing left to chain on
    c.stitch_step(rigs[0][1][0], rigs[0][0], PCT, want_out=False)
    out = np.full((ROWS, COLS, 4), 7, np.uint8)
    with pytest.raises(pf.PanoflowError, match=r"error -1: .*frame 0 differs from the stitch plan in 1 pixels"):
        c.stitch_step(Ls[frame], Rs[frame], PCT, plan=plan, out=out)
    assert (out == 7).all()
    with pytest.raises(pf.PanoflowError, match="error -1: .*chain"):
        c.stitch_step(rigs[0][1][1], None, PCT)
    # a later unchained call works, lone and batched
    got = c.stitch_step(rigs[0][1][0], rigs[0][0], PCT, plan=plan)
    assert np.array_equal(got, chains[0][0])
    outs = c.stitch_step_batch([imgs[0] for _, imgs in rigs[:3]], [top for top, _ in rigs[:3]], PCT, in_flight=3, plan=plan)
    for k in range(3):
        assert np.array_equal(outs[k], chains[k][0])
    c.close()


@pytest.mark.gpu
def test_device_form_off_the_plan_clears_its_outputs(pf, rig_a, chain_a, rigs):
    c = pf.Context(0)
    plan = _plans(c, rig_a, chain_a, 1)[0]
    nb = COLS * ROWS * 4
    bufs = [c.dev_alloc(nb) for _ in range(6)]
    try:
        dl, dr, dout = bufs[0:2], bufs[2:4], bufs[4:6]
        for k in range(2):
            L, R = rigs[k][1][0], rigs[k][0]
            if k == 1:
                L, R = _changed(L, R, "inner", (255, 0))
            c.upload(dl[k], L); c.upload(dr[k], R)
            c.upload(dout[k], np.full((ROWS, COLS, 4), 7, np.uint8))
        with pytest.raises(pf.PanoflowError, match=r"error -1: .*frame 1 differs from the stitch plan in 1 pixels"):
            c.stitch_step_batch_dev(dl, dr, COLS, ROWS, PCT, dout, in_flight=2, plan=plan)
        for k in range(2):
            assert not c.download(np.empty((ROWS, COLS, 4), np.uint8), dout[k]).any(), "frame %d: a failed call left a composite" % k
    finally:
        for p in bufs:
            c.dev_free(p)
        c.close()


@pytest.mark.gpu
def test_alpha_255_to_1_is_on_the_plan(pf, rig_a, chain_a, rigs):
    top, imgs = rigs[1]
    L = imgs[0].copy()
    ys, xs = np.nonzero(L[..., 3] == 255)
    pick = np.random.RandomState(5).choice(len(ys), 1000, replace=False)
    L[ys[pick], xs[pick], 3] = 1
    c = pf.Context(0)
    plan = _plans(c, rig_a, chain_a, 1)[0]
    want = c.stitch_step(L, top, PCT)
    got = c.stitch_step(L, top, PCT, plan=plan)
    assert np.array_equal(got, want), "%d bytes differ" % _ndiff(got, want)
    assert not np.array_equal(want, c.stitch_step(imgs[0], top, PCT)), "the changed alphas changed nothing: the case checks nothing"
    c.close()


@pytest.mark.gpu
def test_plans_that_are_refused(pf, synth, rig_a, chain_a, rigs):
    top, imgs = rigs[0]
    c = pf.Context(0); other = pf.Context(0)
    plan = _plans(c, rig_a, chain_a, 1)[0]
    small = c.stitch_plan(*[t.numpy() for t in synth.make_canvas_pair(240, 200)])
    foreign = _plans(other, rig_a, chain_a, 1)[0]
    nb = COLS * ROWS * 4
    d = [c.dev_alloc(nb) for _ in range(3)]
    for bad, msg in ((small, "the plan is 240x200"), (foreign, "not a live stitch plan")):
        with pytest.raises(pf.PanoflowError, match="error -1: .*" + msg):
            c.stitch_step(imgs[0], top, PCT, plan=bad)
        with pytest.raises(pf.PanoflowError, match="error -1: .*" + msg):
            c.stitch_step_batch([imgs[0]], [top], PCT, plan=bad)
        with pytest.raises(pf.PanoflowError, match="error -1: .*" + msg):
            c.stitch_step_batch_dev(d[:1], d[1:2], COLS, ROWS, PCT, d[2:3], plan=bad)
    with pytest.raises(pf.PanoflowError, match="not a live stitch plan"):
        foreign.ctx = c
        foreign.download()
    foreign.ctx = other
    # a destroyed plan: the handle is looked up in the context's list, never dereferenced
    h = plan.h
    plan.close()
    sz = C.c_size_t(COLS * 4)
    out = np.empty((ROWS, COLS, 4), np.uint8)
    assert c.l.pf_stitch_step_planned(c.h, h, imgs[0].ctypes.data_as(C.c_void_p), top.ctypes.data_as(C.c_void_p), COLS, ROWS, sz, PCT,
                                      out.ctypes.data_as(C.c_void_p), sz) == -1
    assert c.l.pf_stitch_plan_destroy(c.h, h) == -1
    assert c.l.pf_stitch_step_planned(c.h, None, imgs[0].ctypes.data_as(C.c_void_p), top.ctypes.data_as(C.c_void_p), COLS, ROWS, sz, PCT,
                                      out.ctypes.data_as(C.c_void_p), sz) == -1
    # creation refuses what pf_stitch_step refuses
    with pytest.raises(pf.PanoflowError, match="error -1"):
        c.stitch_plan(np.zeros((1, 1, 4), np.uint8), np.zeros((1, 1, 4), np.uint8))
    fresh = pf.Context(0)
    with pytest.raises(pf.PanoflowError, match="error -1: .*no previous result"):
        fresh.stitch_plan(imgs[0], None)
    for p in d:
        c.dev_free(p)
    fresh.close(); other.close(); c.close()


@pytest.mark.gpu
def test_planned_batch_launches_no_ramp_kernels(pf, synth):
    """400x820: countblend, the tile pass (step 2, window 6) and the box blur (window 2) all run in an unplanned step"""
    cols, rows = 400, 820
    top_a, imgs_a = _rig(synth, cols, rows, SEED_A, 1)
    frames = [_rig(synth, cols, rows, s, 1) for s in SEEDS[:2]]
    Ls, Rs = [imgs[0] for _, imgs in frames], [top for top, _ in frames]
    c = pf.Context(0)
    plan = c.stitch_plan(imgs_a[0], top_a)
    c.profile_enable(1)
    c.profile_reset()
    want = c.stitch_step_batch(Ls, Rs, PCT, in_flight=2)
    prof = c.profile()
    for fam in RAMP_FAMILIES:
        assert prof.get(fam, (0.0, 0))[1] > 0, "the unplanned batch reports no %s launch: %r" % (fam, sorted(prof))
    c.profile_reset()
    got = c.stitch_step_batch(Ls, Rs, PCT, in_flight=2, plan=plan)
    prof = c.profile()
    for fam in RAMP_FAMILIES:
        assert prof.get(fam, (0.0, 0))[1] == 0, "the planned batch launched %s: %r" % (fam, prof[fam])
    assert prof.get("match_images", (0.0, 0))[1] == 0 and prof["match_verify"][1] == 1 and prof["blend"][1] == 1 and prof["gather"][1] == 1
    for k in range(2):
        assert np.array_equal(got[k], want[k]), "frame %d: %d bytes differ" % (k, _ndiff(got[k], want[k]))
    c.close()
