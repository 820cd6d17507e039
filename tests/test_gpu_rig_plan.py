"""Rig plans (pf_rig_plan_*): the plans of every step of a chain, made from its n + 1 input masks by one k_rig_maps pass and one grouped
blend ramp, are the oracle's stitch_prepare on the stand-in R of each step and the plans pf_stitch_plan_create makes step by step."""
import ctypes as C

import numpy as np
import pytest

from rig_cases import COLS, PCT, ROWS, SEED_A, rig, rig_codes, stand_ins, window_set


def _ndiff(a, b):
    return int((a != b).sum())


def _same_plan(got, want, what):
    """got, want: StitchPlan objects (or (map, ramp, overlap) tuples)"""
    a = got.download() + (got.overlap_px,) if hasattr(got, "download") else got
    b = want.download() + (want.overlap_px,) if hasattr(want, "download") else want
    assert np.array_equal(a[0], b[0]), "%s: %d map codes differ" % (what, _ndiff(a[0], b[0]))
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "%s: %d ramp values differ" % (what, _ndiff(a[1].view(np.uint32), b[1].view(np.uint32)))
    assert a[2] == b[2], "%s: overlap count %d, expected %d" % (what, a[2], b[2])


def _against_step_plans(c, rg, top, Ls, what):
    """every step of the rig against pf_stitch_plan_create on the step's stand-in R, and its map against the numpy restatement"""
    codes = rig_codes(top, Ls)
    for i, (L, R) in enumerate(zip(Ls, stand_ins(top, Ls))):
        want = c.stitch_plan(L, R)
        _same_plan(rg.steps[i], want, "%s, step %d" % (what, i + 1))
        assert np.array_equal(rg.steps[i].download()[0], codes[i]), "%s, step %d: the map is not the numpy restatement's" % (what, i + 1)
        want.close()


@pytest.fixture(scope="module")
def rig_a(synth):
    return rig(synth, COLS, ROWS, SEED_A)


@pytest.fixture(scope="module")
def oracle_a(orc, rig_a):
    top, imgs = rig_a
    ref = []
    for L, R in zip(imgs, stand_ins(top, imgs)):
        mp, _, _, blend, _ = orc.stitch_prepare(L, R, True)
        ref.append((mp, blend, int((mp == 150).sum())))
    return ref


@pytest.mark.gpu
def test_rig_plan_equals_oracle_and_step_plans(pf, rig_a, oracle_a):
    top, imgs = rig_a
    c = pf.Context(0)
    rg = c.rig_plan(top, imgs)
    assert (rg.n_steps, rg.cols, rg.rows) == (5, COLS, ROWS)
    for i in range(5):
        assert rg.steps[i].overlap_px > 0
        _same_plan(rg.steps[i], oracle_a[i], "step %d against the oracle" % (i + 1))
    _against_step_plans(c, rg, top, imgs, "523x261")
    rg.close()
    c.close()


@pytest.mark.gpu
def test_device_form_with_unaligned_images(pf, rig_a, oracle_a):
    """every image pointer 4 bytes into its allocation: the launch takes 4-byte image loads (vec = 0)"""
    top, imgs = rig_a
    nb = COLS * ROWS * 4
    c = pf.Context(0)
    bufs = [c.dev_alloc(nb + 16) for _ in range(6)]
    try:
        for b, im in zip(bufs, [top] + imgs):
            c.upload(b + 4, im)
        rg = c.rig_plan_dev(bufs[0] + 4, [b + 4 for b in bufs[1:]], COLS, ROWS)
        for i in range(5):
            _same_plan(rg.steps[i], oracle_a[i], "unaligned device form, step %d" % (i + 1))
        # ... and the aligned device form
        for b, im in zip(bufs, [top] + imgs):
            c.upload(b, im)
        rg2 = c.rig_plan_dev(bufs[0], bufs[1:], COLS, ROWS)
        for i in range(5):
            _same_plan(rg2.steps[i], oracle_a[i], "aligned device form, step %d" % (i + 1))
    finally:
        for b in bufs:
            c.dev_free(b)
        c.close()


@pytest.mark.gpu
def test_rig_plan_with_active_smoothing(pf, synth):
    """1003x800, 3 steps: tile window rows/130 = 6 and box blur rows/400 = 2, so the grouped ramp does real smoothing.  No solve."""
    cols, rows = 1003, 800
    top, imgs = rig(synth, cols, rows, SEED_A, 3)
    c = pf.Context(0)
    rg = c.rig_plan(top, imgs)
    raw, md = c.stitch_raw_blend(imgs[0], top)
    step = min(cols, rows) // 200
    assert int((md[0:rows - step:step, 0:cols - step:step] > step).sum()) >= 100, "too few active tiles for the case to mean anything"
    assert not np.array_equal(rg.steps[0].download()[1], raw), "the smoothing changed nothing"
    _against_step_plans(c, rg, top, imgs, "1003x800")
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_steps", [1, 16])
def test_rig_plan_of_1_and_16_steps(pf, n_steps):
    cols, rows = 240, 200
    top, Ls = window_set(cols, rows, n_steps, 99 + n_steps)
    codes = rig_codes(top, Ls)
    assert all((m == 150).any() for m in codes), "a step without overlap: the masks were not drawn as meant"
    c = pf.Context(0)
    rg = c.rig_plan(top, Ls)
    assert rg.n_steps == n_steps
    for i in range(n_steps):
        assert rg.steps[i].overlap_px == int((codes[i] == 150).sum())
    _against_step_plans(c, rg, top, Ls, "240x200 x %d" % n_steps)
    c.close()


@pytest.mark.gpu
def test_step_without_overlap_is_pf_stitch_plan_create_s(pf):
    cols, rows = 240, 200
    top, Ls = window_set(cols, rows, 4, 7, gap_step=2)
    codes = rig_codes(top, Ls)
    assert not (codes[2] == 150).any() and (codes[3] == 150).any()
    c = pf.Context(0)
    rg = c.rig_plan(top, Ls)
    assert rg.steps[2].overlap_px == 0
    _against_step_plans(c, rg, top, Ls, "a step without overlap")
    c.close()


@pytest.mark.gpu
def test_step_handles_are_stitch_plans(pf, synth, rig_a):
    top_a, imgs_a = rig_a
    top, imgs = rig(synth, COLS, ROWS, 1235)
    c = pf.Context(0)
    rg = c.rig_plan(top_a, imgs_a)
    want = [c.stitch_step(imgs[i], top if i == 0 else None, PCT) for i in range(2)]
    got = [c.stitch_step(imgs[i], top if i == 0 else None, PCT, plan=rg.steps[i]) for i in range(2)]
    for i in range(2):
        assert np.array_equal(got[i], want[i]), "planned step %d on a rig's step handle: %d bytes differ" % (i + 1, _ndiff(got[i], want[i]))
    mp, ramp = rg.steps[1].download()
    assert mp.shape == (ROWS, COLS) and ramp.dtype == np.float32
    # the rig owns its steps
    with pytest.raises(pf.PanoflowError, match="error -1: .*step of a rig plan"):
        rg.steps[1].close()
    assert np.array_equal(c.stitch_step(imgs[0], top, PCT, plan=rg.steps[0]), want[0])
    # after the rig is gone its step handles are no plans any more
    h = C.c_void_p(rg.steps[0].h.value)
    rg.close()
    sz = C.c_size_t(COLS * 4)
    out = np.empty((ROWS, COLS, 4), np.uint8)
    assert c.l.pf_stitch_step_planned(c.h, h, imgs[0].ctypes.data_as(C.c_void_p), top.ctypes.data_as(C.c_void_p), COLS, ROWS, sz, PCT,
                                      out.ctypes.data_as(C.c_void_p), sz) == -1
    c.close()


@pytest.mark.gpu
def test_plan_lifetime_across_owners(pf):
    """two stitch plans and a rig's step plans live in one list: the rig's end takes its steps out and leaves the others whole, a plan's end
    leaves its neighbour whole, and the context's end takes what is left"""
    cols, rows = 240, 200
    top, Ls = window_set(cols, rows, 2, 41)
    Rs = stand_ins(top, Ls)
    c = pf.Context(0)
    plans = [c.stitch_plan(Ls[i], Rs[i]) for i in range(2)]
    rg = c.rig_plan(top, Ls)
    before = [p.download() for p in plans]
    assert not np.array_equal(before[0][0], before[1][0]), "the two plans were meant to differ"
    h = C.c_void_p(rg.steps[0].h.value)   # what pf_rig_plan_step returned
    rg.close()
    sz = C.c_size_t(cols * 4)
    out = np.empty((rows, cols, 4), np.uint8); mp = np.empty((rows, cols), np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for name, call in (("pf_stitch_plan_download", lambda: c.l.pf_stitch_plan_download(c.h, h, ptr(mp), C.c_size_t(cols), None, sz)),
                       ("pf_stitch_step_planned", lambda: c.l.pf_stitch_step_planned(c.h, h, ptr(Ls[0]), ptr(top), cols, rows, sz, PCT, ptr(out), sz)),
                       ("pf_stitch_plan_destroy", lambda: c.l.pf_stitch_plan_destroy(c.h, h))):
        assert call() == -1, name
        assert name.encode() + b": not a live stitch plan" in c.l.pf_last_error(c.h)
    for i, p in enumerate(plans):
        _same_plan(p, before[i] + (p.overlap_px,), "stitch plan %d after the rig's end" % i)
    plans[0].close()
    want = c.stitch_step(Ls[1], Rs[1], PCT)
    got = c.stitch_step(Ls[1], Rs[1], PCT, plan=plans[1])
    assert np.array_equal(got, want), "planned step after its neighbour's end: %d bytes differ" % _ndiff(got, want)
    c.close()   # with plans[1] still live


@pytest.mark.gpu
def test_rig_plans_that_are_refused(pf, rig_a):
    top, imgs = rig_a
    c = pf.Context(0); other = pf.Context(0)
    rg = c.rig_plan(top, imgs)
    foreign = other.rig_plan(top, imgs)
    arr = lambda v: (C.c_void_p * len(v))(*[a.ctypes.data for a in v])
    sz = C.c_size_t(COLS * 4)
    assert c.l.pf_rig_stitch_batch(c.h, foreign.h, 1, arr([top]), arr(imgs), COLS, ROWS, sz, PCT, None, sz, 1) == -1
    assert b"not a live rig plan" in c.l.pf_last_error(c.h)
    assert c.l.pf_rig_plan_step(c.h, foreign.h, 0) is None
    assert c.l.pf_rig_plan_destroy(c.h, foreign.h) == -1
    # a wrong size
    small_top, small_ls = window_set(240, 200, 5, 3)
    with pytest.raises(pf.PanoflowError, match="error -1: .*the rig plan is 523x261"):
        c._chk(c.l.pf_rig_stitch_batch(c.h, rg.h, 1, arr([small_top]), arr(small_ls), 240, 200, C.c_size_t(240 * 4), PCT, None, C.c_size_t(240 * 4), 1))
    # step indices
    for bad in (-1, 5):
        assert c.l.pf_rig_plan_step(c.h, rg.h, bad) is None
        assert b"step %d of a rig plan of 5 steps" % bad in c.l.pf_last_error(c.h)
    # n_steps outside 1..16
    with pytest.raises(pf.PanoflowError, match="error -1: .*1..16 steps"):
        c.rig_plan(top, [])
    with pytest.raises(pf.PanoflowError, match="error -1: .*1..16 steps"):
        c.rig_plan(top, imgs * 4)
    # creation refuses what pf_stitch_plan_create refuses
    with pytest.raises(pf.PanoflowError, match="error -1"):
        c.rig_plan(np.zeros((1, 1, 4), np.uint8), [np.zeros((1, 1, 4), np.uint8)])
    # a destroyed rig: the handle is looked up, never dereferenced
    h = C.c_void_p(rg.h.value)
    rg.close()
    assert c.l.pf_rig_plan_step(c.h, h, 0) is None
    assert c.l.pf_rig_plan_destroy(c.h, h) == -1
    arr = lambda v: (C.c_void_p * len(v))(*[a.ctypes.data for a in v])
    assert c.l.pf_rig_stitch_batch(c.h, h, 1, arr([top]), arr(imgs), COLS, ROWS, C.c_size_t(COLS * 4), PCT, None, C.c_size_t(COLS * 4), 1) == -1
    # pf_destroy frees a live rig (foreign is still alive in `other`)
    other.close(); c.close()
