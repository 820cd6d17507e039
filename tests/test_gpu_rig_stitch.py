"""pf_rig_stitch_batch / _dev: the whole chain of every frame in one call gives, step by step, the bytes of the frame's own unplanned
pf_stitch_step chain; every frame is verified against the rig before anything is solved.  Seed A makes the rig; seeds B..E are the frames."""
import ctypes as C

import numpy as np
import pytest

from rig_cases import COLS, PCT, ROWS, SEED_A, SEEDS, rig

NB = COLS * ROWS * 4


def _ndiff(a, b):
    return int((a != b).sum())


@pytest.fixture(scope="module")
def rig_a(synth):
    return rig(synth, COLS, ROWS, SEED_A)


@pytest.fixture(scope="module")
def frames(synth):
    return [rig(synth, COLS, ROWS, s) for s in SEEDS]


@pytest.fixture(scope="module")
def chains(pf, frames):
    """the unplanned pf_stitch_step chains of seeds B..E: the reference of every result below"""
    c = pf.Context(0)
    ref = [[c.stitch_step(L, top if i == 0 else None, PCT) for i, L in enumerate(imgs)] for top, imgs in frames]
    c.close()
    return ref


def _check(outs, chains, what):
    for k in range(len(outs)):
        for i in range(5):
            assert np.array_equal(outs[k][i], chains[k][i]), "%s, frame %d step %d: %d bytes differ from pf_stitch_step's" % (
                what, k, i + 1, _ndiff(outs[k][i], chains[k][i]))


@pytest.mark.gpu
@pytest.mark.parametrize("in_flight", [1, 2, 4])
def test_host_form_equals_the_step_chains(pf, rig_a, frames, chains, in_flight):
    c = pf.Context(0)
    rg = c.rig_plan(*rig_a)
    outs = c.rig_stitch_batch(rg, [t for t, _ in frames], [ls for _, ls in frames], PCT, in_flight=in_flight)
    _check(outs, chains, "host form, in_flight %d" % in_flight)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [0, 1])
def test_host_form_of_more_than_two_waves_in_both_upload_forms(pf, rig_a, frames, chains, overlap):
    """4 frames at in_flight 1 are four waves: waves 3 and 4 go up a second time, beside the wave before (1) or between the waves (0);
    rows of a wider buffer (step_bytes > 4 cols) take the 2-D copies of either form"""
    c = pf.Context(0)
    c.rig_set_upload_overlap(overlap)
    rg = c.rig_plan(*rig_a)
    outs = c.rig_stitch_batch(rg, [t for t, _ in frames], [ls for _, ls in frames], PCT, in_flight=1)
    _check(outs, chains, "four waves, overlap %d" % overlap)
    wide = lambda im: np.ascontiguousarray(np.pad(im, ((0, 0), (0, 3), (0, 0))))
    tops, Ls = [wide(t) for t, _ in frames[:3]], [[wide(a) for a in ls] for _, ls in frames[:3]]
    out = [[np.empty((ROWS, COLS, 4), np.uint8) for _ in range(5)] for _ in range(3)]
    arr = lambda v: (C.c_void_p * len(v))(*[a.ctypes.data for a in v])
    c._chk(c.l.pf_rig_stitch_batch(c.h, rg.h, 3, arr(tops), arr([a for r in Ls for a in r]), COLS, ROWS, C.c_size_t((COLS + 3) * 4), PCT,
                                   arr([o for r in out for o in r]), C.c_size_t(COLS * 4), 1))
    _check(out, chains, "three waves from padded rows, overlap %d" % overlap)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("in_flight", [1, 2, 4])
def test_device_form_equals_the_step_chains(pf, rig_a, frames, chains, in_flight):
    c = pf.Context(0)
    rg = c.rig_plan(*rig_a)
    bufs = [c.dev_alloc(NB) for _ in range(4 * (6 + 5))]
    try:
        d_top, d_l, d_out = bufs[0:4], [bufs[4 + 5 * k:9 + 5 * k] for k in range(4)], [bufs[24 + 5 * k:29 + 5 * k] for k in range(4)]
        for k, (top, imgs) in enumerate(frames):
            c.upload(d_top[k], top)
            for i in range(5):
                c.upload(d_l[k][i], imgs[i])
        c.rig_stitch_batch_dev(rg, d_top, d_l, PCT, d_out, in_flight=in_flight)
        outs = [[c.download(np.empty((ROWS, COLS, 4), np.uint8), d_out[k][i]) for i in range(5)] for k in range(4)]
        _check(outs, chains, "device form, in_flight %d" % in_flight)
        # only the last composite asked for (frame 1 also its second): the others live in the internal ping-pong planes
        fill = np.full((ROWS, COLS, 4), 7, np.uint8)
        for k in range(4):
            for i in range(5):
                c.upload(d_out[k][i], fill)
        sparse = [[d_out[k][i] if i == 4 or (k == 1 and i == 1) else None for i in range(5)] for k in range(4)]
        c.rig_stitch_batch_dev(rg, d_top, d_l, PCT, sparse, in_flight=in_flight)
        for k in range(4):
            for i in range(5):
                got = c.download(np.empty((ROWS, COLS, 4), np.uint8), d_out[k][i])
                want = chains[k][i] if sparse[k][i] else fill
                assert np.array_equal(got, want), "device form with NULL entries, frame %d step %d: %d bytes differ" % (k, i + 1, _ndiff(got, want))
    finally:
        for p in bufs:
            c.dev_free(p)
        c.close()


@pytest.mark.gpu
def test_step_1_equals_the_oracle_and_null_entries_skip_downloads(pf, orc, rig_a, frames, chains):
    c = pf.Context(0)
    rg = c.rig_plan(*rig_a)
    tops, Ls = [t for t, _ in frames[:2]], [ls for _, ls in frames[:2]]
    out = [[np.full((ROWS, COLS, 4), 7, np.uint8) if (k + i) % 2 == 0 else None for i in range(5)] for k in range(2)]
    got = c.rig_stitch_batch(rg, tops, Ls, PCT, in_flight=2, out=out)
    for k in range(2):
        for i in range(5):
            if out[k][i] is not None:
                assert got[k][i] is out[k][i] and np.array_equal(got[k][i], chains[k][i]), "frame %d step %d: %d bytes differ" % (k, i + 1, _ndiff(got[k][i], chains[k][i]))
    # nothing asked for at all
    c.rig_stitch_batch(rg, tops, Ls, PCT, in_flight=2, want=lambda k, i: False)
    c.close()
    L, R = frames[0][1][0], frames[0][0]
    mp, ovl, ovr, blend, _ = orc.stitch_prepare(L, R, True)
    f0, f1 = orc.flow_bidir(ovl, ovr, PCT)
    want = orc.stitch_gather(L, R, orc.combine_novel_views(ovl, ovr, f0, f1, blend), mp)
    assert np.array_equal(got[0][0], want), "frame 0 step 1: %d bytes differ from the oracle's composite" % _ndiff(got[0][0], want)


def _third_image_with_one_alpha(frames, k, new_alpha):
    """frame k's images with ONE pixel of its third image changed from alpha 255 to new_alpha"""
    top, imgs = frames[k]
    im = imgs[2].copy()
    ys, xs = np.nonzero(im[..., 3] == 255)
    im[ys[len(ys) // 2], xs[len(ys) // 2], 3] = new_alpha
    return top, imgs[:2] + [im] + imgs[3:]


@pytest.mark.gpu
def test_frame_off_the_rig_fails_the_call_before_any_solve(pf, rig_a, frames, chains):
    c = pf.Context(0)
    rg = c.rig_plan(*rig_a)
    bad = list(frames[:3])
    bad[1] = _third_image_with_one_alpha(frames, 1, 0)
    tops, Ls = [t for t, _ in bad], [ls for _, ls in bad]
    out = [[np.full((ROWS, COLS, 4), 7, np.uint8) for _ in range(5)] for _ in range(3)]
    c.profile_enable(1)
    c.profile_reset()
    with pytest.raises(pf.PanoflowError, match=r"error -1: .*frame 1 differs from the rig plan at step 3 in 1 pixels"):
        c.rig_stitch_batch(rg, tops, Ls, PCT, in_flight=2, out=out)
    assert all((o == 7).all() for row in out for o in row), "a failed call delivered a composite"
    prof = c.profile()
    assert prof["rig_verify"][1] == 2 and "match_verify" not in prof and "blend" not in prof, "something was solved: %r" % sorted(prof)
    c.profile_enable(0)
    # the device form: the same refusal, its outputs zero-filled
    bufs = [c.dev_alloc(NB) for _ in range(2 * 11)]
    try:
        d_top, d_l, d_out = bufs[0:2], [bufs[2:7], bufs[7:12]], [bufs[12:17], bufs[17:22]]
        for k in range(2):
            c.upload(d_top[k], bad[k][0])
            for i in range(5):
                c.upload(d_l[k][i], bad[k][1][i]); c.upload(d_out[k][i], out[0][0])
        with pytest.raises(pf.PanoflowError, match=r"error -1: .*frame 1 differs from the rig plan at step 3 in 1 pixels"):
            c.rig_stitch_batch_dev(rg, d_top, d_l, PCT, d_out, in_flight=2)
        for k in range(2):
            for i in range(5):
                assert not c.download(np.empty((ROWS, COLS, 4), np.uint8), d_out[k][i]).any(), "frame %d step %d: a failed call left bytes" % (k, i + 1)
    finally:
        for p in bufs:
            c.dev_free(p)
    # a following good call gives the right bytes
    outs = c.rig_stitch_batch(rg, [t for t, _ in frames[:3]], [ls for _, ls in frames[:3]], PCT, in_flight=2, want=lambda k, i: i == 4)
    for k in range(3):
        assert np.array_equal(outs[k][4], chains[k][4]), "frame %d after a failed call: %d bytes differ" % (k, _ndiff(outs[k][4], chains[k][4]))
    c.close()


@pytest.mark.gpu
def test_alpha_255_to_1_is_on_the_rig(pf, rig_a, frames, chains):
    top, imgs = _third_image_with_one_alpha(frames, 0, 1)
    c = pf.Context(0)
    rg = c.rig_plan(*rig_a)
    want = [c.stitch_step(L, top if i == 0 else None, PCT) for i, L in enumerate(imgs)]
    got = c.rig_stitch_batch(rg, [top], [imgs], PCT, in_flight=1)
    for i in range(5):
        assert np.array_equal(got[0][i], want[i]), "step %d: %d bytes differ" % (i + 1, _ndiff(got[0][i], want[i]))
    c.close()


@pytest.mark.gpu
def test_the_call_leaves_the_step_chain_and_the_batch_slots_usable(pf, rig_a, frames, chains):
    c = pf.Context(0)
    rg = c.rig_plan(*rig_a)
    tops, Ls = [t for t, _ in frames[:2]], [ls for _, ls in frames[:2]]
    # a running pf_stitch_step chain (frame 2) and running batch slots (frames 0, 1), each one step in
    c.stitch_step(frames[2][1][0], frames[2][0], PCT, want_out=False)
    c.stitch_step_batch([ls[0] for ls in Ls], tops, PCT, in_flight=2, want_out=False)
    outs = c.rig_stitch_batch(rg, tops, Ls, PCT, in_flight=2, want=lambda k, i: i == 4)
    for k in range(2):
        assert np.array_equal(outs[k][4], chains[k][4])
    got = c.stitch_step(frames[2][1][1], None, PCT)
    assert np.array_equal(got, chains[2][1]), "pf_stitch_step's chain after a rig call: %d bytes differ" % _ndiff(got, chains[2][1])
    got = c.stitch_step_batch([ls[1] for ls in Ls], None, PCT, in_flight=2)
    for k in range(2):
        assert np.array_equal(got[k], chains[k][1]), "the batch slots after a rig call, frame %d: %d bytes differ" % (k, _ndiff(got[k], chains[k][1]))
    # the lone forms are the batch of one frame
    lib = c.l
    arr = lambda v: (C.c_void_p * len(v))(*[a.ctypes.data if a is not None else None for a in v])
    lone = [None, None, None, None, np.empty((ROWS, COLS, 4), np.uint8)]
    c._chk(lib.pf_rig_stitch(c.h, rg.h, tops[1].ctypes.data_as(C.c_void_p), arr(Ls[1]), COLS, ROWS, C.c_size_t(COLS * 4), PCT, arr(lone), C.c_size_t(COLS * 4)))
    assert np.array_equal(lone[4], chains[1][4])
    c.close()
