"""The latency form's record stream carries three floats per record, (E(C), rC); the sweep's loader completes the record in LDS with g0 and
blurred at the record's own pixel, read from the planes (zeros for a pixel that is not updated), and with Ea.  Held here to the oracle bit for bit
(uint32 views) where that can go wrong: the smallest windows in both orientations and directions, a record ring that wraps, planes whose
values at the pixels that are not updated must never reach a result, a context whose record buffer still holds a longer stream, a whole
level, and batched launches (blockIdx.z >= 1: every plane pointer of the loader carries the pair's offset).  Product library, latency form."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (w, h, box): a0 = 1 in the box, 0.5 in a hole inside it, corners kept gated; a1 = 1 (the gate pattern of test_sweep_only_covers_the_window_of_gated_pixels)
CASES = [
    (9, 9, (4, 4, 5, 5)),          # one updated pixel
    (43, 29, (10, 9, 37, 26)),     # first band and first column inside the image, h % 8 = 5, two workgroups
    (29, 43, (3, 11, 20, 43)),     # transposed, window on the bottom edge
    (70, 21, (17, 3, 66, 20)),     # more than 64 steps: the record ring wraps
    (21, 70, (2, 17, 19, 61)),     # transposed with a ring wrap
    (40, 40, (0, 0, 40, 40)),      # the whole image
]
POISON = np.array([np.nan, np.inf, -np.inf, 3e38, 1e-42], np.float32)
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _case(orc, w, h, box):
    """planes of a case and the oracle's result for both directions: computed once, shared by every test, never written to"""
    key = (w, h, box)
    if key not in _cache:
        r = np.random.default_rng(7 * w + h)
        img0 = r.random((h, w)).astype(np.float32); img1 = r.random((h, w)).astype(np.float32)
        g0 = np.stack(orc.gradients(img0), -1); g1 = np.stack(orc.gradients(img1), -1)
        flow = (r.standard_normal((h, w, 2)) * 2.0).astype(np.float32)
        blurred = orc.gaussian_blur(flow, 15, 8.0)
        a0 = np.zeros((h, w), np.float32); a1 = np.ones((h, w), np.float32)
        x0, y0, x1, y1 = box
        a0[y0:y1, x0:x1] = 1.0
        a0[y0 + (y1 - y0) // 3:y0 + (y1 - y0) // 2, x0 + (x1 - x0) // 4:x0 + (x1 - x0) // 2] = 0.5
        a0[y0, x0] = 1.0; a0[y1 - 1, x1 - 1] = 1.0
        ref = {fwd: orc.sweep(g0[..., 0], g0[..., 1], g1[..., 0], g1[..., 1], blurred, a0, a1, flow, fwd) for fwd in (1, 0)}
        for a in (g0, g1, flow, blurred, a0, a1, ref[0], ref[1]):
            a.setflags(write=False)
        _cache[key] = (g0, g1, blurred, a0, a1, flow, ref)
    return _cache[key]


@pytest.fixture(scope="module")
def ctx(pf):
    c = pf.Context(0, sweep_wide=0)
    yield c
    c.close()


def _check(ctx, orc, w, h, box, g0=None, blurred=None):
    cg0, g1, cbl, a0, a1, flow, ref = _case(orc, w, h, box)
    g0 = cg0 if g0 is None else g0
    blurred = cbl if blurred is None else blurred
    for fwd in (1, 0):
        got = ctx.stage_sweep(g0, g1, blurred, a0, a1, flow, fwd)
        bad = int((_bits(got) != _bits(ref[fwd])).sum())
        print("%dx%d fwd=%d: %d words differ" % (w, h, fwd, bad))
        assert bad == 0, "%dx%d fwd=%d: %d words differ" % (w, h, fwd, bad)
        upd = (a0 > 0.9) & (a1 > 0.9)
        assert (_bits(ref[fwd])[upd] != _bits(flow)[upd]).any(axis=-1).all()   # every gated pixel moves: a sweep that did nothing cannot pass


@pytest.mark.parametrize("w,h,box", CASES)
def test_smallest_windows_both_directions(ctx, orc, w, h, box):
    _check(ctx, orc, w, h, box)


@pytest.mark.parametrize("w,h,box", CASES)
def test_static_planes_of_pixels_not_updated_never_reach_the_result(ctx, orc, w, h, box):
    """g0 and blurred hold NaN, +inf, -inf, 3e38 or 1e-42 at every pixel that is not updated; the expected result is the oracle's on the
    clean planes (the reference never reads those values).  Catches a loader that forgets the `updated` select of the record's first quad,
    or reads another pixel's static half.  All five poison values are used, the non-finite ones included: the sweep with the two-quad
    record stream (the commit before this file) passes all twelve runs as well -- the loader's window offsets do read `blurred` at such
    pixels, but any offset gives the same bits."""
    g0, _, blurred, a0, a1, _, _ = _case(orc, w, h, box)
    r = np.random.default_rng(1000 + 3 * w + h)
    off = ~((a0 > 0.9) & (a1 > 0.9))
    pg0 = g0.copy(); pbl = blurred.copy()
    pg0[off] = r.choice(POISON, size=(int(off.sum()), 2))
    pbl[off] = r.choice(POISON, size=(int(off.sum()), 2))
    _, g1, _, _, _, flow, ref = _case(orc, w, h, box)
    for fwd in (1, 0):   # the premise: the reference's result does not depend on those values
        assert np.array_equal(_bits(orc.sweep(pg0[..., 0], pg0[..., 1], g1[..., 0], g1[..., 1], pbl, a0, a1, flow, fwd)), _bits(ref[fwd]))
    _check(ctx, orc, w, h, box, pg0, pbl)


def test_a_shorter_stream_does_not_pick_up_the_previous_sweeps_records(pf, orc):
    """one context, 70x21 then 9x9 then 43x29: the record buffer still holds the longer stream of the sweep before"""
    c = pf.Context(0, sweep_wide=0)
    try:
        for k in (3, 0, 1):
            _check(c, orc, *CASES[k])
    finally:
        c.close()


@pytest.mark.parametrize("w,h", [(61, 45), (45, 61)])
def test_a_whole_level_with_incoming_flow(ctx, orc, synth, w, h):
    """both prepasses, the medians between them and the transposed form"""
    L, R, _ = synth.make_pair_np(2 * w, 2 * h, 31)
    I0, A0 = orc.preprocess(L); I1, A1 = orc.preprocess(R)
    assert I0.shape == (h, w)
    A0 = A0.copy(); A0[h // 3:h // 2, w // 4:w // 2] = 0.5   # a hole of pixels that are not updated
    fin = (np.random.default_rng(w).standard_normal((h, w, 2)) * 0.7).astype(np.float32)
    ref = orc.level(I0, I1, A0, A1, fin, 3, 0)
    got = ctx.stage_level(I0, I1, A0, A1, fin, 3, 0)
    bad = int((_bits(got) != _bits(ref)).sum())
    print("%dx%d level: %d words differ" % (w, h, bad))
    assert bad == 0
    assert not np.array_equal(ref, fin)


def test_batched_launches_offset_every_plane(pf, orc, synth):
    """three pairs of 160x128 in one batch: latency-form launches with blockIdx.z = 0, 1, 2, each pair against the oracle"""
    cols, rows, n = 160, 128, 3
    c = pf.Context(0, sweep_wide=0, batch_pairs=n)
    try:
        px = cols * rows
        host, dev = [], []
        for i in range(n):
            L, R, blend = synth.make_pair_np(cols, rows, 500 + i)
            d = {"L": c.dev_alloc(px * 4), "R": c.dev_alloc(px * 4), "b": c.dev_alloc(px * 4), "o": c.dev_alloc(px * 4), "f0": c.dev_alloc(px * 8), "f1": c.dev_alloc(px * 8)}
            c.upload(d["L"], L); c.upload(d["R"], R); c.upload(d["b"], blend)
            host.append((L, R)); dev.append(d)
        c.novel_view_batch_dev([d["L"] for d in dev], [d["R"] for d in dev], cols, rows, 20, [d["b"] for d in dev], [d["o"] for d in dev],
                               [d["f0"] for d in dev], [d["f1"] for d in dev], in_flight=n)
        for i, ((L, R), d) in enumerate(zip(host, dev)):
            r0, r1 = orc.flow_bidir(L, R, 20)
            f0 = c.download(np.empty((rows, cols, 2), np.float32), d["f0"]); f1 = c.download(np.empty((rows, cols, 2), np.float32), d["f1"])
            bad = int((_bits(f0) != _bits(r0)).sum()) + int((_bits(f1) != _bits(r1)).sum())
            print("pair %d: %d words differ" % (i, bad))
            assert bad == 0, "pair %d: %d words differ" % (i, bad)
    finally:
        c.close()
