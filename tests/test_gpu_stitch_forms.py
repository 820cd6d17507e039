"""The kernels around the solver (csrc/kernels_misc.hip) against the oracle in every form, bit pattern by bit pattern: the final box blur
of the ramp smoothing (K14), the novel-view blend (K11), MatchImages, countblend and Gather (K12, K13, K15).

The stage tests feed these kernels canvases from synth, which never reach most of their code: a box blur of width 1, alphas 0 and 255,
overlaps away from the seam, one rectangular hole.  The inputs here are built for the kernels' geometry instead:

  box blur    explicit widths on both sides of the staged / wide switch (32 | 33), odd and even anchors, 64-column chunks and 64-row
              blocks with and without tails, the 8-row unrolled column pass with a tail, kernels wider than the image, and planes
              of a dynamic range at which the fp64 sliding sums round (on ordinary planes they are exact in any order);
  blend       a 766 x 256 table image that reads every entry of g_blend_tanh (row n: colour difference n) and of g_blend_alpha (column
              a: L alpha a, R alpha a permutation), with and without flows, widths that are no multiple of the block, flows longer
              than the image is wide, and the tables read from a context that did not initialise them;
  countblend  a hand-built map: an overlap across the seam (the wrapped ends of the virtual extended map), a nearest pixel on a
              diagonal, an overlap with nothing in reach, overlaps in row 0 and at extended column 0 (the reference's strict guards),
              one-pixel stripes that a stride of 2 steps over;
  gather      all eight codes, the L-before-R rule at equal distance, a nearer R, each diagonal alone, the 99-pixel reach, holes on
              every border.

What a case is meant to reach is asserted on its inputs and on the oracle's result alone, before the device is compared with anything.
Shapes are cols x rows.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
INF = np.inf


@pytest.fixture(scope="module")
def ctx(pf):
    c = pf.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def assert_bits(got, ref, what=""):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = bits(got) != bits(ref)
    if bad.any():
        at = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError("%s: %d of %d words differ, first at %s: got %r, reference %r" % (what, int(bad.sum()), bad.size, at, got[at], ref[at]))


def assert_bytes(got, ref, what=""):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape)
    bad = got != ref
    if bad.any():
        at = tuple(int(v[0]) for v in np.nonzero(bad))
        px = at[:2]
        raise AssertionError("%s: %d of %d bytes differ, first at %s: got %r, reference %r" % (what, int(bad.sum()), bad.size, at, got[px], ref[px]))


_cache = {}


def cached(key, make):
    """inputs and oracle results of a case, computed once per module run and never modified"""
    if key not in _cache:
        v = make()
        for a in (v.values() if isinstance(v, dict) else v):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


# ================================================================================================
# K14, the final box blur: orc.box_blur_roi over the whole image, which is what the oracle's ramp smoothing calls
# ================================================================================================
BOX_SHAPES = [
    (200, 70),   # four 64-column chunks, the last 8 wide; two 64-row blocks, the last 6 high
    (64, 64),    # exactly one chunk and one block
    (65, 65),    # one column and one row past them (rows % 8 = 1)
    (63, 9),     # less than a chunk; the rows of a short block repeat the last one while staging (rows % 8 = 1)
    (129, 64),   # two whole chunks and one column
    (128, 24),   # two whole chunks, no tail; whole 8-row groups
    (5, 130),    # kernel wider than the image in x: repeated reflection in the row pass
    (130, 5),    # ... and in y, in the column pass
    (1, 9), (9, 1),
    (33, 15),    # rows % 8 = 7
]
BOX_KS = [1, 2, 3, 10, 31, 32,   # row pass staged through LDS (k <= 32): odd and even anchors, the widest staged window
          33, 65]                # row pass straight from memory


def box_plane(cols, rows, seed=0):
    """standard-normal noise on a ramp: the sliding fp64 sums round differently with the order of their terms"""
    r = np.random.default_rng(1000 * cols + rows + 7919 * seed)
    ramp = np.arange(cols, dtype=F32)[None, :] * F32(0.25) + np.arange(rows, dtype=F32)[:, None] * F32(0.5)
    return (r.standard_normal((rows, cols)).astype(F32) + ramp).astype(F32)


def box_case(orc, cols, rows, k, seed=0):
    def make():
        img = box_plane(cols, rows, seed)
        return {"img": img, "ref": orc.box_blur_roi(img, 0, 0, cols, rows, k)}
    return cached(("box", cols, rows, k, seed), make)


@pytest.mark.parametrize("k", BOX_KS)
@pytest.mark.parametrize("cols,rows", BOX_SHAPES)
def test_box_blur_every_form(ctx, orc, cols, rows, k):
    c = box_case(orc, cols, rows, k)
    if k == 1:
        assert np.array_equal(bits(c["ref"]), bits(c["img"]))      # the identity: what nearly every small canvas runs
    else:
        assert not np.array_equal(c["ref"], c["img"])
    assert_bits(ctx.stage_box_blur(c["img"], k), c["ref"], "box blur %dx%d k %d" % (cols, rows, k))


def box_plane_wide_range(cols, rows):
    """noise scaled by 2^-40 .. 2^40 per pixel.  The planes above do not make the fp64 sliding sums round at all: floats of about one
    magnitude add exactly in 53 bits, in any order.  Here a window holds values 80 binary orders apart, every update rounds, and a sum
    carried along the row differs from a fresh sum of the same window."""
    r = np.random.default_rng(77 * cols + rows)
    return (r.standard_normal((rows, cols)) * np.exp2(r.integers(-40, 41, (rows, cols)))).astype(F32)


def sliding_row_sums(img, k):
    """RowSum of blur(): the first window summed left to right, then one add and one subtract per pixel, in fp64 (BORDER_REFLECT_101)"""
    rows, cols = img.shape
    a = k // 2

    def col(x):
        while x < 0 or x >= cols:
            x = -x if x < 0 else 2 * cols - 2 - x
        return img[:, x].astype(np.float64)
    s = np.zeros(rows)
    for i in range(k):
        s = s + col(-a + i)
    out = [s]
    for x in range(1, cols):
        s = s + (col(x - a - 1 + k) - col(x - a - 1))
        out.append(s)
    return np.stack(out, 1)


@pytest.mark.parametrize("k", [2, 3, 10, 31, 32, 33])
@pytest.mark.parametrize("cols,rows", [(200, 70), (129, 64), (65, 65)])
def test_box_blur_sums_that_round(ctx, orc, cols, rows, k):
    """the sliding sum is carried from one 64-column chunk into the next exactly as it stands"""
    def make():
        img = box_plane_wide_range(cols, rows)
        return {"img": img, "ref": orc.box_blur_roi(img, 0, 0, cols, rows, k)}
    c = cached(("box_wide", cols, rows, k), make)
    carried = sliding_row_sums(c["img"], k)
    for x in range(64, cols, 64):   # at every chunk's first column the carried sum is not the fresh sum of its window, in most rows
        fresh = np.zeros(rows)
        for i in range(k):
            fresh = fresh + c["img"][:, min(x - k // 2 + i, 2 * cols - 2 - (x - k // 2 + i))].astype(np.float64)
        assert (fresh != carried[:, x]).mean() > 0.5, (x, float((fresh != carried[:, x]).mean()))
    assert np.isfinite(c["ref"]).all()
    assert_bits(ctx.stage_box_blur(c["img"], k), c["ref"], "box blur, wide range, %dx%d k %d" % (cols, rows, k))


@pytest.mark.parametrize("k", [3, 33])
@pytest.mark.parametrize("cols,rows", [(200, 70), (65, 65)])
def test_box_blur_batch_of_three(ctx, orc, cols, rows, k):
    """three different planes in one launch (blockIdx.z = frame, 256-byte-aligned frame strides): each equals its lone result and the oracle"""
    cases = [box_case(orc, cols, rows, k, seed) for seed in range(3)]
    assert not np.array_equal(cases[0]["img"], cases[1]["img"]) and not np.array_equal(cases[1]["img"], cases[2]["img"])
    got = ctx.stage_box_blur(np.stack([c["img"] for c in cases]), k)
    for f, c in enumerate(cases):
        assert_bits(got[f], c["ref"], "frame %d of 3, %dx%d k %d" % (f, cols, rows, k))
        assert_bits(ctx.stage_box_blur(c["img"], k), got[f], "lone frame %d, %dx%d k %d" % (f, cols, rows, k))


def test_box_blur_argument_errors(ctx, pf):
    img = box_plane(16, 8)
    with pytest.raises(pf.PanoflowError):
        ctx.stage_box_blur(img, 0)
    with pytest.raises(pf.PanoflowError):
        ctx.stage_box_blur(img, -3)
    with pytest.raises(pf.PanoflowError):
        ctx.stage_box_blur(np.stack([img] * 4), 3)
    out = np.empty_like(img)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    f = ctx.l.pf_stage_box_blur
    assert f(ctx.h, 0, ptr(img), 16, 8, 3, ptr(out)) != 0
    assert f(ctx.h, 1, None, 16, 8, 3, ptr(out)) != 0
    assert f(ctx.h, 1, ptr(img), 16, 8, 3, None) != 0
    assert f(ctx.h, 1, ptr(img), 0, 8, 3, ptr(out)) != 0
    assert f(ctx.h, 1, ptr(img), 16, 0, 3, ptr(out)) != 0
    assert f(ctx.h, 1, ptr(img), 16, 8, 3, ptr(out)) == 0   # the context still works


# ================================================================================================
# K11, the novel-view blend: orc.combine_novel_views
# ================================================================================================
TAB_COLS, TAB_ROWS = 256, 766
EXP_MAX = 700.0   # exp() of a larger argument nears DBL_MAX (709.78): inf / inf is a NaN and its conversion to a byte is undefined


def random_flow(r, cols, rows, max_mag):
    ang = r.random((rows, cols)) * 2 * np.pi
    mag = r.random((rows, cols)) * max_mag
    return np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1).astype(F32)


def exp_bound(fLR, fRL, cols, alpha_max=255):
    """upper bound of the softmax's exp arguments: kSoftmaxSharpness * blend * alpha * (1 + kFlowMagCoef * |flow| / cols), blend <= 1"""
    mag = max(float(np.sqrt(f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1]).max()) for f in (fLR, fRL)) / cols
    return 10.0 * (alpha_max / 255.0) * (1.0 + 100.0 * mag)


def blend_table(orc, flows):
    """Row n: the two colours differ by n in all (split over the channels, the first share rotating with n, either image the brighter one
    per channel and column); column a: L alpha a, R alpha (7a + 3) % 256; blend random with rows of exact 0 and exact 1."""
    def make():
        cols, rows = TAB_COLS, TAB_ROWS
        r = np.random.default_rng(766256 + int(flows))
        n = np.arange(rows)
        d = np.zeros((rows, 3), np.int64)
        d[:, 0] = np.minimum(n, 255); d[:, 1] = np.minimum(n - d[:, 0], 255); d[:, 2] = n - d[:, 0] - d[:, 1]
        d = np.stack([np.roll(d[i], i % 3) for i in range(rows)])[:, None, :]
        base = r.integers(0, 256 - d, size=(rows, cols, 3))
        l_brighter = (np.arange(cols)[None, :, None] + np.arange(3)[None, None, :] + n[:, None, None]) % 2 == 0
        a = np.arange(cols)
        L = np.empty((rows, cols, 4), np.uint8); R = np.empty_like(L)
        L[..., :3] = base + np.where(l_brighter, d, 0); R[..., :3] = base + np.where(l_brighter, 0, d)
        L[..., 3] = a[None, :]; R[..., 3] = ((7 * a + 3) % 256)[None, :]
        blend = r.random((rows, cols), dtype=F32)
        blend[[100, 600]] = F32(0.0); blend[[101, 601]] = F32(1.0)
        if flows:
            fLR = random_flow(r, cols, rows, 0.59 * cols); fRL = random_flow(r, cols, rows, 0.59 * cols)
        else:
            fLR = np.zeros((rows, cols, 2), F32); fRL = np.zeros((rows, cols, 2), F32)
        return {"L": L, "R": R, "fLR": fLR, "fRL": fRL, "blend": blend, "ref": orc.combine_novel_views(L, R, fLR, fRL, blend)}
    return cached(("table", bool(flows)), make)


def check_table_inputs(c):
    diff = np.abs(c["L"][..., :3].astype(np.int64) - c["R"][..., :3].astype(np.int64))
    assert np.array_equal(np.unique(diff.sum(-1)), np.arange(766))           # every entry of g_blend_tanh
    for ch in range(3):   # either image is the brighter one, in every channel
        assert (c["L"][..., ch] > c["R"][..., ch]).any() and (c["L"][..., ch] < c["R"][..., ch]).any()
    assert np.unique(c["L"][..., 3]).size == 256 and np.unique(c["R"][..., 3]).size == 256   # every entry of g_blend_alpha, from either image
    assert (c["blend"] == 0).all(1).sum() == 2 and (c["blend"] == 1).all(1).sum() == 2
    assert (c["ref"][..., 3] == 255).mean() >= 0.95


def test_blend_table_reads_every_table_entry(ctx, orc):
    c = blend_table(orc, False)
    check_table_inputs(c)
    assert not c["fLR"].any() and not c["fRL"].any()
    # zero flows: every pixel blends its own two colours, so the valid pixels themselves cover the tables
    valid = c["ref"][..., 3] == 255
    diff = np.abs(c["L"][..., :3].astype(np.int64) - c["R"][..., :3].astype(np.int64)).sum(-1)
    assert np.unique(diff[valid]).size == 766
    # alpha 0 is the invalid pixel: two columns, and with them one value of the other image's alpha; between them the images read 1..255
    assert np.unique(c["L"][..., 3][valid]).size == 254 and np.unique(c["R"][..., 3][valid]).size == 254
    assert np.array_equal(np.union1d(c["L"][..., 3][valid], c["R"][..., 3][valid]), np.arange(1, 256))
    assert_bytes(ctx.blend(c["L"], c["R"], c["fLR"], c["fRL"], c["blend"]), c["ref"], "blend table, zero flows")


def test_blend_table_with_flows(ctx, orc):
    """the same table gathered through flows of random direction, up to 0.6 * cols long: the flow-magnitude factor of the exp arguments"""
    c = blend_table(orc, True)
    check_table_inputs(c)
    assert exp_bound(c["fLR"], c["fRL"], TAB_COLS) <= 10.0 * (1 + 60) < EXP_MAX
    assert float(np.abs(c["fRL"][..., 0]).max()) > 0.5 * TAB_COLS   # sources on the far side of the seam: the single wrap
    assert_bytes(ctx.blend(c["L"], c["R"], c["fLR"], c["fRL"], c["blend"]), c["ref"], "blend table with flows")


def blend_odd(orc, cols, rows, alphas, max_mag, seed=0):
    def make():
        r = np.random.default_rng(31 * cols + rows + 101 * seed)
        L = r.integers(0, 256, (rows, cols, 4), dtype=np.uint8); R = r.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
        L[..., 3] = r.choice(alphas, (rows, cols)); R[..., 3] = r.choice(alphas, (rows, cols))
        same = r.random((rows, cols)) < 0.25   # equal colours: c * wL + c * wR lies within an ulp of the integer c
        R[same, :3] = L[same, :3]
        blend = r.random((rows, cols), dtype=F32)
        blend[0] = F32(0.0); blend[rows - 1] = F32(1.0)
        fLR = random_flow(r, cols, rows, max_mag * cols); fRL = random_flow(r, cols, rows, max_mag * cols)
        return {"L": L, "R": R, "fLR": fLR, "fRL": fRL, "blend": blend, "ref": orc.combine_novel_views(L, R, fLR, fRL, blend)}
    return cached(("odd", cols, rows, tuple(alphas), max_mag, seed), make)


@pytest.mark.parametrize("cols,rows", [(257, 33), (255, 31)])
def test_blend_widths_off_the_block(ctx, orc, cols, rows):
    """cols % 256 = 1 and 255 (a block of one pixel, a block one short), odd rows, the alphas next to the table's ends"""
    alphas = [0, 1, 127, 254, 255]
    c = blend_odd(orc, cols, rows, alphas, 0.3)
    for img in (c["L"], c["R"]):
        assert set(np.unique(img[..., 3]).tolist()) == set(alphas)
    assert exp_bound(c["fLR"], c["fRL"], cols) < EXP_MAX
    assert 0.3 < (c["ref"][..., 3] == 255).mean() < 0.9   # valid and invalid pixels side by side
    assert_bytes(ctx.blend(c["L"], c["R"], c["fLR"], c["fRL"], c["blend"]), c["ref"], "blend %dx%d" % (cols, rows))


def test_blend_flows_longer_than_the_image_is_wide(ctx, orc):
    """sources more than a width away: the true modulo both sides define behind the reference's single wrap.  Alphas 1..3 keep the exp
    arguments small whatever the flow's length."""
    cols, rows = 130, 40
    c = blend_odd(orc, cols, rows, [1, 2, 3], 2.5)
    assert exp_bound(c["fLR"], c["fRL"], cols, alpha_max=3) < EXP_MAX
    reach = np.abs(c["fRL"][..., 0].astype(np.float64) * c["blend"])
    assert (reach > 2 * cols).sum() >= 20 and (reach > cols).sum() >= 200
    assert (c["ref"][..., 3] == 255).all()
    assert_bytes(ctx.blend(c["L"], c["R"], c["fLR"], c["fRL"], c["blend"]), c["ref"], "blend with flows of 2.5 widths")


def test_blend_tables_read_from_a_second_context(pf, ctx, orc):
    """g_blend_tanh / g_blend_alpha are written once per device, by the first context: three different pairs through pf_blend_dev on a
    context created after it (pf_novel_view_batch_dev solves its own flows, so the tables go through the device form of the blend)"""
    cases = [blend_table(orc, True), blend_odd(orc, 257, 33, [0, 1, 127, 254, 255], 0.3), blend_odd(orc, 255, 31, [0, 1, 127, 254, 255], 0.3, seed=1)]
    assert ctx.h   # the module's context came first
    c2 = pf.Context(0)
    try:
        pend = []
        for c in cases:
            rows, cols = c["blend"].shape
            n = cols * rows
            d = {"L": c2.dev_alloc(n * 4), "R": c2.dev_alloc(n * 4), "fLR": c2.dev_alloc(n * 8), "fRL": c2.dev_alloc(n * 8), "blend": c2.dev_alloc(n * 4), "o": c2.dev_alloc(n * 4)}
            for k in ("L", "R", "fLR", "fRL", "blend"):
                c2.upload(d[k], c[k])
            pend.append(d)
        for c, d in zip(cases, pend):
            rows, cols = c["blend"].shape
            c2.blend_dev(d["L"], d["R"], d["fLR"], d["fRL"], d["blend"], cols, rows, d["o"])
        for i, (c, d) in enumerate(zip(cases, pend)):
            got = c2.download(np.empty_like(c["ref"]), d["o"])
            assert_bytes(got, c["ref"], "pair %d of 3 on the second context" % i)
            for p in d.values():
                c2.dev_free(p)
    finally:
        c2.close()


# ================================================================================================
# K12 MatchImages + overlap masking
# ================================================================================================
@pytest.mark.parametrize("cols,rows", [(257, 33), (64, 5), (300, 7)])
def test_match_images_alpha_values(ctx, orc, cols, rows):
    """alpha 1 and 128 are as opaque as 255; cols * rows off the block size"""
    r = np.random.default_rng(cols * 7 + rows)
    L = r.integers(0, 256, (rows, cols, 4), dtype=np.uint8); R = r.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    L[..., 3] = r.choice([0, 1, 128, 255], (rows, cols)); R[..., 3] = r.choice([0, 1, 128, 255], (rows, cols))
    mp, ovl, ovr = orc.stitch_prepare(L, R, False)[:3]
    assert set(np.unique(mp).tolist()) == {0, 50, 100, 150}
    for a in (1, 128, 255):
        assert (mp[L[..., 3] == a] >= 100).all() and (mp[R[..., 3] == a] % 100 == 50).all()
    gm, gl, gr = ctx.stitch_match(L, R)
    assert_bytes(gm, mp, "map"); assert_bytes(gl, ovl, "overlap L"); assert_bytes(gr, ovr, "overlap R")


# ================================================================================================
# K13 countblend: orc.stitch_prepare(L, R, False), through pf_stitch_raw_blend on images whose alphas encode a hand-built map
# ================================================================================================
AXES = [(0, 1), (0, -1), (1, 0), (-1, 0)]
DIAGS = [(1, 1), (-1, -1), (-1, 1), (1, -1)]


def cb_map(cols, rows, shift=0):
    """The map (0 / 50 = R only / 100 = L only / 150 = overlap) and a mask per feature.  s = 1 on the 230 x 210 canvas (stride 1), 2 on
    420 x 400 (stride 2).  shift moves the stripes of (e) by that many pixels."""
    s = cols // 210
    m = np.zeros((rows, cols), np.uint8)
    feat = {}

    def put(code, r0, r1, c0, c1):
        assert 0 <= r0 < r1 <= rows and 0 <= c0 < c1 <= cols, (r0, r1, c0, c1)
        m[r0:r1, c0:c1] = code

    def mask(*boxes):
        k = np.zeros((rows, cols), bool)
        for r0, r1, c0, c1 in boxes:
            k[r0:r1, c0:c1] = True
        return k
    # (a) an overlap band across the seam; L only directly left of it on the far side, R only directly right
    b0, b1 = cols // 12, cols - cols // 14
    segs = ((36 * s, 90 * s),)
    for r0, r1 in segs:
        put(150, r0, r1, 0, b0); put(150, r0, r1, b1, cols)
        put(100, r0, r1, b1 - 14 * s, b1); put(50, r0, r1, b0, b0 + 14 * s)
    feat["a"] = mask(*[(r0, r1, 0, b0) for r0, r1 in segs], *[(r0, r1, b1, cols) for r0, r1 in segs])
    # (b) a block whose nearest L-only pixels lie on a diagonal (a square off its lower right corner); an axis hit much farther right
    put(150, 14 * s, 26 * s, 40 * s, 52 * s)
    put(100, 26 * s, 32 * s, 52 * s, 58 * s)
    put(100, 14 * s, 26 * s, 82 * s, 84 * s)
    put(50, 14 * s, 26 * s, 30 * s, 36 * s)
    feat["b"] = mask((14 * s, 26 * s, 40 * s, 52 * s))
    # (c) a block with neither L only nor R only along any of its probes (those to the left run through the wrap): the eight rays of
    # each of its pixels miss every other feature on both canvases
    put(150, 136 * s, 144 * s, 6 * s, 14 * s)
    feat["c"] = mask((136 * s, 144 * s, 6 * s, 14 * s))
    # (d) the strict guards (x - i > 0, y - i > 0).  Row 0: overlap with L only / R only directly below; L only IN row 0 above an
    # overlap that no upward probe may see.  Column 0: L only directly left through the wrap, then directly right.  Extended column 0
    # (source column cols - cols / 5), the one column no leftward probe reads: L only there and nowhere else in reach.
    put(150, 0, 1, 130 * s, 160 * s); put(100, 1, 2, 130 * s, 145 * s); put(50, 1, 2, 145 * s, 160 * s)
    put(100, 0, 1, 165 * s, 195 * s); put(150, 1, 3, 165 * s, 195 * s); put(50, 3, 4, 165 * s, 195 * s)
    put(150, 166 * s, 176 * s, 0, 1); put(100, 166 * s, 176 * s, cols - 1, cols); put(50, 166 * s, 176 * s, 1, 4)
    put(150, 178 * s, 188 * s, 0, 1); put(100, 178 * s, 188 * s, 1, 2); put(50, 178 * s, 188 * s, cols - 1, cols)
    put(150, 190 * s, 198 * s, 0, 19 * s); put(100, 190 * s, 198 * s, cols - cols // 5, cols - cols // 5 + 1); put(50, 190 * s, 198 * s, 19 * s, 21 * s)
    feat["d"] = mask((0, 1, 130 * s, 160 * s), (1, 3, 165 * s, 195 * s), (166 * s, 176 * s, 0, 1), (178 * s, 188 * s, 0, 1), (190 * s, 198 * s, 0, 19 * s))
    feat["d_ext0"] = mask((190 * s, 198 * s, 0, 19 * s))
    # (e) one-pixel stripes at odd offsets from a block: L only 5 columns right of its last column, R only 5 rows below its last row
    put(150, 146 * s, 160 * s, 150 * s, 160 * s)
    put(100, 146 * s, 160 * s, 160 * s + 4 + shift, 160 * s + 5 + shift)
    put(50, 160 * s + 4 + shift, 160 * s + 5 + shift, 150 * s, 160 * s)
    feat["e"] = mask((146 * s, 160 * s, 150 * s, 160 * s))
    for k in feat.values():
        assert (m[k] == 150).all()
    return m, feat


def cb_probe(m, code, wrap=True):
    """distance of the first pixel of `code` along each of countblend's eight probes (StitchTool.cpp:148-191), from the map alone: the
    map extended by cols / 5 wrapped columns per side (wrap=False: by columns of no code), stride min(cols, rows) / 200, i < cols / 2,
    the guards x + i < width, x - i > 0, y + i < rows, y - i > 0.  Returns {(dy, dx): (rows, cols) float64}: inf = no hit, and
    everywhere outside the overlap, which is all countblend probes from."""
    rows, cols = m.shape
    length, step = cols // 5, max(1, min(cols, rows) // 200)
    side = lambda a: a if wrap else np.full_like(a, 255)
    ext = np.concatenate([side(m[:, cols - length:]), m, side(m[:, :length])], 1)
    MW = ext.shape[1]
    Y, X = np.nonzero(m == 150)
    X = X + length
    out = {}
    for dy, dx in AXES + DIAGS:
        best = np.full(Y.size, INF)
        for i in range(0, cols // 2, step):
            yy = Y + dy * i; xx = X + dx * i
            ok = best == INF
            if dy > 0: ok &= yy < rows
            if dy < 0: ok &= yy > 0
            if dx > 0: ok &= xx < MW
            if dx < 0: ok &= xx > 0
            hit = ok & (ext[np.clip(yy, 0, rows - 1), np.clip(xx, 0, MW - 1)] == code)
            best[hit] = i * (np.sqrt(2.0) if dy and dx else 1.0)
        full = np.full((rows, cols), INF)
        full[Y, X - length] = best
        out[(dy, dx)] = full
    return out


def cb_case(orc, cols, rows, shift=0):
    def make():
        m, feat = cb_map(cols, rows, shift)
        r = np.random.default_rng(cols + rows)
        L = r.integers(0, 256, (rows, cols, 4), dtype=np.uint8); R = r.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
        L[..., 3] = np.where(m >= 100, r.choice([1, 128, 255], (rows, cols)), 0)
        R[..., 3] = np.where(m % 100 == 50, r.choice([1, 128, 255], (rows, cols)), 0)
        mp, _, _, blend, md = orc.stitch_prepare(L, R, False)
        assert np.array_equal(mp, m)
        c = {"L": L, "R": R, "map": m, "blend": blend, "md": md}
        c.update(("feat_" + k, v) for k, v in feat.items())
        return c
    return cached(("cb", cols, rows, shift), make)


def check_cb_inputs(c, orc):
    """what the map is meant to reach, from the map alone (cb_probe) and from the oracle's result alone"""
    m = c["map"]
    rows, cols = m.shape
    mn = lambda p, dirs: np.minimum.reduce([p[d] for d in dirs])
    pl, pr = cb_probe(m, 100), cb_probe(m, 50)
    # (a) the seam: the nearest L only along the row lies across the wrap
    row_wrap = mn(pl, [(0, 1), (0, -1)])
    row_flat = mn(cb_probe(m, 100, wrap=False), [(0, 1), (0, -1)])
    assert int((row_wrap < row_flat)[c["feat_a"]].sum()) >= 500
    # ... through both of the extended map's ends
    left_half = c["feat_a"] & (np.arange(cols)[None, :] < cols // 2)
    assert (pl[(0, -1)][left_half] < INF).all() and (pr[(0, 1)][c["feat_a"] & ~left_half] < INF).all()
    # (b) a diagonal hit beats every axis hit, although an axis hit exists
    diag, axis = mn(pl, DIAGS), mn(pl, AXES)
    assert int(((diag < axis) & (axis < INF))[c["feat_b"]].sum()) >= 50
    # (c) nothing along any probe
    none = (mn(pl, AXES + DIAGS) == INF) & (mn(pr, AXES + DIAGS) == INF)
    assert none[c["feat_c"]].all() and int(c["feat_c"].sum()) >= 50
    assert (c["blend"][c["feat_c"]] == F32(0.5)).all() and (c["md"][c["feat_c"]] == F32(10 * cols)).all()
    # (d) overlap in row 0 and in column 0, the neighbours the comment of cb_map names, and the one column the strict guard hides
    d = c["feat_d"]
    assert int(d[0].sum()) >= 25 and int(d[:, 0].sum()) >= 25 and int(d.sum()) >= 50
    assert (m[1, d[0]] != 150).all() and (m[0, d[1]] == 100).all()
    col0 = np.nonzero(d[:, 0])[0]
    assert set(np.unique(m[col0, cols - 1]).tolist()) >= {50, 100} and set(np.unique(m[col0, 1]).tolist()) >= {50, 100}
    assert (pl[(-1, 0)][1:3][d[1:3]] == INF).all()                 # L only in row 0 directly above: never seen
    e0 = c["feat_d_ext0"]
    step = max(1, min(cols, rows) // 200)
    assert (mn(pl, [(0, 1), (0, -1)])[e0] == INF).all()            # with x - i >= 0 they would see it at i = x + cols / 5
    hidden = e0 & ((np.arange(cols)[None, :] + cols // 5) % step == 0) & (np.arange(cols)[None, :] + cols // 5 < cols // 2)
    assert int(hidden.sum()) >= 50 and (m[e0.any(1), cols - cols // 5] == 100).all()
    assert int((mn(pl, AXES + DIAGS)[hidden] > np.arange(cols)[None, :].repeat(rows, 0)[hidden] + cols // 5).sum()) >= 50   # nothing nearer would mask it
    # (e) stride: on the stride-2 canvas half of the block's columns step over the stripe
    if step >= 2:
        e = c["feat_e"]
        assert (pl[(0, 1)][e] == INF).any() and (pl[(0, 1)][e] < INF).any()
        moved = cb_case(orc, cols, rows, shift=1)
        assert np.array_equal(moved["feat_e"], e)
        assert (bits(moved["blend"])[e] != bits(c["blend"])[e]).sum() >= e.sum() // 2


@pytest.mark.parametrize("cols,rows", [(230, 210), (420, 400)])
def test_countblend_hand_built_map(ctx, orc, cols, rows):
    """stride 1 and stride 2 (min(cols, rows) / 200)"""
    c = cb_case(orc, cols, rows)
    check_cb_inputs(c, orc)
    ov = c["map"] == 150
    assert len(np.unique(c["blend"][ov])) > 100 and (c["md"][~ov] == 0).all()
    blend, md = ctx.stitch_raw_blend(c["L"], c["R"])
    assert_bits(blend, c["blend"], "raw blend %dx%d" % (cols, rows))
    assert_bits(md, c["md"], "MergedDis %dx%d" % (cols, rows))


# ================================================================================================
# K15 Gather: orc.stitch_gather on hand-built maps and merged images
# ================================================================================================
def gather_case(orc, cols, rows):
    """Base: overlap (150) whose merged alpha is random in {0, 1, 255}: a third of the canvas are holes, which neither attract nor stop a
    probe.  Columns [cols - 40, cols): four row bands of map 0 / 50 / 100 / 150, which with the merged alphas give all eight codes.
    Left of column cols - 139 no hole reaches them, and the only L-only / R-only pixels are the planted ones:
    expect[(y, x)] = 'L', 'R' or 'none' for the hole at (y, x)."""
    def make():
        r = np.random.default_rng(cols * 3 + rows)
        L = r.integers(0, 256, (rows, cols, 4), dtype=np.uint8); R = r.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
        merged = r.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
        merged[..., 3] = r.choice([0, 1, 255], (rows, cols))
        mp = np.full((rows, cols), 150, np.uint8)
        q = rows // 4
        for j, code in enumerate((0, 50, 100, 150)):
            mp[j * q:(rows if j == 3 else (j + 1) * q), cols - 40:] = code
        expect = {}

        def hole(y, x, want, plants):
            assert x + 99 < cols - 40
            merged[y, x, 3] = 0
            expect[(y, x)] = want
            for (py, px, code) in plants:
                assert mp[py, px] == 150 and (py, px) not in expect
                mp[py, px] = code; merged[py, px, 3] = 0   # (with a merged alpha it would be code 125 / 175: merged, no match)
        hole(10, 30, "L", [(10, 33, 100), (10, 27, 50)])           # L only and R only both at k = 3: L wins
        hole(10, 60, "R", [(10, 62, 50), (10, 57, 100)])           # R only at k = 2, L only at k = 3: R wins
        hole(30, 20, "R", [(26, 16, 50)])                          # each diagonal alone, k = 4
        hole(30, 40, "L", [(26, 44, 100)])
        hole(30, 60, "R", [(34, 56, 50)])
        hole(30, 80, "L", [(34, 84, 100)])
        hole(20, 5, "L", [(20, 104, 100)])                         # k = 99: the last distance probed
        hole(40, 6, "none", [(40, 106, 50)])                       # k = 100: out of reach
        hole(0, 0, "R", [(0, 2, 50)])                              # holes on the borders: probes outside the canvas match nothing
        hole(0, 50, "L", [(1, 50, 100)])
        hole(rows - 1, 50, "R", [(rows - 2, 51, 50)])
        hole(50, 0, "L", [(50, 1, 100)])
        if rows >= 120:   # the reach along a column and along a diagonal
            hole(5, 150, "L", [(104, 150, 100)])
            hole(6, 135, "none", [(106, 135, 50)])
            hole(120, 10, "R", [(219, 109, 50)])
            hole(125, 100, "none", [(225, 0, 100)])
        merged[rows - 2, cols - 1, 3] = 0; merged[rows - 1, cols - 1, 3] = 0   # holes on the right border and in a corner (band of map 150)
        return {"L": L, "R": R, "merged": merged, "map": mp, "expect": expect, "ref": orc.stitch_gather(L, R, merged, mp)}
    return cached(("gather", cols, rows), make)


@pytest.mark.parametrize("cols,rows", [(300, 257), (257, 60)])
def test_gather_decision_table(ctx, orc, cols, rows):
    c = gather_case(orc, cols, rows)
    mp, merged, ref = c["map"], c["merged"], c["ref"]
    code = mp.astype(np.int64) + np.where(merged[..., 3] > 0, 75, 0)
    assert set(np.unique(code).tolist()) == {0, 50, 100, 150, 75, 125, 175, 225}
    assert set(np.unique(merged[..., 3]).tolist()) == {0, 1, 255}
    for v in (75, 125, 175, 225):   # merged alpha 1 counts as merged
        assert (merged[..., 3][code == v] == 1).any()
    # the oracle alone: every code's rule, and the planted holes
    assert (ref[code == 0] == 0).all() and (ref[code == 75] == 0).all()
    assert np.array_equal(ref[code == 50], c["R"][code == 50]) and np.array_equal(ref[code == 100], c["L"][code == 100])
    for v in (125, 175, 225):
        assert np.array_equal(ref[code == v], merged[code == v])
        assert (merged[code == v] != c["L"][code == v]).any(1).mean() > 0.99 and (merged[code == v] != c["R"][code == v]).any(1).mean() > 0.99
    want = {"L": lambda y, x: c["L"][y, x], "R": lambda y, x: c["R"][y, x], "none": lambda y, x: np.array([0, 0, 0, 255], np.uint8)}
    for (y, x), w in c["expect"].items():
        assert code[y, x] == 150
        assert np.array_equal(ref[y, x], want[w](y, x)), ((y, x), w, ref[y, x])
        assert not np.array_equal(c["L"][y, x], c["R"][y, x])
    holes = code == 150
    assert holes[0].any() and holes[rows - 1].any() and holes[:, 0].any() and holes[:, cols - 1].any()
    none = holes & (ref == np.array([0, 0, 0, 255], np.uint8)).all(-1)
    assert int(none.sum()) >= 100 and int((holes & ~none).sum()) >= 100
    assert_bytes(ctx.stitch_gather(c["L"], c["R"], merged, mp), ref, "gather %dx%d" % (cols, rows))
