"""The head of the pipeline against the oracle, bit pattern by bit pattern, in the forms a solve runs it.

k_downscale_gray + the 5 x 5 pre-blur (batched: one caller pointer per pair, planes in slabs), k_pyr_down4 with four planes times the
pairs, k_pyr_chain at every depth, k_intensity_ratio, k_adjust_initial_flow beyond its first 64-pixel segment, above the 4096 pixels up
to which it sums the ratio itself, with the widest search boxes, on batches.  The stage entries fill their slabs with 0xFF bytes and
return whole padded planes, so a write outside its place shows.  Inputs and what each reaches: tests/front_form_cases.py,
tests/test_front_form_inputs.py.  Shapes are w x h.
"""
import numpy as np
import pytest

import front_form_cases as fc

pytestmark = pytest.mark.gpu

F32 = np.float32
UNWRITTEN = 0xFFFFFFFF


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


def assert_unwritten(tail, what):
    rest = bits(tail)
    assert (rest == UNWRITTEN).all(), "%s: %d words outside the plane were written" % (what, int((rest != UNWRITTEN).sum()))


# ---- downscale + pre-blur ----
def check_pre(orc, got, cols, rows, pad, ks):
    g, a, (dw, dh) = got
    for p, k in enumerate(ks):
        I, A = fc.pre_reference(orc, cols, rows, pad, k)
        assert I.shape == (dh, dw)
        for name, plane, ref in (("alpha", a[p], A), ("gray", g[p], I)):
            what = "%s of image %d, %dx%d pad %d" % (name, p, cols, rows, pad)
            assert_bits(plane[:dw * dh].reshape(dh, dw), ref, what)
            assert_unwritten(plane[dw * dh:], what)


@pytest.mark.parametrize("cols,rows,pad", fc.PRE_CASES)
def test_preprocess_block_edges_wrap_and_clamp(ctx, orc, cols, rows, pad):
    """one image through the lone form of the solver's two launches (stride 0, the image behind a pointer table)"""
    check_pre(orc, ctx.stage_preprocess_batch(fc.pre_image(cols, rows)[None], pad), cols, rows, pad, [0])


@pytest.mark.parametrize("cols,rows,pad", fc.PRE_CASES)
def test_preprocess_older_entry_agrees(ctx, orc, cols, rows, pad):
    I, A = fc.pre_reference(orc, cols, rows, pad)
    g, a = ctx.stage_preprocess(fc.pre_image(cols, rows), pad)
    assert_bits(a, A, "alpha"); assert_bits(g, I, "gray")


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1), (1, 1, 0)])
def test_preprocess_three_images_in_slabs(ctx, orc, order):
    cols, rows, pad = fc.PRE_BATCH
    imgs = np.stack([fc.pre_image(cols, rows, k) for k in order])
    check_pre(orc, ctx.stage_preprocess_batch(imgs, pad), cols, rows, pad, order)


@pytest.mark.parametrize("pad", [-1, 31, 1000])
@pytest.mark.parametrize("batched", [False, True])
def test_preprocess_refuses_a_pad_the_wrap_cannot_reach(ctx, pf, pad, batched):
    """the kernel wraps a tap once (+- cols): pad > cols would leave it outside the row.  Refused before any launch."""
    img = fc.pre_image(30, 12)
    with pytest.raises(pf.PanoflowError, match="pad"):
        if batched:
            ctx.stage_preprocess_batch(img[None], pad)
        else:
            ctx.stage_preprocess(img, pad)


# ---- pyramids ----
def check_pyramid(orc, out, w0, h0, pairs, what):
    sizes, off = out["sizes"], out["off"]
    assert sizes == fc.pyramid_sizes(w0, h0)
    for p, pair in enumerate(pairs):
        ref = fc.pyr_reference(orc, w0, h0, pair)
        for k in range(4):
            plane = out["planes"][p, k]
            written = np.zeros(plane.shape[0], bool)
            for l, (w, h) in enumerate(sizes):
                o = int(off[l]); written[o:o + w * h] = True
                assert_bits(plane[o:o + w * h].reshape(h, w), ref[l][k], "%s: pair %d plane %d level %d (%dx%d)" % (what, p, k, l, w, h))
            assert_unwritten(plane[~written], "%s: pair %d plane %d" % (what, p, k))


def expected_ks(sizes, mode):
    return [1] * (len(sizes) - 1) if mode == 0 else fc.product_rule(sizes) if mode == 1 else fc.forced_rule(sizes, mode)


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_pyramid_every_chaining_mode(ctx, orc, mode):
    """500 x 400: the product's rule (mode 1) launches one level, then two at a time, then three; the four modes write the same planes"""
    w0, h0 = fc.PYR_BIG
    out = ctx.stage_pyramid(fc.pyr_level0(w0, h0)[None], mode)
    assert out["ks"] == expected_ks(out["sizes"], mode)
    if mode == 1:
        ks = out["ks"]
        assert ks[0] == 1 and ks[1] == 2 and 3 in ks and ks == sorted(ks[:-1]) + ks[-1:]
    check_pyramid(orc, out, w0, h0, [0], "mode %d" % mode)


@pytest.mark.parametrize("size,last", [(fc.PYR_END2, 2), (fc.PYR_END1, 1), (fc.PYR_BATCH, 1)])
def test_pyramid_product_rule_last_launch(ctx, orc, size, last):
    out = ctx.stage_pyramid(fc.pyr_level0(*size)[None], 1)
    assert out["ks"] == fc.product_rule(out["sizes"]) and out["ks"][-1] == last and out["ks"][0] == 3
    check_pyramid(orc, out, size[0], size[1], [0], "%dx%d" % size)


def test_pyramid_block_count_changes_between_levels(ctx, orc):
    """300 -> 270 -> 243 wide, one level per launch: two 256-thread blocks per row, then one"""
    w0, h0 = fc.PYR_NARROW
    out = ctx.stage_pyramid(fc.pyr_level0(w0, h0)[None], 0)
    assert [s[0] for s in out["sizes"][:3]] == [300, 270, 243]
    check_pyramid(orc, out, w0, h0, [0], "300x64")


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("pairs", [(0, 1, 2), (2, 1)])
def test_pyramid_pairs_in_slabs(ctx, orc, mode, pairs):
    """twelve distinct planes (denormals in one, -0.0 in another): plane = z & 3 and pair = z >> 2 in the chain kernel, z % 4 and z / 4 in
    the one-level kernel, each pair's levels at the pair's own offsets"""
    w0, h0 = fc.PYR_BATCH
    out = ctx.stage_pyramid(np.stack([fc.pyr_level0(w0, h0, p) for p in pairs]), mode)
    assert out["ks"] == expected_ks(out["sizes"], mode)
    check_pyramid(orc, out, w0, h0, pairs, "mode %d, pairs %s" % (mode, pairs))


# ---- intensity ratio ----
def ratio_inputs(n, pair=0):
    """the planes of the 185 x 27 search case, cut or tiled to n elements"""
    c = fc.search_case(185, 27, 1 + pair, 20, pair=pair)
    return [np.resize(c[k].ravel(), n) for k in ("i0", "i1", "a0", "a1")]


@pytest.mark.parametrize("n", [1, 7, 8, 1024, 1025, 4995])
def test_intensity_ratio_is_the_sequential_sum(ctx, n):
    v = ratio_inputs(n)
    got = ctx.stage_intensity_ratio(*[a[None] for a in v])
    assert_bits(got, np.array([fc.ratio_reference(*v)], F32), "ratio of %d elements" % n)


@pytest.mark.parametrize("n", [4995, 1031])
def test_intensity_ratio_three_pairs(ctx, n):
    v = [ratio_inputs(n, p) for p in range(3)]
    ref = np.array([fc.ratio_reference(*x) for x in v], F32)
    assert len(set(bits(ref).tolist())) == 3
    got = ctx.stage_intensity_ratio(*[np.stack([x[k] for x in v]) for k in range(4)])
    assert_bits(got, ref, "ratios of three pairs")


def test_intensity_ratio_of_nothing_visible(ctx):
    """alpha 0 everywhere: 0 / 0, as the reference"""
    z = np.zeros((1, 100), F32); o = np.ones((1, 100), F32)
    assert np.isnan(ctx.stage_intensity_ratio(o, o, z, o)[0])


# ---- coarsest-level search ----
def run_search(ctx, orc, w, h, hint, pct, variant, pairs=(0,)):
    cs = [fc.search_case(w, h, hint, pct, variant, p) for p in pairs]
    got = ctx.stage_adjust_initial_flow_batch(*[np.stack([c[k] for c in cs]) for k in ("i0", "i1", "a0", "a1")], hint, pct)
    for i, p in enumerate(pairs):
        what = "%dx%d hint %d max_pct %d %s pair %d" % (w, h, hint, pct, variant, p)
        assert_bits(got[i, :2 * w * h].reshape(h, w, 2), fc.search_reference(orc, w, h, hint, pct, variant, p), what)
        assert_unwritten(got[i, 2 * w * h:], what)


@pytest.mark.parametrize("pct", fc.PCTS)
@pytest.mark.parametrize("hint", [1, 2, 3, 4])
@pytest.mark.parametrize("w,h", fc.SEARCH_SIZES)
def test_search_segments_ratio_paths_and_boxes(ctx, orc, w, h, hint, pct):
    run_search(ctx, orc, w, h, hint, pct, "noise")


@pytest.mark.parametrize("pct", fc.PCTS)
@pytest.mark.parametrize("hint", [1, 2, 3, 4])
@pytest.mark.parametrize("w,h", [(65, 26), (150, 26), (185, 27)])
def test_search_exact_ties(ctx, orc, w, h, hint, pct):
    """four grey levels and a block of zeros: candidates tie exactly, the reference's `>` and its order of candidates decide"""
    run_search(ctx, orc, w, h, hint, pct, "quant")


@pytest.mark.parametrize("pct", [20, 100])
@pytest.mark.parametrize("hint", [1, 2, 3, 4])
@pytest.mark.parametrize("w,h", [(185, 27), (150, 26)])
def test_search_three_pairs_in_slabs(ctx, orc, w, h, hint, pct):
    """185 x 27: each pair's ratio goes through its own slab's scratch word.  150 x 26: the kernel sums the ratio itself and must not read
    the scratch, which holds 0xFF bytes (a NaN)."""
    run_search(ctx, orc, w, h, hint, pct, "noise", pairs=(0, 1, 2))


@pytest.mark.parametrize("w,h", [(29, 25), (185, 27)])
def test_search_older_entry_agrees(ctx, orc, w, h):
    c = fc.search_case(w, h, 3, 50)
    got = ctx.stage_adjust_initial_flow(c["i0"], c["i1"], c["a0"], c["a1"], 3, 50)
    assert_bits(got, fc.search_reference(orc, w, h, 3, 50), "%dx%d" % (w, h))
