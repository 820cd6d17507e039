"""Do the inputs of tests/test_gpu_front_forms.py reach what they are named for?  Asserted on the builders (tests/front_form_cases.py) and
the oracle alone: no GPU.  A case whose input misses its form would pass on the GPU for the wrong reason."""
import numpy as np
import pytest

import front_form_cases as fc

F32 = np.float32


def u32(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- preprocess ----
@pytest.mark.parametrize("cols,rows,pad", fc.PRE_CASES + [fc.PRE_BATCH])
def test_overshoot_image_reaches_both_clamps(orc, cols, rows, pad):
    """alpha (no pre-blur behind it) sits at 0 and at 255 and strictly between; so does grey wherever the image has room for a whole
    5 x 5 window of the pre-blur inside a saturated area.  The 4 x 4 image has room for neither: it is there for the 2 x 2 minimum."""
    img = fc.pre_image(cols, rows)
    assert (img[..., 3] != img[..., 0]).any() and (img[..., 3] != 255).any()   # alpha is a channel of noise like the others, not a constant 255
    I, A = fc.pre_reference(orc, cols, rows, pad)
    if cols * rows > 16:
        assert (A == 0).any() and (A == 1).any() and ((A > 0) & (A < 1)).any()
    if cols >= 40 and rows >= 40:
        assert (I == 0).any() and (I == 1).any() and ((I > 0) & (I < 1)).any()


def test_overshoot_image_leaves_0_255_before_the_clamp(orc):
    """the cubic itself, in float on the same image, leaves 0..255 in both directions: what the 8-bit result holds at 0 / 255 there is the clamp"""
    cols, rows, pad = 301, 203, 15
    p = fc.wrap_pad(fc.pre_image(cols, rows), pad)
    dw, dh = int(F32(p.shape[1]) * F32(0.5)), int(F32(rows) * F32(0.5))
    f = orc.resize_cubic_f32(p.astype(F32), dw, dh)
    u = orc.resize_cubic_u8(p, dw, dh)
    assert f.min() < -20 and f.max() > 275
    assert (u[f < -1] == 0).all() and (u[f > 256] == 255).all()


def test_batch_images_differ():
    a, b, c = (fc.pre_image(*fc.PRE_BATCH[:2], k=k) for k in range(3))
    assert (a != b).mean() > 0.5 and (a != c).mean() > 0.5 and (b != c).mean() > 0.5


def test_block_edges():
    for (cols, rows, pad), dw in zip(fc.PRE_CASES[:2], (256, 257)):
        assert int(F32(cols + 2 * pad) * F32(0.5)) == dw


# ---- pyramids ----
def test_pyramid_launch_plans():
    big = fc.product_rule(fc.pyramid_sizes(*fc.PYR_BIG))
    assert big[0] == 1 and 2 in big and 3 in big and big.index(2) < big.index(3)   # 1, then 2, then 3
    s1 = fc.pyramid_sizes(*fc.PYR_BIG)[1]
    assert s1 == (450, 360) and s1[0] * s1[1] > 160000
    assert fc.product_rule(fc.pyramid_sizes(*fc.PYR_END2))[-1] == 2
    assert fc.product_rule(fc.pyramid_sizes(*fc.PYR_END1))[-1] == 1
    assert [s[0] for s in fc.pyramid_sizes(*fc.PYR_NARROW)[:3]] == [300, 270, 243]   # two blocks, two blocks, one block of 256 threads
    n = len(fc.pyramid_sizes(*fc.PYR_BATCH))
    assert n >= 8 and fc.forced_rule(fc.pyramid_sizes(*fc.PYR_BATCH), 3)[0] == 3


def test_pyramid_sizes_are_the_oracles(orc):
    for s in (fc.PYR_BIG, fc.PYR_END2, fc.PYR_END1, fc.PYR_NARROW, fc.PYR_BATCH):
        assert fc.pyramid_sizes(*s) == orc.pyramid_sizes(*s)


def test_pyramid_scales_differ_between_levels():
    """a chain launch takes each level's own scale: in the first three-level launch of the batch case the second and the third level differ
    in it on both axes (100 / 90 and 90 / 81 do not: the first and the second share their vertical scale)"""
    z = fc.pyramid_sizes(*fc.PYR_BATCH)
    assert z[1][1] / z[2][1] != z[2][1] / z[3][1] and z[1][0] / z[2][0] != z[2][0] / z[3][0]
    assert z[0][0] / z[1][0] != z[1][0] / z[2][0]


def test_twelve_planes_differ_and_special_regions_survive(orc):
    w0, h0 = fc.PYR_BATCH
    planes = np.concatenate([fc.pyr_level0(w0, h0, p) for p in range(3)])
    assert len({pl.tobytes() for pl in planes}) == 12
    l1 = fc.pyr_reference(orc, w0, h0, 0)[1]
    den = np.abs(l1[1]); den = den[(den > 0) & (den < F32(2.0) ** -126)]
    assert den.size > 50                                  # denormals at level 1 ...
    assert (u32(l1[2]) == 0x80000000).sum() > 50          # ... and -0.0
    mid = fc.pyr_reference(orc, w0, h0, 0)[6]               # (the regions lose a pixel per side and level: they last twelve levels)
    assert ((np.abs(mid[1]) > 0) & (np.abs(mid[1]) < F32(2.0) ** -126)).sum() > 50 and (u32(mid[2]) == 0x80000000).sum() > 50


# ---- search ----
SEARCH_ALL = [(w, h, hint, pct, v) for (w, h) in fc.SEARCH_SIZES for pct in fc.PCTS for hint in (1, 2, 3, 4) for v in ("noise", "quant")]


def test_search_sizes_take_their_paths():
    px = {s: s[0] * s[1] for s in fc.SEARCH_SIZES}
    assert px[(150, 26)] <= 4096 < px[(185, 27)] and px[(27, 194)] > 4096
    assert px[(185, 27)] == 4995 and 4995 - 4 * 1024 == 899 == 112 * 8 + 3
    assert (64 + 63) // 64 == 1 and (65 + 63) // 64 == 2 and (150 + 63) // 64 == 3
    assert fc.search_dist(100) == 24 and fc.search_box(1, 100)[2:] == (25, 7) and fc.search_box(2, 100)[2:] == (7, 25)


@pytest.mark.parametrize("w,h", fc.SEARCH_SIZES)
def test_search_moves(orc, w, h):
    for (ww, hh, hint, pct, v) in SEARCH_ALL:
        if (ww, hh) != (w, h):
            continue
        f = fc.search_reference(orc, w, h, hint, pct, v)
        assert (f != 0).any(-1).mean() > 0.2, (hint, pct, v)
        c = fc.search_case(w, h, hint, pct, v)
        assert (f[c["a0"] <= fc.T] == 0).all()
        # max_pct 100: the half of the level that moved by the whole distance, 24, has to be wider than that along the hint's axis for a pixel
        # to find its patch there.  Levels of 64 and more along that axis have the room, in both variants; on 25..29 pixels the moved half is
        # mostly replicated edge, and whether the far corner of the box wins is left to the content (with noise it does on 26 and 27 rows).
        along = w if hint in (1, 3) else h
        if pct == 100 and (along >= 64 or (v == "noise" and (w, h) != (29, 25))):
            assert np.abs(f).max() == fc.search_dist(pct), (hint, pct, v)   # the far corner of the widest box
        # around the block on the threshold the search does move: `>=` there would show
        ys, xs = fc.search_regions(w, h)["thr"]
        ring = f[max(0, ys.start - 2):ys.stop + 2, max(0, xs.start - 2):xs.stop + 2]
        assert (ring != 0).any(), (hint, pct, v)


@pytest.mark.parametrize("w,h", [(65, 26), (150, 26), (185, 27)])
@pytest.mark.parametrize("hint", [1, 2, 3, 4])
def test_quantised_variant_ties(orc, w, h, hint):
    """at the middle of the zero block every candidate's error is exactly 0: the zero flow ties with each of them, `>` keeps it, `>=` would
    take the last one.  And the restatement agrees with the oracle at that pixel and at a textured one."""
    pct = 20
    c = fc.search_case(w, h, hint, pct, "quant")
    ref = fc.search_reference(orc, w, h, hint, pct, "quant")
    ys, xs = fc.search_regions(w, h)["zero"]
    x, y = xs.start + 3, (ys.start + ys.stop) // 2
    assert c["a0"][y, x] > fc.T and c["a1"][y, x] > 0
    zero, cands = fc.candidate_errors(c, x, y, hint, pct)
    best = min([zero] + [e for _, _, e in cands])
    assert zero == best == 0 and sum(e == best for _, _, e in cands) >= 2          # the best ties with later candidates
    assert fc.search_pick(zero, cands) == (0, 0) == tuple(ref[y, x])
    assert fc.search_pick(zero, cands, lambda b, e: b >= e) != (0, 0)
    for (tx, ty) in ((5, h // 2), (w - 6, h // 2), (w // 3, 3)):                    # textured pixels, a segment's end included
        if c["a0"][ty, tx] > fc.T:
            z, cs = fc.candidate_errors(c, tx, ty, hint, pct)
            assert fc.search_pick(z, cs) == tuple(ref[ty, tx]), (tx, ty)


@pytest.mark.parametrize("variant", ["noise", "quant"])
def test_zero_alpha1_block_gives_non_finite_penalties(variant):
    w, h, hint, pct = 185, 27, 1, 20
    c = fc.search_case(w, h, hint, pct, variant)
    ys, xs = fc.search_regions(w, h)["a1zero"]
    assert ys.stop - ys.start >= 5 + 2 and xs.stop - xs.start >= 5 + 5 + 20   # larger than the patch plus the box of pct 20 .. 100 along x
    kinds = set()
    for x in (xs.start + 4, xs.start + 12):   # inside the zero block of I0 / I1 (0 / 0), and outside it (sad / 0)
        zero, cands = fc.candidate_errors(c, x, (ys.start + ys.stop) // 2, hint, pct)
        kinds |= {"nan" if np.isnan(e) else "inf" if np.isinf(e) else "finite" for e in [zero] + [e for _, _, e in cands]}
    assert "nan" in kinds and "inf" in kinds


def test_ratio_reference_is_sequential():
    """a pairwise or chunked sum of the same products differs from the sequential one in the last place on these inputs"""
    c = fc.search_case(185, 27, 1, 20)
    al = c["a0"].ravel() * c["a1"].ravel()
    seq = np.cumsum(al * c["i0"].ravel(), dtype=F32)[-1]
    acc = F32(0)
    for v in (al * c["i0"].ravel())[:300]:
        acc = F32(acc + v)
    assert acc == np.cumsum(al * c["i0"].ravel(), dtype=F32)[299]
    halves = F32(0)
    for k in range(0, al.size, 1024):
        ch = al[k:k + 1024] * c["i0"].ravel()[k:k + 1024]
        m = ch.size // 2
        halves = F32(halves + F32(np.cumsum(ch[:m], dtype=F32)[-1] + np.cumsum(ch[m:], dtype=F32)[-1]))
    assert halves != seq
