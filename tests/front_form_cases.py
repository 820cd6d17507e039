"""Inputs, case lists and plain-numpy restatements for the head of the pipeline: preprocess, pyramids, coarsest-level search.

Shared by tests/test_front_form_inputs.py (CPU tier: does each input reach what it is named for?) and tests/test_gpu_front_forms.py (the
kernels against the oracle, bit for bit).  Everything is built once per process and handed out read-only.  Shapes are w x h.
"""
import numpy as np

F32 = np.float32
T = F32(0.9)   # kUpdateAlphaThreshold

_cache = {}


def _frozen(key, make):
    if key not in _cache:
        v = make()
        for a in (v.values() if isinstance(v, dict) else v if isinstance(v, (tuple, list)) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


# ---- preprocess ----
PRE_CASES = [
    (512, 40, 0),     # dw = 256: exactly one 256-thread block
    (514, 40, 0),     # dw = 257: a one-thread second block
    (301, 203, 15),   # odd sizes, non-integer scales
    (41, 9, 2),       # the product's cols / 20 on a tiny image; dh = 4: vertical replication on every row
    (4, 4, 0),        # the 2 x 2 minimum
    (30, 12, 30),     # pad == cols: every branch of the wrap, at its extreme
]
PRE_BATCH = (130, 50, 6)   # three different images as one batch


def bgra_overshoot(cols, rows, seed):
    """uint8 noise in all four channels (alpha too), with what makes the fixed-point cubic leave 0..255 in both directions:
    a band of 2 x 2 blocks of 0 next to 255 across the whole width, both seams included (at a scale of 2 the taps are
    (-3/32, 19/32, 19/32, -3/32): 255 in the middle and 0 outside gives 303, the opposite -48), a band whose middle is a one-pixel
    checkerboard, and a band of noise whose first column is 0 and whose last is 255 (the seam of the wrap padding at full contrast), with
    two flat 16-pixel blocks of 0 and 255 side by side where the image is 40 wide or more."""
    r = np.random.default_rng(seed)
    img = r.integers(0, 256, (rows, cols, 4), dtype=np.uint8)
    y, x = np.mgrid[0:rows, 0:cols]
    b1, b2 = max(1, rows // 3), max(2, 2 * rows // 3)
    blocks = np.where(((x + seed) % 4 < 2) == (y % 4 < 2), 255, 0).astype(np.uint8)
    img[:b1] = blocks[:b1, :, None]
    cb = (((x + y) & 1) * 255).astype(np.uint8)
    img[b1:b2, cols // 4:max(cols // 4 + 1, 3 * cols // 4)] = cb[b1:b2, cols // 4:max(cols // 4 + 1, 3 * cols // 4), None]
    if cols >= 40:   # flat blocks of 0 next to 255, wide enough for whole windows of the pre-blur: the grey plane reaches 0 and 1 exactly
        x0 = cols // 2 - 16
        img[b2:, x0:x0 + 16] = 0
        img[b2:, x0 + 16:x0 + 32] = 255
    img[b2:, 0] = 0
    img[b2:, cols - 1] = 255
    return img


def pre_image(cols, rows, k=0):
    return _frozen(("bgra", cols, rows, k), lambda: bgra_overshoot(cols, rows, 7 * cols + rows + 1013 * k))


def wrap_pad(img, pad):
    """[last pad columns | image | first pad columns] (CPU/OpticalFlow.cpp:113-126), explicitly"""
    if pad == 0:
        return img
    cols = img.shape[1]
    return np.ascontiguousarray(np.concatenate([img[:, cols - pad:], img, img[:, :pad]], axis=1))


def pre_reference(orc, cols, rows, pad, k=0):
    return _frozen(("pre", cols, rows, pad, k), lambda: orc.preprocess(wrap_pad(pre_image(cols, rows, k), pad)))


# ---- pyramids ----
def pyramid_sizes(w0, h0):
    """PixFlow.hpp:137-151 on a given level 0, in float as the library computes it"""
    sizes = [(w0, h0)]
    while True:
        w, h = sizes[-1]
        nw = int(F32(w) * F32(0.9) + F32(0.5)); nh = int(F32(h) * F32(0.9) + F32(0.5))
        if (nw >= w and nh >= h) or nw <= 24 or nh <= 24:
            return sizes
        sizes.append((nw, nh))


def product_rule(sizes):
    """levels written by each launch of a solve's pyramid loop: three per launch from 40000 pixels down, two from 160000 down, while that
    many levels are left"""
    ks, l, n = [], 1, len(sizes)
    while l < n:
        px = sizes[l][0] * sizes[l][1]
        k = 3 if px <= 40000 and l + 2 < n else 2 if px <= 160000 and l + 1 < n else 1
        ks.append(k); l += k
    return ks


def forced_rule(sizes, k):
    ks, left = [], len(sizes) - 1
    while left > 0:
        ks.append(min(k, left)); left -= ks[-1]
    return ks


PYR_BIG = (500, 400)     # level 1 = 450 x 360 = 162000 px > 160000: the product's rule launches 1, then 2s, then 3s; last launch 3
PYR_END2 = (60, 60)      # 9 levels, all small: 3, 3 and a last launch of 2
PYR_END1 = (75, 80)      # 11 levels: 3, 3, 3 and a last launch of 1
PYR_NARROW = (300, 64)   # 300 -> 270 -> 243: the second 256-thread block disappears between two levels
PYR_BATCH = (130, 100)   # three pairs, twelve distinct planes
DENORM = F32(2.0) ** -135


def pyr_level0(w0, h0, pair=0):
    """(4, h0, w0): I0, I1, alpha0, alpha1 of one pair; every plane of every pair differs (the seed).  In each pair I1 carries a region of fp32
    denormals (random * 2^-135) and alpha0 a region of -0.0; both regions are a quarter of the plane per axis and lose a pixel per side
    and level on the way down."""
    def make():
        r = np.random.default_rng(100000 * pair + 1000 * w0 + h0)
        p = r.random((4, h0, w0)).astype(F32)
        p[p == 0] = F32(0.5)
        ys, xs = slice(h0 // 4, h0 // 2), slice(w0 // 8, w0 // 2)
        p[1, ys, xs] = (r.random((ys.stop - ys.start, xs.stop - xs.start)).astype(F32) + F32(0.5)) * DENORM
        p[2, slice(h0 // 2, 3 * h0 // 4), slice(w0 // 2, 7 * w0 // 8)] = F32(-0.0)
        return p
    return _frozen(("pyr0", w0, h0, pair), make)


def pyr_reference(orc, w0, h0, pair=0):
    """the oracle's pyramid, level by level: a list over levels of (4, h, w)"""
    def make():
        sizes = pyramid_sizes(w0, h0)
        levels = [pyr_level0(w0, h0, pair)]
        for (w, h) in sizes[1:]:
            levels.append(np.stack([orc.pyr_down(pl, w, h) for pl in levels[-1]]))
        return levels
    return _frozen(("pyr", w0, h0, pair), make)


# ---- coarsest-level search ----
SEARCH_SIZES = [
    (29, 25),    # the old case
    (64, 26),    # one 64-pixel segment exactly
    (65, 26),    # a one-pixel second segment: x0 = 64
    (150, 26),   # three segments, 3900 px: the ratio computed in the kernel
    (185, 27),   # 4995 px > 4096: the separate ratio launch, five chunks, a tail of 899 = 112 * 8 + 3
    (27, 194),   # tall, 5238 px: separate ratio
]
PCTS = (20, 50, 100)


def search_dist(pct):
    return (24 * pct + 50) // 100   # computeSearchDistance


def search_box(hint, pct):
    """computeSearchBox: bx, by, bw, bh"""
    dist = search_dist(pct); ortho = (dist + 4) // 8; thick = 2 * ortho + 1
    return {1: (0, -ortho, dist + 1, thick), 2: (-ortho, 0, thick, dist + 1), 3: (-dist, -ortho, dist + 1, thick), 4: (-ortho, -dist, thick, dist + 1)}[hint]


def _shift(img, sx, sy):
    """out[y + sy, x + sx] = img[y, x], edges replicated"""
    h, w = img.shape
    ys = np.clip(np.arange(h) - sy, 0, h - 1); xs = np.clip(np.arange(w) - sx, 0, w - 1)
    return img[np.ix_(ys, xs)]


def search_regions(w, h):
    """where the planted regions lie (slices y, x): `zero` = I0 = I1 = 0 (every candidate's SAD is exactly 0: ties), `a1zero` = alpha1 = 0,
    larger than patch + box where the level has the room, overlapping `zero` (0 / 0) and textured pixels (sad / 0); `thr` = alpha0
    exactly on the threshold; `holes` = alpha0 = 0.5"""
    if w >= h:
        zero = (slice(h // 2 - 6, h // 2 + 6), slice(w // 2 - 8, w // 2 + 8))
        a1z = (slice(max(0, h // 2 - 8), h // 2 + 8), slice(w // 2, min(w, w // 2 + 34)))
        thr = (slice(2, 8), slice(4, 14)); holes = (slice(h - 9, h - 3), slice(w - 12, w - 6))
    else:
        zero = (slice(h // 2 - 8, h // 2 + 8), slice(w // 2 - 6, w // 2 + 6))
        a1z = (slice(h // 2, min(h, h // 2 + 34)), slice(max(0, w // 2 - 8), w // 2 + 8))
        thr = (slice(4, 14), slice(2, 8)); holes = (slice(h - 12, h - 6), slice(w - 9, w - 3))
    return {"zero": zero, "a1zero": a1z, "thr": thr, "holes": holes}


def search_case(w, h, hint, pct, variant="noise", pair=0):
    """I0, I1, a0, a1 of one level.  I1 is I0 moved along the hint's direction, by 3 pixels in the first half of the level and by the whole
    search distance in the second, plus noise of 1 %; pairs 1 and 2 of a batch multiply I1 by 0.7 and 1.4.  variant "quant": I0 is a blocky field of four grey levels 0, 1/4, 1/2, 3/4 and I1 its
    shifted copy without noise, so candidates tie exactly."""
    def make():
        r = np.random.default_rng(((w * 1000 + h) * 10 + hint) * 1000 + pct + 77777 * pair + (500 if variant == "quant" else 0))
        dist = search_dist(pct)
        if variant == "quant":
            coarse = r.integers(0, 4, ((h + 2) // 3, (w + 2) // 3))
            i0 = (np.kron(coarse, np.ones((3, 3), np.int64))[:h, :w] * 0.25).astype(F32)
        else:
            i0 = r.random((h, w)).astype(F32)
        reg = search_regions(w, h)
        i0[reg["zero"]] = F32(0)
        ux, uy = {1: (1, 0), 2: (0, 1), 3: (-1, 0), 4: (0, -1)}[hint]
        near, far = _shift(i0, 3 * ux, 3 * uy), _shift(i0, dist * ux, dist * uy)
        i1 = near.copy()
        if w >= h:
            i1[:, w // 2:] = far[:, w // 2:]
        else:
            i1[h // 2:] = far[h // 2:]
        if variant != "quant":
            i1 = (i1 + F32(0.01) * r.standard_normal((h, w)).astype(F32)).astype(F32)
        if pair:   # every pair of a batch has an intensity ratio of its own, far from the others': I1 with the pair's gain
            i1 = (i1 * F32((1.0, 0.7, 1.4)[pair])).astype(F32)
        i1[reg["zero"]] = F32(0)
        a0 = (F32(0.91) + F32(0.09) * r.random((h, w)).astype(F32)).astype(F32)
        a0[reg["holes"]] = F32(0.5); a0[reg["thr"]] = T
        a1 = (F32(0.5) + F32(0.5) * r.random((h, w)).astype(F32)).astype(F32)
        a1[reg["a1zero"]] = F32(0)
        return {"i0": i0, "i1": i1, "a0": a0, "a1": a1}
    return _frozen(("search", w, h, hint, pct, variant, pair), make)


def search_reference(orc, w, h, hint, pct, variant="noise", pair=0):
    c = search_case(w, h, hint, pct, variant, pair)
    return _frozen(("search_ref", w, h, hint, pct, variant, pair), lambda: orc.adjust_initial_flow(c["i0"], c["i1"], c["a0"], c["a1"], hint, pct))


def ratio_reference(i0, i1, a0, a1):
    """computeIntensityRatio (PixFlow.hpp:190-205): sequential fp32 sums in row-major order, one fp32 division"""
    al = a0.ravel() * a1.ravel()
    with np.errstate(all="ignore"):
        return F32(np.cumsum(al * i0.ravel(), dtype=F32)[-1]) / F32(np.cumsum(al * i1.ravel(), dtype=F32)[-1])


def candidate_errors(c, x, y, hint, pct):
    """Plain numpy restatement of adjustInitialFlow (PixFlow.hpp:226-270) at ONE pixel: the zero-flow candidate's error (already times
    0.8) and the list of (dx, dy, error) of the box's candidates in the order the reference visits them.  fp32, sequential."""
    i0, a0, a1 = c["i0"], c["a0"], c["a1"]
    h, w = i0.shape
    i1eq = (c["i1"] * ratio_reference(i0, c["i1"], a0, a1) + F32(0)).astype(F32)
    dist = search_dist(pct)

    def err(i1x, i1y):
        sad, al = F32(0), F32(0)
        for dy in range(-2, 3):
            if not 0 <= y + dy < h:
                continue
            d1y = min(max(i1y + dy, 0), h - 1)
            for dx in range(-2, 3):
                if not 0 <= x + dx < w:
                    continue
                d1x = min(max(i1x + dx, 0), w - 1)
                sad = F32(sad + np.abs(F32(i0[y + dy, x + dx] - i1eq[d1y, d1x])))
                al = F32(al + F32(a0[y + dy, x + dx] * a1[d1y, d1x]))
        fx, fy = float(i1x - x), float(i1y - y)
        length = F32(np.sqrt(fx * fx + fy * fy))
        with np.errstate(all="ignore"):
            return F32(F32(sad / al) * F32(F32(1) + F32(length / F32(dist))))
    bx, by, bw, bh = search_box(hint, pct)
    with np.errstate(all="ignore"):
        zero = F32(F32(0.8) * err(x, y))
    cands = [(dx, dy, err(x + dx, y + dy)) for dy in range(by, by + bh) for dx in range(bx, bx + bw) if 0 <= x + dx < w and 0 <= y + dy < h]
    return zero, cands


def search_pick(zero, cands, better=lambda best, e: best > e):
    """the reference's selection over candidate_errors' output: (dx, dy) of the winner"""
    best, pick = zero, (0, 0)
    for dx, dy, e in cands:
        if better(best, e):
            best, pick = e, (dx, dy)
    return pick
