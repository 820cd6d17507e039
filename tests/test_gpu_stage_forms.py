"""Every FORM of the front-end and stencil kernels against the oracle, bit pattern by bit pattern (+0 and -0 differ here).

tests/test_gpu_stages.py runs each kernel family at one arbitrary shape, which picks one form.  These cases are chosen by the kernels'
geometry instead: interior and rim tiles of the fused Gaussian 15 (64 x 32 tiles, ring of 7: the first interior tile exists at 135 x 71),
its persistent tile walk (block cap), its UPS / MED instantiations, batch slabs; the float4 store of the tiled median (even widths) and
its tile edges; several tile columns of the cubic upsample and the final flow; gradients and gate + boxes + count on whole level tables
(levels sharing a 1024-element chunk, w > 1024, w = 1024, levels across several 16384-pixel gate blocks), the boxes and the count
themselves, which no solve can see: a box that is too large gives the same flows.

References come from the oracle; boxes, count and gate bytes, for which it has no call, from numpy.  Shapes are w x h.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F32 = np.float32
T = F32(0.9)                       # kUpdateAlphaThreshold: gated means alpha0 > T and alpha1 > T
MUL = float(F32(1.0) / F32(0.9))   # the inter-level factor of a solve (1.0f / pyrScaleFactor)
UNWRITTEN = 0xFFFFFFFF             # the stage entries fill the device planes with 0xFF bytes before a kernel runs


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


def _rect(r, w, h):
    """a random rectangle: a third of the plane per axis, 16 where that is narrower (a whole Gaussian window inside it) but never more than
    half the axis, at least one pixel"""
    rw, rh = max(1, w // 3, min(16, w // 2)), max(1, h // 3, min(16, h // 2))
    x0, y0 = int(r.integers(0, w - rw + 1)), int(r.integers(0, h - rh + 1))
    return slice(y0, y0 + rh), slice(x0, x0 + rw)


def _gap(a, b):
    """pixels between two rectangles (the larger of the gaps along x and y; <= 0: they touch or overlap)"""
    return max(max(a[k].start - b[k].stop, b[k].start - a[k].stop) for k in (0, 1))


def flow_plane(w, h, seed):
    """standard_normal flow with planted regions of +0, -0, a constant and values quantised to halves (ties for the median), and single
    denormals of both signs (some inside the -0 region, where they survive the Gaussian's products).
    No 5 x 5 window holds zeros of BOTH signs: the median of such a window is a zero whose sign is the reference's to choose -- OpenCV's
    sorting network keeps or swaps two equal operands depending on whether the pixel goes through its vector or its scalar body, the
    oracle's std::nth_element has an order of its own -- so there is no reference to hold the kernels to
    (test_median5_zeros_of_both_signs says what they do).  The +0 and the -0 region therefore lie at least five pixels apart; a plane too
    small for that gets one of them, by the seed's parity; and the quantised region has no zeros."""
    r = np.random.default_rng(seed)
    f = r.standard_normal((h, w, 2)).astype(F32)
    f[f == 0] = F32(1.0)
    ys, xs = _rect(r, w, h)
    q = np.round(f[ys, xs] * 2) / 2
    q[q == 0] = F32(0.5)
    f[ys, xs] = q
    ys, xs = _rect(r, w, h); f[ys, xs] = F32(1.25)
    pz, nz = next((c for c in ((_rect(r, w, h), _rect(r, w, h)) for _ in range(200)) if _gap(*c) >= 5), (None, None))
    if nz is None:
        pz, nz = (_rect(r, w, h), None) if seed % 2 == 0 else (None, _rect(r, w, h))
    if pz is not None:
        f[pz] = F32(0.0)
    if nz is not None:
        f[nz] = F32(-0.0)
    zy, zx = nz if nz is not None else pz
    for k in (range(6) if w * h >= 64 else (5,)):   # (a plane of a few pixels keeps its zero)
        y, x = int(r.integers(0, h)), int(r.integers(0, w))
        if k < 3:   # inside a zero region
            y, x = int(r.integers(zy.start, zy.stop)), int(r.integers(zx.start, zx.stop))
        f[y, x, k % 2] = F32(1e-41) if k % 3 else F32(-3e-39)
    return f


def alpha_plane(w, h, seed):
    r = np.random.default_rng(seed)
    a = r.random((h, w)).astype(F32)
    ys, xs = _rect(r, w, h); a[ys, xs] = F32(0.0)
    ys, xs = _rect(r, w, h); a[ys, xs] = F32(1.0)
    return a


_cache = {}


def g15_case(orc, w, h, k=0):
    """inputs and oracle results of plane k at w x h, computed once per module run and never modified"""
    key = ("g15", w, h, k)
    if key not in _cache:
        f = flow_plane(w, h, 1000 * w + h + 7919 * k)
        a0 = alpha_plane(w, h, 3 * w + h + 31 * k); a1 = alpha_plane(w, h, 5 * w + 7 * h + 17 * k)
        c = {"f": f, "a0": a0, "a1": a1, "plain": orc.gaussian_blur(f, 15, 8.0), "mix": orc.diffusion(a0, a1, f)}
        for v in c.values():
            v.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def run_g15(ctx, form, cases, **kw):
    f = np.stack([c["f"] for c in cases])
    if form == "plain":
        return ctx.stage_gauss15_form("plain", f, **kw)
    return ctx.stage_gauss15_form(form, f, np.stack([c["a0"] for c in cases]), np.stack([c["a1"] for c in cases]), **kw)


# ---- Gaussian 15, plain and MIX ----
G15_SHAPES = [
    (135, 71),   # exactly one interior tile (x0 = 64, y0 = 32: 64 + 71 = 135, 32 + 39 = 71)
    (134, 70),   # one short on both axes: rim tiles only
    (199, 103),  # 4 x 4 tiles, four interior, rim tiles 7 wide and 7 high
    (64, 300),   # a single tile column
    (300, 33),   # a single tile row (+ one row)
    (8, 8), (7, 9), (3, 40), (40, 3), (2, 2),   # repeated reflection inside the ring of 7
]


@pytest.mark.parametrize("form", ["plain", "mix"])
@pytest.mark.parametrize("w,h", G15_SHAPES)
def test_gauss15_interior_and_rim_tiles(ctx, orc, form, w, h):
    c = g15_case(orc, w, h)
    assert_bits(run_g15(ctx, form, [c])[0], c[form], "%s %dx%d" % (form, w, h))


@pytest.mark.parametrize("form", ["plain", "mix"])
@pytest.mark.parametrize("cap", [1, 2, 3])
def test_gauss15_persistent_tile_walk(ctx, orc, form, cap):
    """16 tiles on 1, 2 or 3 blocks: the next tile is prefetched (pre[], coef[]) while the current one is computed.  With 3, block 0 walks
    tiles 0, 3, 6, 9, 12, 15 = rim, rim, interior, interior, rim, rim: the prefetch crosses the two forms in both directions."""
    c = g15_case(orc, 199, 103)
    assert_bits(run_g15(ctx, form, [c], max_blocks=cap)[0], c[form], "%s cap %d" % (form, cap))


@pytest.mark.parametrize("form", ["plain", "mix"])
def test_gauss15_three_planes_in_slabs(ctx, orc, form):
    cases = [g15_case(orc, 199, 103, k) for k in range(3)]
    got = run_g15(ctx, form, cases)
    for k in range(3):
        assert_bits(got[k], cases[k][form], "%s plane %d" % (form, k))


def test_gauss15_plane_of_negative_zero(ctx, orc):
    """OpenCV's column pass starts from `k * centre + 0`: a window of -0 gives +0.  Interior and rim tiles."""
    f = np.full((71, 135, 2), -0.0, F32)
    ref = orc.gaussian_blur(f, 15, 8.0)
    assert not bits(ref).any()   # the oracle: +0 everywhere
    assert_bits(ctx.stage_gauss15_form("plain", f), ref, "plane of -0")


# ---- UPS: the upsample inside the Gaussian's tile loader ----
UPS_TARGETS = [(199, 103), (135, 71), (29, 26), (3, 3)]


def _coarse(n):
    return 2 if n == 3 else int(n * 0.9 + 0.5)


def ups_case(orc, w, h, k=0):
    key = ("ups", w, h, k)
    if key not in _cache:
        sw, sh = _coarse(w), _coarse(h)
        coarse = flow_plane(sw, sh, 77 * w + h + 101 * k)
        up = orc.resize_cubic_f32(coarse, w, h) * F32(MUL) + F32(0)
        c = {"coarse": coarse, "up": up, "dst": orc.gaussian_blur(up, 15, 8.0)}
        for v in c.values():
            v.setflags(write=False)
        _cache[key] = c
    return _cache[key]


@pytest.mark.parametrize("w,h", UPS_TARGETS)
def test_gauss15_upsample_form(ctx, orc, w, h):
    c = ups_case(orc, w, h)
    dst, up = ctx.stage_gauss15_form("ups", c["coarse"], size=(w, h), mul=MUL)
    assert_bits(up, c["up"], "up_out %dx%d" % (w, h))
    assert_bits(dst, c["dst"], "dst %dx%d" % (w, h))


def test_gauss15_upsample_form_two_planes(ctx, orc):
    cases = [ups_case(orc, 135, 71, k) for k in range(2)]
    dst, up = ctx.stage_gauss15_form("ups", np.stack([c["coarse"] for c in cases]), size=(135, 71), mul=MUL)
    for k in range(2):
        assert_bits(up[k], cases[k]["up"], "up_out plane %d" % k)
        assert_bits(dst[k], cases[k]["dst"], "dst plane %d" % k)


# ---- MED + MIX: the median inside the diffusion's tile loader ----
@pytest.mark.parametrize("w,h", UPS_TARGETS)
def test_gauss15_median_mix_form(ctx, orc, w, h):
    c = g15_case(orc, w, h)
    ref = orc.diffusion(c["a0"], c["a1"], orc.median5(c["f"]))
    assert_bits(run_g15(ctx, "med_mix", [c])[0], ref, "median + mix %dx%d" % (w, h))


# ---- median 5: the entry runs the direct and the LDS-tiled kernel and refuses if they differ ----
@pytest.mark.parametrize("w,h", [
    (94, 70),    # even width: the tiled form's float4 store, on whole and on cut tiles (94 = 2 * 32 + 30)
    (32, 16), (33, 17), (31, 15), (64, 32),   # the 32 x 16 tile exactly, one over, one under, 2 x 2 tiles
    (130, 5), (5, 5), (3, 2), (2, 2),         # rows / columns fewer than the window: replicate on both sides at once
])
def test_median5_tile_edges_and_store_forms(ctx, orc, w, h):
    f = flow_plane(w, h, 13 * w + h)
    assert_bits(ctx.stage_median5(f), orc.median5(f), "median %dx%d" % (w, h))


def _median5_total_order(f):
    """plain numpy: rank 13 of each 5 x 5 window (replicate border) in the total order of the bit patterns, where -0 < +0"""
    h, w, _ = f.shape
    u = bits(f)
    key = np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000))
    kp = np.pad(key, ((2, 2), (2, 2), (0, 0)), mode="edge")
    med = np.sort(np.stack([kp[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5)]), axis=0)[12]
    return np.where(med >> 31 == 1, med & np.uint32(0x7FFFFFFF), ~med).view(F32)


@pytest.mark.parametrize("w,h", [(33, 17), (94, 70)])
def test_median5_zeros_of_both_signs(ctx, orc, w, h):
    """Windows that hold +0 and -0 and whose median is a zero: its VALUE is the oracle's; its sign is not the reference's to give (see
    flow_plane), so plain numpy states what the kernels do: v_min / v_max order -0 below +0, the selection network returns rank 13 of that
    total order.  Direct and tiled form (the entry compares them), and the form inside the diffusion's tile loader."""
    r = np.random.default_rng(w)
    f = r.choice(np.array([0.0, -0.0, 0.0, -0.0, -1.0, 1.0, 0.5], F32), size=(h, w, 2)).astype(F32)
    med = _median5_total_order(f)
    assert np.array_equal(med, orc.median5(f))          # the same values ...
    assert (bits(med) != bits(orc.median5(f))).any()    # ... and this input does reach the zeros whose sign is open
    assert_bits(ctx.stage_median5(f), med, "median %dx%d" % (w, h))
    a0, a1 = alpha_plane(w, h, w + 1), alpha_plane(w, h, w + 2)
    assert_bits(ctx.stage_gauss15_form("med_mix", f, a0, a1), orc.diffusion(a0, a1, med), "median + mix %dx%d" % (w, h))


# ---- cubic upsample: 64 x 16 tiles ----
@pytest.mark.parametrize("sw,sh,dw,dh", [(58, 40, 64, 44), (59, 41, 65, 45), (117, 90, 130, 100), (2, 2, 3, 3)])
def test_upsample_cubic_tile_columns(ctx, orc, sw, sh, dw, dh):
    f = flow_plane(sw, sh, 17 * sw + sh)
    ref = orc.resize_cubic_f32(f, dw, dh) * F32(MUL) + F32(0)
    assert_bits(ctx.stage_upsample_cubic(f, dw, dh, MUL), ref, "%dx%d -> %dx%d" % (sw, sh, dw, dh))


def test_upsample_cubic_refuses_what_no_pyramid_asks_for(ctx, pf):
    """The kernel's LDS holds the source rows of an upsampling tile (source / destination rows <= 1.1875); there is no other form."""
    f = np.zeros((20, 10, 2), F32)
    with pytest.raises(pf.PanoflowError, match="1.1875"):
        ctx.stage_upsample_cubic(f, 10, 16, MUL)   # 20 / 16 = 1.25


# ---- final flow: 64 x 16 tiles over the cropped columns ----
@pytest.mark.parametrize("sw,sh,pad_cols,rows,pad", [
    (64, 8, 128, 16, 32),     # 64 columns exactly: one tile column, full
    (65, 8, 131, 17, 33),     # 65 columns, 17 rows: one over on both axes
    (30, 26, 61, 53, 0),      # no pad: the ring reflects at the plane's own border
    (110, 16, 220, 33, 95),   # 30 columns, the pad wider than a tile
])
def test_final_flow_tiles_and_crop(ctx, orc, sw, sh, pad_cols, rows, pad):
    f = flow_plane(sw, sh, 19 * sw + sh)
    up = orc.resize_linear_f32(f, pad_cols, rows) * F32(2.0) + F32(0)
    ref = orc.gaussian_blur(up, 3, 1.0)[:, pad:pad_cols - pad]
    assert_bits(ctx.stage_final(f, pad_cols, rows, pad, 2.0), ref, "final %dx%d" % (pad_cols - 2 * pad, rows))


# ---- level tables: gradients, gate + boxes + count ----
def table_sizes(orc, name):
    if name == "a":   # several levels inside one 1024-element chunk, pixel counts that are no multiple of 4 or 64
        return [(131, 97), (64, 9), (26, 24), (7, 5), (40, 4), (2, 2)]
    if name == "b":
        return orc.pyramid_sizes(281, 256)
    return [(1100, 20), (1024, 17), (990, 18), (300, 200)]   # w > 1024, w = 1024 (rStep = 0), a level across four gate blocks


SPECIAL = {"a": {1: "empty", 2: "first", 3: "last"}, "b": {3: "empty", 5: "first", 7: "last"}, "c": {}}


def alpha_pair(w, h, kind, r):
    """two alpha planes of one level.  Background below the threshold; gated pixels only where both planes lie above it."""
    a0 = (r.random((h, w)) * 0.85).astype(F32); a1 = (r.random((h, w)) * 0.85).astype(F32)
    hi = lambda shape: (0.9001 + 0.0999 * r.random(shape)).astype(F32)
    if kind == "first":
        a0[0, 0] = a1[0, 0] = F32(1.0)
    elif kind == "last":
        a0[-1, -1] = a1[-1, -1] = F32(0.95)
    elif kind is None:
        for _ in range(int(r.integers(1, 4))):
            x0, y0 = int(r.integers(0, w)), int(r.integers(0, h))
            x1, y1 = int(r.integers(x0, w)) + 1, int(r.integers(y0, h)) + 1
            a0[y0:y1, x0:x1] = hi((y1 - y0, x1 - x0)); a1[y0:y1, x0:x1] = hi((y1 - y0, x1 - x0))
            # the rectangle's last row and column sit exactly ON the threshold in one plane: not gated, so the box must not reach them
            if y1 - y0 > 1:
                a0[y1 - 1, x0:x1] = T
            if x1 - x0 > 1:
                a1[y0:y1, x1 - 1] = T
        x0, y0 = int(r.integers(0, w)), int(r.integers(0, h))
        a0[y0:y0 + 5, x0:x0 + 9] = hi(a0[y0:y0 + 5, x0:x0 + 9].shape)   # above the threshold in ONE plane only: not gated
        for _ in range(3):   # lone gated pixels
            y, x = int(r.integers(0, h)), int(r.integers(0, w))
            a0[y, x] = a1[y, x] = F32(1.0)
        if (w * h) % 4:      # a gated pixel in the level's last, partial group of four
            i = w * h - 1 - int(r.integers(0, (w * h) % 4))
            a0[i // w, i % w] = a1[i // w, i % w] = F32(0.91)
    return a0, a1


def gate_reference(a0, a1):
    g = (a0 > T) & (a1 > T)
    ys, xs = np.nonzero(g)
    box = None if ys.size == 0 else (int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max()))
    return g.astype(np.uint8), box, int(g.sum())


def table_case(orc, name, pair=0):
    key = ("tbl", name, pair)
    if key not in _cache:
        sizes = table_sizes(orc, name)
        r = np.random.default_rng({"a": 1, "b": 2, "c": 3}[name] * 1000 + pair)
        c = {"sizes": sizes, "img0": [], "img1": [], "a0": [], "a1": [], "g0": [], "g1": [], "gate": [], "box": []}
        for l, (w, h) in enumerate(sizes):
            i0 = r.random((h, w)).astype(F32); i1 = r.random((h, w)).astype(F32)
            i0[h // 3:h // 3 + 4, w // 4:w // 4 + 9] = F32(0.5)   # a flat patch: gradients of exactly 0 there
            a0, a1 = alpha_pair(w, h, SPECIAL[name].get(l) if pair == 0 else (None if l % 3 != pair % 3 else "empty"), r)
            g, box, cnt = gate_reference(a0, a1)
            c["img0"].append(i0); c["img1"].append(i1); c["a0"].append(a0); c["a1"].append(a1)
            c["g0"].append(np.stack(orc.gradients(i0), -1)); c["g1"].append(np.stack(orc.gradients(i1), -1))
            c["gate"].append(g); c["box"].append(box)
            if l == 0:
                c["count0"] = cnt
        _cache[key] = c
    return _cache[key]


def run_table(ctx, cases, **kw):
    return ctx.stage_level_table(cases[0]["sizes"], *[[c[k] for c in cases] for k in ("img0", "img1", "a0", "a1")], **kw)


def check_gradients(out, cases, lo=None, hi=None):
    """levels lo..hi-1 hold the oracle's gradients; every other element of the padded plane -- the other levels, the padding between
    levels -- still holds what the entry filled it with"""
    sizes, off = cases[0]["sizes"], out["off"]
    lo = 0 if lo is None else lo; hi = len(sizes) if hi is None else hi
    for p, c in enumerate(cases):
        for name in ("g0", "g1"):
            plane = out[name][p]
            written = np.zeros(plane.shape[0], bool)
            for l, (w, h) in enumerate(sizes):
                if lo <= l < hi:
                    o = int(off[l]); written[o:o + w * h] = True
                    assert_bits(plane[o:o + w * h].reshape(h, w, 2), c[name][l], "pair %d %s level %d (%dx%d)" % (p, name, l, w, h))
            rest = bits(plane)[~written]
            assert (rest == UNWRITTEN).all(), "pair %d %s: %d words outside the levels %d..%d were written" % (p, name, int((rest != UNWRITTEN).sum()), lo, hi - 1)


def check_gate(out, cases):
    sizes, off = cases[0]["sizes"], out["off"]
    for p, c in enumerate(cases):
        for l, (w, h) in enumerate(sizes):
            o = int(off[l])
            got = out["gate"][p][o:o + w * h].reshape(h, w)
            assert np.array_equal(got, c["gate"][l]), "pair %d level %d (%dx%d): %d gate bytes differ" % (p, l, w, h, int((got != c["gate"][l]).sum()))
            b = tuple(int(v) for v in out["boxes"][p, l])
            if c["box"][l] is None:
                assert b[2] < b[0] and b[3] < b[1], "pair %d level %d gates nothing, box %s" % (p, l, b)
            else:
                assert b == c["box"][l], "pair %d level %d (%dx%d): box %s, reference %s" % (p, l, w, h, b, c["box"][l])
        assert int(out["count0"][p]) == c["count0"], "pair %d: level-0 count" % p


@pytest.mark.parametrize("mode", ["full", "range", "one_block"])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_level_table_gradients(ctx, orc, name, mode):
    c = table_case(orc, name)
    n = len(c["sizes"])
    if mode == "range":   # levels 2 .. n-3: `first` > 0, a `total` that is not the plane's end
        off = np.concatenate([[0], np.cumsum([(w * h + 63) & ~63 for w, h in c["sizes"]])])
        out = run_table(ctx, [c], first=int(off[2]), total=int(off[n - 2]))
        check_gradients(out, [c], 2, n - 2)
    else:                 # one_block: the grid-stride loop walks the whole plane
        out = run_table(ctx, [c], max_blocks=1 if mode == "one_block" else 0)
        check_gradients(out, [c])


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_level_table_gate_boxes_and_count(ctx, orc, name):
    c = table_case(orc, name)
    kinds = SPECIAL[name]
    for l, kind in kinds.items():   # the cases this test is about are really there
        w, h = c["sizes"][l]
        assert c["box"][l] == {"empty": None, "first": (0, 0, 0, 0), "last": (w - 1, h - 1, w - 1, h - 1)}[kind]
    check_gate(run_table(ctx, [c]), [c])


def test_level_table_work_area_resets_itself(ctx, orc):
    """the gate kernel's last block puts its work area back: a second call on the same context, with another table in between, gives the
    same boxes and count"""
    a, c = table_case(orc, "a"), table_case(orc, "c")
    first = run_table(ctx, [a])
    check_gate(first, [a])
    check_gate(run_table(ctx, [c]), [c])
    again = run_table(ctx, [a])
    check_gate(again, [a])
    assert np.array_equal(first["boxes"], again["boxes"]) and np.array_equal(first["count0"], again["count0"])


def test_level_table_three_pairs(ctx, orc):
    """three pairs in slabs (blockIdx.z): each has its own alphas, so its own gate, boxes and count -- and its own gradients.  Twice: the
    slabs' work areas reset themselves too."""
    cases = [table_case(orc, "a", p) for p in range(3)]
    assert len({tuple(c["box"]) for c in cases}) == 3 and len({c["count0"] for c in cases}) == 3
    for _ in range(2):
        out = run_table(ctx, cases)
        check_gate(out, cases)
        check_gradients(out, cases)
