"""Inputs shared by tests/test_ref_core.py (the reference's own text against the oracle), tests/golden/make_refcore_golden.py (fixtures
produced by the reference's text) and tests/test_gpu_refcore.py (the HIP path against those fixtures).

Planes are built in a quantised form (uint8 images and alphas, int16 flows in 1/64 px) and decoded with one float operation each, so a
fixture can store the small integer arrays and every reader gets the same float bits."""
import numpy as np

# (pyrScaleFactor, smoothnessCoef, verticalRegularizationCoef, horizontalRegularizationCoef, gradientStepSize): tests/test_gpu_solver_params.py's
SET_POW2 = (0.8, 0.002, 0.02, 0.005, 0.25)
SET_ODD = (0.85, 0.0005, 0.0, 0.03, 0.7)


def img_f32(q):
    return q.astype(np.float32) / np.float32(255.0)


def flow_f32(q):
    return q.astype(np.float32) / np.float32(64.0)


def level_case_q(w, h, seed, gate="rects", levels=256):
    """Quantised planes of one pyramid level: I0, I1 (I1 = I0 shifted, plus noise), alpha0, alpha1, incoming flow.
    gate: 'rects' (alpha 255 / 242 / 153 rectangles over 0: gated, gated, not gated), 'empty' (no pixel passes 0.9), 'one' (one pixel does)."""
    r = np.random.default_rng(seed)
    base = r.integers(0, levels, (h, w))
    i0 = (base * (255 // (levels - 1))).astype(np.uint8)
    i1 = np.roll(base, int(r.integers(-3, 4)), axis=1)
    noise = r.integers(0, 8, (h, w)) if levels == 256 else (r.random((h, w)) < 0.1)
    i1 = (np.clip(i1 + noise, 0, levels - 1) * (255 // (levels - 1))).astype(np.uint8)
    a0 = np.zeros((h, w), np.uint8); a1 = np.zeros((h, w), np.uint8)
    if gate == "rects":
        for a in (a0, a1):
            a[h // 8:h - h // 9, w // 10:w - w // 7] = 255
            for _ in range(3):
                x0, y0 = int(r.integers(0, w)), int(r.integers(0, h))
                a[y0:int(r.integers(y0, h)) + 1, x0:int(r.integers(x0, w)) + 1] = int(r.choice([255, 242, 153, 0]))
    elif gate == "empty":
        a0[:] = 229; a1[:] = 255        # 229/255 = 0.898 < 0.9
    elif gate == "one":
        a0[:] = 153; a1[:] = 255; a0[h // 2, w // 3] = 255
    fin = np.clip(np.rint(r.standard_normal((h, w, 2)) * 1.2 * 64), -32000, 32000).astype(np.int16)
    return dict(I0=i0, I1=i1, a0=a0, a1=a1, fin=fin)


def decode_level(q):
    return img_f32(q["I0"]), img_f32(q["I1"]), img_f32(q["a0"]), img_f32(q["a1"]), flow_f32(q["fin"])


# smoothnessCoef 0: the error of a candidate is its data term plus the two regularisers, which see only |flow.x| and |flow.y|
SET_TIES = (0.9, 0.0, 0.01, 0.01, 0.5)


def tie_case_q(w, h, seed):
    """A level on which two DIFFERENT proposals often have EXACTLY the same error, so that the order of the two proposals of a sweep and the
    strictness of proposeFlowUpdate's comparison decide the result (on ordinary data exact ties between different flows do not occur).
    Images vary with y only (the data term cannot tell +x from -x), the incoming flow is (+-a, b) with a from three values and b from two, run
    with SET_TIES; only pixels at odd x and odd y are gated, so every proposal a gated pixel sees is an untouched incoming flow."""
    r = np.random.default_rng(seed)
    i0 = np.repeat(r.integers(0, 256, (h, 1)), w, axis=1).astype(np.uint8)
    i1 = np.repeat(r.integers(0, 256, (h, 1)), w, axis=1).astype(np.uint8)
    a0 = np.full((h, w), 153, np.uint8); a0[1::2, 1::2] = 255
    a1 = np.full((h, w), 255, np.uint8)
    fx = r.choice([32, 64, 96], (h, w)) * r.choice([-1, 1], (h, w))
    fy = r.choice([0, 32], (h, w))
    return dict(I0=i0, I1=i1, a0=a0, a1=a1, fin=np.stack([fx, fy], -1).astype(np.int16))


def adjust_case_q(w, h, seed):
    """Five grey levels (ties everywhere), alpha planes with zero blocks wide enough that a whole clamped 5x5 patch has sum(alpha) = 0:
    the inf / NaN loser path of computePatchError."""
    q = level_case_q(w, h, seed, gate="rects", levels=5)
    a0 = np.full((h, w), 255, np.uint8); a1 = np.full((h, w), 255, np.uint8)
    a0[:h // 4, :w // 3] = 0; a0[h // 2:h // 2 + 3, :] = 204          # 0.8: not updated
    a1[h // 3:h // 3 + 12, w // 4:w // 4 + 14] = 0                    # 12 x 14 hole: patches inside it have sum(alpha) = 0
    a1[:, w - 3:] = 0
    q["a0"], q["a1"] = a0, a1
    del q["fin"]
    return q


def rect_canvas(synth, cols, rows, seed, rects_l, rects_r, notch=None):
    """A stitch canvas pair: synthetic texture, alpha 255 inside the union of each side's rectangles (x0, y0, x1, y1; x1 > cols wraps round the
    seam), every channel 0 outside.  notch = (x0, y0, x1, y1) is cut out of L."""
    L, R, _ = synth.make_pair_np(cols, rows, seed)
    x = np.arange(cols)[None, :]; y = np.arange(rows)[:, None]
    out = []
    for img, rects, cut in ((L, rects_l, notch), (R, rects_r, None)):
        m = np.zeros((rows, cols), bool)
        for (x0, y0, x1, y1) in rects:
            m |= ((x - x0) % cols < (x1 - x0)) & (y >= y0) & (y < y1)
        if cut is not None:
            m &= ~((x >= cut[0]) & (x < cut[2]) & (y >= cut[1]) & (y < cut[3]))
        im = img.copy()
        im[..., :3] = np.maximum(im[..., :3], 1)
        im[..., 3] = 255
        im[~m] = 0
        out.append(im)
    return out[0], out[1]


# name -> (cols, rows, seed, L rectangles, R rectangles, notch in L, hole in the crafted merged image)
#   tall_even : cols <= rows, step 2, tile kernel rows/130 = 6 (even), final kernel rows/400 = 2; L has a notch
#   tall_odd  : cols <= rows, tile kernel 7 (odd), final kernel 2
#   wide_seam : cols > rows, tile kernel 3, final kernel 1; both images wrap round the 360 degree seam, and so does their overlap
#   small     : step 1 (1 x 1 tiles), tile kernel 3, final kernel 1: the cheapest canvas that is in no regime the oracle had to define
CANVASES = {
    "tall_even": (400, 800, 31, [(60, 150, 230, 600)], [(170, 250, 350, 700)], (170, 380, 200, 430), (190, 300, 215, 330)),
    "tall_odd": (420, 1000, 32, [(110, 200, 300, 640)], [(130, 560, 330, 900)], None, (180, 580, 230, 610)),
    "wide_seam": (800, 400, 33, [(650, 120, 950, 300)], [(670, 60, 930, 200)], None, (105, 140, 125, 170)),
    "small": (240, 400, 34, [(30, 100, 140, 300)], [(100, 150, 220, 350)], None, (105, 160, 130, 190)),
}


def canvas(synth, name):
    cols, rows, seed, rl, rr, notch, hole = CANVASES[name]
    L, R = rect_canvas(synth, cols, rows, seed, rl, rr, notch)
    return L, R, hole


def crafted_merged(mp, ovl, hole):
    """A merged image for Gather: the overlap's L pixels, with a hole (alpha 0) so that 150-valued pixels remain in Gather's map."""
    m = np.where((mp == 150)[..., None], ovl, 0).astype(np.uint8)
    m[hole[1]:hole[3], hole[0]:hole[2]] = 0
    return m


def gather_map(mp, merged):
    return (mp.astype(np.int32) + np.where(merged[..., 3] > 0, 75, 0)).clip(0, 255).astype(np.uint8)


def n150_near_border(gmap, margin=100):
    """150-valued pixels of Gather's map nearer than `margin` px to a canvas border: Gather's 8-direction probes (up to 99 px) would leave the image."""
    rows, cols = gmap.shape
    inner = np.zeros_like(gmap, bool)
    inner[margin:rows - margin, margin:cols - margin] = True
    return int(((gmap == 150) & ~inner).sum())


def combine_case(synth, cols=203, rows=131, seed=9):
    """Crafted inputs of combineNovelViews: alpha 0 in either source, blend exactly 0 and 1, equal colours (deghost 0), flows that wrap the seam
    once; |flow * t| stays below cols (beyond that the reference reads out of bounds)."""
    L, R, blend = synth.make_pair_np(cols, rows, seed)
    L = L.copy(); R = R.copy(); blend = blend.copy()
    L[..., 3] = 255; R[..., 3] = 255
    L[20:40, 30:70] = 0                      # alpha 0 in L only
    R[60:85, 100:150] = 0                    # alpha 0 in R only
    L[90:110, 10:60, 3] = 128; R[95:120, 40:90, 3] = 1     # partial alphas
    R[5:18, 120:190] = L[5:18, 120:190]      # equal colours
    blend[:, :25] = 0.0; blend[:, cols - 25:] = 1.0; blend[40:50, :] = 0.5
    r = np.random.default_rng(seed)
    f0 = flow_f32(np.rint(r.standard_normal((rows, cols, 2)) * 3 * 64).astype(np.int16))
    f1 = flow_f32(np.rint(r.standard_normal((rows, cols, 2)) * 3 * 64).astype(np.int16))
    f0[5:18, 120:190] = 0; f1[5:18, 120:190] = 0           # ... sampled where they lie
    f0[:, cols - 12:, 0] += 40.0; f1[:, cols - 12:, 0] += 55.0   # leaves on the right: wraps once
    f0[:, :12, 0] -= 40.0; f1[:, :12, 0] -= 55.0                 # leaves on the left
    f0[:6, :, 1] -= 20.0; f1[rows - 6:, :, 1] += 20.0            # leaves above / below: clamped
    f0[70:80, 60:90] = 150.0; f1[70:80, 60:90] = -150.0          # long, still below cols
    assert max(np.abs(f0[..., 0]).max(), np.abs(f1[..., 0]).max()) < cols
    return L, R, f0, f1, blend
