"""Shapes and images shared by the resize tests (model vs Pillow, host-run kernels vs model, device vs model)."""
import numpy as np

import resize_model

FILTER_IDS = [resize_model.LANCZOS, resize_model.BILINEAR, resize_model.BICUBIC, resize_model.BOX, resize_model.HAMMING]

# (cols, rows, out_cols, out_rows): down- and upscaling, one axis unchanged, nearly the same size, many taps, one source pixel
MODEL_SHAPES = [(97, 41, 31, 17), (64, 48, 64, 20), (50, 33, 77, 33), (130, 7, 9, 5), (33, 29, 32, 28), (200, 100, 3, 2), (1, 1, 5, 4), (300, 2, 1, 1)]

MEDIUM_SHAPE = (1000, 600, 455, 273)

# a tile of the horizontal pass (64 output columns) whose source window needs three LDS pieces of 256 columns, next to a partial tile
PIECE_SHAPE = (700, 5, 70, 5)


def image(cols, rows, seed=0):
    """(rows, cols, 4) uint8: random colour; alpha random, with a fully transparent quadrant (its colour stays: it must not bleed) and an opaque block"""
    rng = np.random.default_rng(1000003 * cols + 1009 * rows + seed)
    img = rng.integers(0, 256, size=(rows, cols, 4), dtype=np.uint8)
    img[:(rows + 1) // 2, :(cols + 1) // 2, 3] = 0
    img[rows // 2:rows // 2 + max(1, rows // 3), cols // 2:cols // 2 + max(1, cols // 3), 3] = 255
    return img


def ringing(cols, rows, bx, by, rest_alpha=255):
    """(rows, cols, 4) uint8 that makes the negative lobes of LANCZOS and BICUBIC overshoot in every channel: four vertical bands; in band q
    channel q (B, G, R, A) is a checkerboard of bx x by blocks of 0 and 255, the other colour channels rest at 128 and alpha, outside its
    own band, at rest_alpha.  255: opaque; 128: translucent, whose overshoot is colour above alpha for the un-premultiply"""
    img = np.empty((rows, cols, 4), dtype=np.uint8)
    img[..., :3] = 128
    img[..., 3] = rest_alpha
    board = (((np.arange(cols)[None, :] // bx) + (np.arange(rows)[:, None] // by)) & 1).astype(np.uint8) * 255
    for q in range(4):
        x0, x1 = q * cols // 4, (q + 1) * cols // 4
        img[:, x0:x1, q] = board[:, x0:x1]
    return img


# (cols, rows, out_cols, out_rows, bx, by) of the ringing image: with LANCZOS and BICUBIC the model clamps at least 10 outputs from below 0
# and 10 from above 255 in each of the four channels in each pass that runs (tests assert it through ringing_case); up- and downscaling,
# and one axis alone, where a single pass carries both fusions
RINGING_SHAPES = [(50, 33, 77, 47, 2, 2), (97, 41, 31, 17, 6, 5), (180, 24, 65, 9, 6, 5), (50, 33, 50, 47, 2, 2), (97, 41, 31, 41, 6, 5)]
RINGING_FILTERS = [resize_model.LANCZOS, resize_model.BICUBIC]
RINGING_MIN_CLAMPED = 10


def ringing_case(shape, f, rest_alpha=255):
    """(image, the model's result, the class of every output byte in the last pass: -1 clamped from below 0, 1 from above 255, 0 neither);
    asserts the condition on the inputs first: the opaque image of the shape clamps often enough in every channel and pass"""
    cols, rows, out_cols, out_rows, bx, by = shape
    key = ("ringing", shape, f)
    if key not in _MODEL_CACHE:
        _MODEL_CACHE[key] = resize_model.clamp_counts(ringing(cols, rows, bx, by), out_cols, out_rows, f)
    counts = _MODEL_CACHE[key]
    assert counts and all(min(low + high) >= RINGING_MIN_CLAMPED for low, high in counts.values()), (shape, f, counts)
    img = ringing(cols, rows, bx, by, rest_alpha)
    want = model(("ringing", shape, rest_alpha), img, out_cols, out_rows, f)
    raw = resize_model.passes_raw(img, out_cols, out_rows, f)[-1][1]
    return img, want, np.where(raw < 0, -1, np.where(raw > 255, 1, 0))


def differing_by_class(got, want, cls):
    """the differing bytes per channel and per clamped class of the model's last pass, for an assertion's message"""
    parts = []
    for c, name in enumerate("BGRA"):
        d = got[..., c] != want[..., c]
        parts.append("%s: %d low, %d high, %d unclamped" % (name, int((d & (cls[..., c] < 0)).sum()), int((d & (cls[..., c] > 0)).sum()), int((d & (cls[..., c] == 0)).sum())))
    return "%d of %d bytes differ (%s)" % (int((got != want).sum()), want.size, "; ".join(parts))


def all_pairs():
    """256 x 256: colour = column, alpha = row: every (colour, alpha) pair once"""
    img = np.empty((256, 256, 4), dtype=np.uint8)
    img[..., :3] = np.arange(256, dtype=np.uint8)[None, :, None]
    img[..., 3] = np.arange(256, dtype=np.uint8)[:, None]
    return img


def all_pairs_distinct():
    """256 x 256: alpha = row; B, G and R three different bijections of the column, so that every (colour, alpha) pair stands once in each
    of the three byte positions and a byte that landed in another position would show"""
    c = np.arange(256)
    img = np.empty((256, 256, 4), dtype=np.uint8)
    for q, col in enumerate((c, 255 - c, (7 * c + 3) & 255)):
        img[..., q] = col.astype(np.uint8)[None, :]
    img[..., 3] = c.astype(np.uint8)[:, None]
    return img


def model_pass(img, axis, n_out, f, premul, unpremul):
    """one pass of the model alone: axis 0 along the columns (the horizontal kernel), axis 1 along the rows, with the two fusions as given"""
    cur = resize_model.premultiply(img) if premul else np.ascontiguousarray(img)
    if axis == 0:
        cur = resize_model.resample_rows(cur.transpose(1, 0, 2), n_out, f).transpose(1, 0, 2)
    else:
        cur = resize_model.resample_rows(cur, n_out, f)
    cur = np.ascontiguousarray(cur)
    return resize_model.unpremultiply(cur) if unpremul else cur


def pass_cases():
    """(name, image, axis, n_out, filter, premul, unpremul, the model's image, class of every output byte as in ringing_case) of one pass alone,
    for each of the two kernels.  A BOX pass that doubles the axis has one tap of exactly 2^22, so the accumulator returns the byte: with one
    fusion on, the all-pairs image puts all 65536 (colour, alpha) pairs through it in all three byte positions, colour above alpha included.
    With neither, a LANCZOS pass over the opaque ringing image leaves the clamp's raw bytes with nothing after it to hide a wrong one; the
    condition on the inputs (10 outputs clamped low and 10 high per channel) is asserted here, on the model."""
    key = "pass_cases"
    if key in _MODEL_CACHE:
        return _MODEL_CACHE[key]
    out = []
    pairs = all_pairs_distinct()
    for axis in (0, 1):
        doubled = np.repeat(pairs, 2, axis=1 - axis)
        assert np.array_equal(model_pass(pairs, axis, 512, resize_model.BOX, 0, 0), doubled)
        none = np.zeros(doubled.shape, np.int64)
        out.append(("unpremultiply_axis%d" % axis, pairs, axis, 512, resize_model.BOX, 0, 1, resize_model.unpremultiply(doubled), none))
        out.append(("premultiply_axis%d" % axis, pairs, axis, 512, resize_model.BOX, 1, 0, resize_model.premultiply(doubled), none))
    for cols, rows, axis, n_out, bx, by in [(97, 41, 0, 31, 6, 5), (50, 33, 0, 77, 2, 2), (50, 33, 1, 47, 2, 2), (97, 41, 1, 17, 6, 5)]:
        img = ringing(cols, rows, bx, by)
        src = img.transpose(1, 0, 2) if axis == 0 else img
        raw = resize_model.resample_rows_raw(src, n_out, resize_model.LANCZOS)
        raw = raw.transpose(1, 0, 2) if axis == 0 else raw
        low, high = [int((raw[..., c] < 0).sum()) for c in range(4)], [int((raw[..., c] > 255).sum()) for c in range(4)]
        assert min(low + high) >= RINGING_MIN_CLAMPED, (cols, rows, axis, n_out, low, high)
        want = model_pass(img, axis, n_out, resize_model.LANCZOS, 0, 0)
        out.append(("raw_%dx%d_axis%d_to_%d" % (cols, rows, axis, n_out), img, axis, n_out, resize_model.LANCZOS, 0, 0, want, np.where(raw < 0, -1, np.where(raw > 255, 1, 0))))
    for case in out:
        case[7].setflags(write=False)
    _MODEL_CACHE[key] = out
    return out


def edge_shapes():
    """output widths and heights on both sides of the passes' tile (64 x 4 outputs) and workgroup (256 threads) edges, each from a source about
    2.2 times and about 0.7 times as large; the other axis is small and changes too, so both passes run"""
    out = []
    for edge in (63, 64, 65, 255, 256, 257):
        for ratio in (2.2, 0.7):
            src = int(round(edge * ratio))
            out.append((src, 11, edge, 6))     # the edge in width
            out.append((13, src, 10, edge))    # ... and in height
    return out


_MODEL_CACHE = {}


def model(key, img, out_cols, out_rows, f):
    """resize_model.resize, computed once per key and shared between tests (the result is read-only)"""
    k = (key, out_cols, out_rows, f)
    if k not in _MODEL_CACHE:
        r = resize_model.resize(img, out_cols, out_rows, f)
        r.setflags(write=False)
        _MODEL_CACHE[k] = r
    return _MODEL_CACHE[k]
