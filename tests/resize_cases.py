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


def all_pairs():
    """256 x 256: colour = column, alpha = row: every (colour, alpha) pair once"""
    img = np.empty((256, 256, 4), dtype=np.uint8)
    img[..., :3] = np.arange(256, dtype=np.uint8)[None, :, None]
    img[..., 3] = np.arange(256, dtype=np.uint8)[:, None]
    return img


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
