"""Reference and inputs of the tile-smoothing tests: the raster-order loop of CPU/StitchTool.cpp:134-141 over the oracle's
blur-on-a-ROI, for an explicit tile size `step` and window `k` (the oracle's own orc_blend_smooth derives both from the canvas)."""
import ctypes as C

import numpy as np


def active_tiles(md, step):
    """(ys, xs) of the tiles the reference smooths, in its raster order: y = 0, step, ... while y + step < rows, likewise x"""
    rows, cols = md.shape
    ty, tx = np.nonzero(md[0:rows - step:step, 0:cols - step:step] > np.float32(step))
    return ty * step, tx * step


def tile_pass_reference(orc, blend, md, step, k):
    """the tile pass alone, in place on a copy; returns (result, number of active tiles)"""
    b = np.ascontiguousarray(blend, dtype=np.float32).copy()
    rows, cols = b.shape
    l = orc.lib()
    p = b.ctypes.data_as(C.c_void_p)
    ys, xs = active_tiles(np.asarray(md, np.float32), step)
    for y, x in zip(ys.tolist(), xs.tolist()):
        l.orc_box_blur_roi(p, cols, rows, x, y, step, step, k)
    return b, len(ys)


def random_inputs(cols, rows, step, seed):
    """A ramp whose magnitudes span 40 binades (fp64 sums of it are inexact, so the order of summation shows in the bits) and a
    MergedDis that makes about two thirds of the tiles active (adjacent active tiles: the wavefront and the in-place reads)."""
    rng = np.random.default_rng(seed)
    blend = (rng.random((rows, cols)) * np.exp2(-rng.integers(0, 41, (rows, cols)).astype(np.float64))).astype(np.float32)
    md = (rng.random((rows, cols)) * 3 * step).astype(np.float32)
    return blend, md
