"""Serial numpy model of the device resize (csrc/kernels_resize.hip, csrc/resize_table.hpp): Pillow's Image.resize of an RGBA image,
restated.  Premultiply by alpha, one antialiased pass per axis whose size changes (horizontal first) in 22-bit fixed point with a 32-bit
accumulator, un-premultiply.  The tables are computed in double in Pillow's order of operations; HAMMING and LANCZOS go through this
host's sin / cos.  tests/test_resize_model.py holds it to Pillow byte for byte; the device and the host-run kernels are held to it."""
import math

import numpy as np

LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = 1, 2, 3, 4, 5
FILTERS = {"lanczos": LANCZOS, "bilinear": BILINEAR, "bicubic": BICUBIC, "box": BOX, "hamming": HAMMING}
SUPPORT = {LANCZOS: 3.0, BILINEAR: 1.0, BICUBIC: 2.0, BOX: 0.5, HAMMING: 1.0}
PREC = 22
# Pillow writes HAMMING's two constants as single-precision literals (0.54f, 0.46f) inside its double expression
HAMMING_A, HAMMING_B = float(np.float32(0.54)), float(np.float32(0.46))


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def weight(f, x):
    if f == BOX:
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if f == LANCZOS:
        return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0
    if x < 0.0:
        x = -x
    if f == BILINEAR:
        return 1.0 - x if x < 1.0 else 0.0
    if f == HAMMING:
        if x == 0.0:
            return 1.0
        if x >= 1.0:
            return 0.0
        x = x * math.pi
        return math.sin(x) / x * (HAMMING_A + HAMMING_B * math.cos(x))
    if f == BICUBIC:
        a = -0.5
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    raise ValueError("unknown filter %r" % (f,))


def table(n_in, n_out, f):
    """per output index: (first source index, int64 array of the taps' 22-bit coefficients)"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = SUPPORT[f] * fs
    ss = 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = [weight(f, (x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(v * 4194304 + (-0.5 if v < 0 else 0.5)) for v in w]
        out.append((xmin, np.array(k, dtype=np.int64)))
    return out


def premultiply(img):
    out = img.copy()
    a = img[..., 3:4].astype(np.int64)
    t = img[..., :3].astype(np.int64) * a + 128
    out[..., :3] = (((t >> 8) + t) >> 8).astype(np.uint8)
    return out


def unpremultiply(img):
    out = img.copy()
    a = img[..., 3:4].astype(np.int64)
    c = img[..., :3].astype(np.int64)
    q = np.minimum(255, (255 * c) // np.maximum(a, 1))
    out[..., :3] = np.where((a == 0) | (a == 255), c, q).astype(np.uint8)
    return out


def resample_rows_raw(img, n_out, f):
    """the pass along axis 0 of an (n, m, 4) uint8 array before its clamp: int64, the 32-bit accumulator shifted down by PREC"""
    n_in = img.shape[0]
    out = np.empty((n_out,) + img.shape[1:], dtype=np.int64)
    p = img.astype(np.int64)
    for yy, (ymin, k) in enumerate(table(n_in, n_out, f)):
        acc = (1 << (PREC - 1)) + np.tensordot(k, p[ymin:ymin + len(k)], axes=(0, 0))
        acc = ((acc + (1 << 31)) % (1 << 32)) - (1 << 31)   # the accumulator has 32 bits
        out[yy] = acc >> PREC
    return out


def resample_rows(img, n_out, f):
    """the pass along axis 0 of an (n, m, 4) uint8 array: every channel alike"""
    return np.clip(resample_rows_raw(img, n_out, f), 0, 255).astype(np.uint8)


def passes_raw(img, out_cols, out_rows, f):
    """[(pass, raw)] for the passes resize() runs, "h" and / or "v": the pass's outputs before the clamp, (rows, cols, 4) int64"""
    img = np.ascontiguousarray(img)
    rows, cols = img.shape[:2]
    cur, out = premultiply(img), []
    if out_cols != cols:
        raw = resample_rows_raw(cur.transpose(1, 0, 2), out_cols, f).transpose(1, 0, 2)
        out.append(("h", raw))
        cur = np.clip(raw, 0, 255).astype(np.uint8)
    if out_rows != rows:
        out.append(("v", resample_rows_raw(np.ascontiguousarray(cur), out_rows, f)))
    return out


def clamp_counts(img, out_cols, out_rows, f):
    """{pass: (low, high)}: per channel (B, G, R, A) how many outputs of the pass the clamp raises from below 0 and lowers from above 255"""
    return {name: ([int((raw[..., c] < 0).sum()) for c in range(4)], [int((raw[..., c] > 255).sum()) for c in range(4)])
            for name, raw in passes_raw(img, out_cols, out_rows, f)}


def resize(img, out_cols, out_rows, f):
    """(rows, cols, 4) uint8 with alpha last -> (out_rows, out_cols, 4)"""
    img = np.ascontiguousarray(img)
    rows, cols = img.shape[:2]
    if f not in SUPPORT:
        raise ValueError("unknown filter %r" % (f,))
    if out_cols == cols and out_rows == rows:
        return img.copy()
    cur = premultiply(img)
    if out_cols != cols:
        cur = resample_rows(cur.transpose(1, 0, 2), out_cols, f).transpose(1, 0, 2)
    if out_rows != rows:
        cur = resample_rows(np.ascontiguousarray(cur), out_rows, f)
    return unpremultiply(np.ascontiguousarray(cur))
