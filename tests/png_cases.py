"""The images of the device PNG encoder's tests (tests/test_gpu_png.py), built from fixed seeds, and what each is named for
(tests/test_png_decode_ref.py checks those properties from the images alone, without a GPU)."""
import numpy as np

# exact-fit shapes: rows of 4 * cols + 1 = 65 bytes; 252 of them fill one 16380-byte deflate segment, 504 two
FIT_COLS = 16
FIT_ROW_BYTES = 4 * FIT_COLS + 1


def fit_rows(segment_bytes, k):
    assert (k * segment_bytes) % FIT_ROW_BYTES == 0, "a segment is not a whole number of %d-byte rows" % FIT_ROW_BYTES
    return k * segment_bytes // FIT_ROW_BYTES


def _rng(seed):
    return np.random.default_rng(seed)


def noise(cols, rows, seed):
    return _rng(seed).integers(0, 256, (rows, cols, 4), dtype=np.uint8)


def smooth(cols, rows):
    """compressible at any size: a gentle gradient, another offset per channel"""
    g = np.add.outer(np.arange(rows) * 3, np.arange(cols) * 2)[:, :, None] + np.array([0, 5, 9, 200])
    return g.astype(np.uint8)


def constant(cols, rows, bgra):
    return np.tile(np.array(bgra, np.uint8), (rows, cols, 1))


def ramp_sub():
    """v(x, y) = 3 x + h(y), h(y) = 12 (y mod 2), all channels, no wrap (70 x 40, at most 219).  Sub leaves 3 per byte and h(y) in the
    first pixel.  Up leaves 12 everywhere, Average 8 or 4, None the values themselves.  Paeth predicts the left byte wherever there is
    one (the upper row's step of 3 is its smallest distance), i.e. ties with Sub there, and in the first pixel predicts the upper byte
    and leaves 12 >= h(y): never less than Sub in total, and the lower type number wins a tie.  Sub on every row."""
    x = np.arange(70)[None, :]; y = np.arange(40)[:, None]
    return np.repeat((3 * x + 12 * (y % 2))[:, :, None], 4, 2).astype(np.uint8)


def ramp_up():
    """ramp_sub's rule transposed: v(x, y) = 3 y + 12 (x mod 2) (80 x 70).  Up leaves 3 per byte; Sub 12, Average at least 3 in the
    first pixel and 8 or 4 elsewhere, Paeth predicts the upper byte (ties with Up).  Up on every row but the first (which has no upper
    row)."""
    x = np.arange(80)[None, :]; y = np.arange(70)[:, None]
    return np.repeat((3 * y + 12 * (x % 2))[:, :, None], 4, 2).astype(np.uint8)


def alpha_noise(cols, rows, seed):
    a = constant(cols, rows, (40, 90, 200, 0))
    a[:, :, 3] = _rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)
    return a


def small_cases(segment_bytes):
    """name -> image for the shapes around every edge of the encoder: no left neighbour, no upper row, row lengths around 256 bytes,
    streams of exactly k segments and one row more and less"""
    out = {}
    for cols, rows in [(1, 1), (1, 5), (7, 1), (2, 2), (63, 3), (64, 3), (65, 3)]:
        out["noise_%dx%d" % (cols, rows)] = noise(cols, rows, 100 + cols + rows)
        out["smooth_%dx%d" % (cols, rows)] = smooth(cols, rows)
    for k in (1, 2):
        full = fit_rows(segment_bytes, k)
        for rows in (full - 1, full, full + 1):
            out["fit%d_noise_%dx%d" % (k, FIT_COLS, rows)] = noise(FIT_COLS, rows, 200 + rows)
            out["fit%d_smooth_%dx%d" % (k, FIT_COLS, rows)] = smooth(FIT_COLS, rows)
    return out
