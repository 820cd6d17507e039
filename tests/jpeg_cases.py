"""The images of the device JPEG encoder's tests, built from fixed seeds.  branch_cases(): each is a small image made to reach one thing
in the coder, at the quality and subsampling it names and the product's restart interval; reached(trace) says, from the serial model's
symbol trace (tests/jpeg_model.py), that it does.  tests/test_jpeg_model.py asserts that for every case, without a GPU."""
import collections
import io

import numpy as np

import jpeg_model as M

Case = collections.namedtuple("Case", "img quality subsampling reached")

BRANCHES = ["zrl", "zrl_twice", "no_eob", "all_zero_block", "dc_category_11", "ac_category_10", "negative_tie", "ff_inside", "ff_last_byte",
            "ends_on_a_byte", "less_than_an_interval", "exactly_k_intervals", "marker_index_wraps", "interval_crosses_a_row", "dummy_right",
            "dummy_bottom", "dummy_both", "odd_chroma_pad", "hostile_noise_q100", "ff_ends_a_window", "interval_fills_its_windows",
            "code_straddles_a_seam"]

# every kind of restart interval the coder admits (jpeg_restart_fits: at most 384 blocks, two rounds of its 192 threads), by subsampling:
# one and two MCUs, a block short of a round and a block past it, a block short of two rounds, two rounds.  The product's are one round.
INTERVALS = {1: (1, 2, 31, 33, 63, 64), 0: (1, 2, 63, 65, 127, 128)}
REFUSED_INTERVAL = {1: 65, 0: 129}

WINDOW = 4096   # kWinBytes of csrc/kernels_jpeg.hip: the coder merges an interval's bits into LDS windows of this many unstuffed bytes


def pillow_file(img, quality, subsampling, restart):
    """libjpeg-turbo's own file for the image (packed BGRA), through Pillow: what tests/test_jpeg_model.py holds the model to, and the
    expected bytes of the shapes that are too large for the model's Python loops"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., [2, 1, 0]]), "RGB").save(buf, format="JPEG", quality=quality, subsampling=2 if subsampling else 0,
                                                                          restart_marker_blocks=restart)
    return buf.getvalue()


def noise(cols, rows, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 4), dtype=np.uint8)


def smooth(cols, rows):
    g = np.add.outer(np.arange(rows) * 3, np.arange(cols) * 2)[:, :, None] + np.array([0, 40, 90, 200])
    return g.astype(np.uint8)


def patched(cols, rows, seed, box):
    """smooth, with a patch of noise: box = (row0, row1, col0, col1)"""
    img = smooth(cols, rows)
    r0, r1, c0, c1 = box
    img[r0:r1, c0:c1] = noise(c1 - c0, r1 - r0, seed)
    return img


# the largest side SOF0 holds, and the largest libjpeg agrees to write (its JPEG_MAX_DIMENSION): Pillow refuses anything longer
MAX_SIDE, LIBJPEG_MAX_SIDE = 65535, 65500


def long_image(across):
    """65535 x 9 (across) or 9 x 65535: smooth, a stripe of noise at 40000 and another over the last 300 pixels of the long side"""
    if across:
        img = patched(MAX_SIDE, 9, 43, (0, 9, 40000, 40600)); img[:, -300:] = noise(300, 9, 44)
    else:
        img = patched(9, MAX_SIDE, 43, (40000, 40600, 0, 9)); img[-300:] = noise(9, 300, 44)
    return img


def grey(plane):
    """B = G = R: Y is the value itself (the three weights sum to 65536) and both chroma planes are 128 throughout"""
    p = np.asarray(plane, np.uint8)
    return np.stack([p, p, p, np.full_like(p, 255)], axis=2)


def _idct_matrix():
    u = np.arange(8)[:, None]; x = np.arange(8)[None, :]
    d = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    d[0] /= np.sqrt(2)
    return d


def from_coefficients(blocks, quality):
    """grey image of 8x8 blocks whose luma coefficients quantise, at `quality`, to the given ones: blocks = (block rows, block cols) nested
    lists of {zigzag index: quantised value}.  Each sample block is the inverse DCT of value * table entry, rounded: the error that
    leaves in a coefficient stays well under half a quantisation step at quality 50."""
    q = M.quant_table(M.QBASE_LUMA, quality)
    d = _idct_matrix()
    br, bc = len(blocks), len(blocks[0])
    out = np.zeros((8 * br, 8 * bc))
    for r in range(br):
        for c in range(bc):
            f = np.zeros(64)
            for zz, v in blocks[r][c].items():
                f[M.ZIGZAG[zz]] = v * q[M.ZIGZAG[zz]]
            out[8 * r:8 * r + 8, 8 * c:8 * c + 8] = d.T @ f.reshape(8, 8) @ d + 128
    assert out.min() >= 0 and out.max() <= 255
    return grey(np.rint(out))


def _padded_bytes(nbits):
    return (nbits + 7) // 8


def ff_ends_a_window(t):
    """some interval has a 0xFF as the last unstuffed byte of a window, and bytes behind it: the stuffed 0x00 is the last byte the
    window writes"""
    return any(((off % WINDOW == WINDOW - 1) & (off < _padded_bytes(n) - 1)).any() for off, n in zip(t["ff_offsets"], t["interval_bits"]))


def interval_fills_its_windows(t):
    """some interval's padded length is two or more whole windows, and its last bits are padding"""
    return any(n % 8 != 0 and _padded_bytes(n) % WINDOW == 0 and _padded_bytes(n) >= 2 * WINDOW for n in t["interval_bits"])


def _bits(raw, lo, hi):
    """bits [lo, hi) of the bytes, as a number"""
    return (int.from_bytes(raw, "big") >> (8 * len(raw) - hi)) & ((1 << (hi - lo)) - 1)


def code_straddles_a_seam(t):
    """a code word of 17 bits or more starts in the last 16 bits of a window, with a 1-bit on either side of the seam: its first part
    goes into the window's last 32-bit word, and the rest opens the next window from before its first word"""
    for raw, starts, lens in zip(t["interval_raw"], t["word_starts"], t["word_lens"]):
        to_seam = (-starts) % (8 * WINDOW)
        for k in np.flatnonzero((lens >= 17) & (to_seam >= 1) & (to_seam <= 16) & (starts + to_seam >= 8 * WINDOW)):
            s, seam, e = int(starts[k]), int(starts[k] + to_seam[k]), int(starts[k] + lens[k])
            if _bits(raw, s, seam) and _bits(raw, seam, e):
                return True
    return False


def filled_interval_image():
    """37 x 3 MCUs of noise at 4:4:4: the last interval is MCUs 64..110.  Its last MCU is noise of a reduced amplitude, chosen so that
    the interval comes to 3 * 32768 - 1 bits"""
    image_seed, mcu_seed, amplitude = FILL_SEEDS
    img = noise(296, 24, image_seed)
    px = noise(8, 8, mcu_seed).astype(np.int64)
    px[..., :3] = 128 + ((px[..., :3] - 128) * amplitude) // 256
    img[16:24, 288:296] = px.astype(np.uint8)
    return img


def branch_cases():
    c = {}
    # one coefficient behind 19 zeros: one ZRL, then (3, size)
    c["zrl"] = Case(from_coefficients([[{0: 2, 20: 3}, {0: 2}]], 50), 50, 0, lambda t: t["zrl"] == 1 and t["zrl_pairs"] == 0)
    # ... behind 39 zeros: two ZRLs in a row, then (7, size)
    c["zrl_twice"] = Case(from_coefficients([[{0: -3, 40: -2}, {0: 1}]], 50), 50, 0, lambda t: t["zrl"] == 2 and t["zrl_pairs"] == 1)
    # coefficient 63 is not zero: the block ends without an EOB
    c["no_eob"] = Case(from_coefficients([[{0: 1, 63: 1}, {0: 1, 5: -1}]], 50), 50, 0, lambda t: t["no_eob"] == 1 and t["zrl"] == 3)
    # a flat image: after the first MCU every block is a zero DC difference and an EOB
    c["all_zero_block"] = Case(grey(np.full((16, 32), 77)), 50, 1, lambda t: t["all_zero"] >= 8)
    # blocks of black and white at quality 100: the DC goes from -1024 to 1016 and back
    c["dc_category_11"] = Case(grey(np.kron((np.add.outer(np.arange(2), np.arange(4)) % 2) * 255, np.ones((8, 8)))), 100, 0, lambda t: t["max_dc_cat"] == 11)
    # a black and a white half in one block at quality 100: the first horizontal coefficient is beyond 512
    c["ac_category_10"] = Case(grey(np.tile(np.repeat([0, 255], 4), (8, 2))), 100, 0, lambda t: t["max_ac_cat"] == 10)
    # every sample 127 at quality 50: the DC is -64 and its step 128, so -0.5 rounds away from zero to -1
    c["negative_tie"] = Case(grey(np.full((8, 16), 127)), 50, 0, lambda t: t["negative_ties"] == 2)
    c["ff_inside"] = Case(noise(16, 16, 3), 100, 0, lambda t: t["ff_inside"] > 0)
    # (the seeds of the next two were searched for)
    c["ff_last_byte"] = Case(noise(128, 64, FF_LAST_SEED), 100, 0, lambda t: t["ff_last"] > 0 and t["intervals"] > 1)
    c["ends_on_a_byte"] = Case(noise(96, 32, EXACT_SEED), 90, 1, lambda t: t["exact_byte"] > 0)
    c["less_than_an_interval"] = Case(noise(8, 8, 5), 90, 1, lambda t: t["intervals"] == 1 and t["mcu_rows"] * t["mcu_cols"] == 1)
    # 8 x 8 MCUs of 16 x 16: two intervals of 32, each four whole MCU rows
    c["exactly_k_intervals"] = Case(smooth(128, 128), 90, 1, lambda t: t["intervals"] == 2 and t["mcu_rows"] * t["mcu_cols"] == 64)
    # 17 x 17 MCUs: ten intervals, so RST0..RST7, RST0; and 17 is no divisor of 32
    c["marker_index_wraps"] = Case(smooth(272, 272), 50, 1, lambda t: t["intervals"] == 10)
    c["interval_crosses_a_row"] = Case(noise(5 * 16, 7 * 16, 6), 50, 1, lambda t: t["mcu_cols"] == 5 and t["intervals"] == 2)
    c["dummy_right"] = Case(noise(40, 32, 7), 90, 1, lambda t: t["dummy_right"] and not t["dummy_bottom"])
    c["dummy_bottom"] = Case(noise(32, 40, 8), 90, 1, lambda t: t["dummy_bottom"] and not t["dummy_right"])
    c["dummy_both"] = Case(noise(24, 24, 9), 90, 1, lambda t: t["dummy_bottom"] and t["dummy_right"])
    c["odd_chroma_pad"] = Case(noise(37, 53, 10), 90, 1, lambda t: t["mcu_cols"] == 3 and t["mcu_rows"] == 4)
    # 64 MCUs of noise with every quantiser 1: an interval of several of the coder's 4096-byte LDS windows
    c["hostile_noise_q100"] = Case(noise(96, 64, 11), 100, 0, lambda t: t["intervals"] == 2 and max(t["interval_bytes"]) > 4 * 4096)
    # the seams of the coder's 4096-byte window, by construction (the seeds were searched for: see below)
    c["ff_ends_a_window"] = Case(noise(96, 64, FF_SEAM_SEED), 100, 0, ff_ends_a_window)
    c["interval_fills_its_windows"] = Case(filled_interval_image(), 100, 0, interval_fills_its_windows)
    c["code_straddles_a_seam"] = Case(noise(96, 64, STRADDLE_SEED), 100, 0, code_straddles_a_seam)
    return c


FF_LAST_SEED = 1
EXACT_SEED = 14
# Found with the serial model's trace at quality 100, 4:4:4, the product's interval.  FF_SEAM_SEED and STRADDLE_SEED: the first seeds from
# 100 on whose 96 x 64 noise satisfies ff_ends_a_window and code_straddles_a_seam (seeds 100..162 hold two of the first kind and five
# of the second).  FILL_SEEDS = (image, last MCU, amplitude): image seeds from 200 on were tried until the last interval without its
# last MCU fell 300..3500 bits short of a multiple of 32768 bits; then, with every other MCU fixed and its bits known, the last MCU
# (on which, the interval being the image's last, nothing else depends) was drawn as noise(8, 8, 1000 + i), i < 40, scaled about 128
# by amplitude / 256, amplitude = 8, 16, ..., until the interval's bits came to within 1..7 of the multiple (about 1 candidate in
# 20 does once the amplitude is right).
FF_SEAM_SEED = 154
STRADDLE_SEED = 120
FILL_SEEDS = (201, 1012, 168)


def small_shapes():
    """name -> image: the shapes around every edge of the block grid, smooth and noise"""
    out = {}
    for cols, rows in [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (9, 40), (40, 9), (25, 25), (75, 100)]:
        out["smooth_%dx%d" % (cols, rows)] = smooth(cols, rows)
        out["noise_%dx%d" % (cols, rows)] = noise(cols, rows, cols * 100 + rows)
    return out
