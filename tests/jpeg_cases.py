"""The images of the device JPEG encoder's tests, built from fixed seeds.  branch_cases(): each is a small image made to reach one thing
in the coder, at the quality and subsampling it names and the product's restart interval; reached(trace) says, from the serial model's
symbol trace (tests/jpeg_model.py), that it does.  tests/test_jpeg_model.py asserts that for every case, without a GPU."""
import collections

import numpy as np

import jpeg_model as M

Case = collections.namedtuple("Case", "img quality subsampling reached")

BRANCHES = ["zrl", "zrl_twice", "no_eob", "all_zero_block", "dc_category_11", "ac_category_10", "negative_tie", "ff_inside", "ff_last_byte",
            "ends_on_a_byte", "less_than_an_interval", "exactly_k_intervals", "marker_index_wraps", "interval_crosses_a_row", "dummy_right",
            "dummy_bottom", "dummy_both", "odd_chroma_pad", "hostile_noise_q100"]


def noise(cols, rows, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 4), dtype=np.uint8)


def smooth(cols, rows):
    g = np.add.outer(np.arange(rows) * 3, np.arange(cols) * 2)[:, :, None] + np.array([0, 40, 90, 200])
    return g.astype(np.uint8)


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
    return c


FF_LAST_SEED = 1
EXACT_SEED = 14


def small_shapes():
    """name -> image: the shapes around every edge of the block grid, smooth and noise"""
    out = {}
    for cols, rows in [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (9, 40), (40, 9), (25, 25), (75, 100)]:
        out["smooth_%dx%d" % (cols, rows)] = smooth(cols, rows)
        out["noise_%dx%d" % (cols, rows)] = noise(cols, rows, cols * 100 + rows)
    return out
