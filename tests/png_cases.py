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


# ---- more than 1024 segments: the compaction scan sums two sizes per thread ----
MANY_COLS, MANY_ROWS, MANY_BAND, MANY_PERIOD = 341, 12300, 12, 84


def many_segments(segment_bytes):
    """341 x 12300: a scanline is 1365 bytes, 12 of them are exactly one segment, and there are 1025 segments.  The image repeats every
    84 rows: seven 12-row bands of different compressibility (flat, a gradient, noise that must be stored, and mixtures with a little
    noise in them), so that the segments' sizes differ, the filtered stream repeats with that period from segment 1 on (row 0 alone has
    no row above it) and tests/png_model.py has nine distinct segments to encode; 1025 is no multiple of 7."""
    cols, band = MANY_COLS, MANY_BAND
    assert (4 * cols + 1) * band == segment_bytes and MANY_ROWS * (4 * cols + 1) == 1025 * segment_bytes
    rng = _rng(31)
    flat = constant(cols, band, (40, 90, 200, 255))
    bands = [flat.copy(), smooth(cols, band), rng.integers(0, 256, (band, cols, 4), dtype=np.uint8)]
    b = flat.copy(); b[5] = rng.integers(0, 256, (cols, 4), dtype=np.uint8); bands.append(b)                       # one row of noise in flat colour
    b = smooth(cols, band); b[:, 100:120] = rng.integers(0, 256, (band, 20, 4), dtype=np.uint8); bands.append(b)    # a stripe of noise down a gradient
    b = smooth(cols, band); b[3:5] = rng.integers(0, 256, (2, cols, 4), dtype=np.uint8); bands.append(b)           # two rows of noise in a gradient
    b = constant(cols, band, (7, 7, 7, 0)); b[2:5, ::16] = rng.integers(0, 256, (3, len(range(0, cols, 16)), 4), dtype=np.uint8); bands.append(b)   # sparse noise pixels
    period = np.concatenate(bands)
    assert period.shape[0] == MANY_PERIOD
    return np.ascontiguousarray(np.tile(period, (MANY_ROWS // MANY_PERIOD + 1, 1, 1))[:MANY_ROWS])


# ---- cases that reach one branch each of the encoder (tests/test_png_decode_ref.py shows from tests/png_model.py that they do) ----
def gray(rows):
    """rows of one value per pixel -> an image with that value in all four channels"""
    return np.repeat((np.array(rows, np.int64) % 256)[:, :, None], 4, 2).astype(np.uint8)


# Rows 1..5: None, Sub, Up, Average and Paeth, in this order, have the strictly smallest sum (row 0 only gives row 1 its upper
# neighbours).  Found by a random search over a 14-value palette at 3 pixels a row; the sums are asserted, not trusted.
FILTER_STRICT = np.array(
    [[[255, 250, 250, 255], [200, 254, 254, 127], [60, 128, 128, 254]], [[254, 0, 60, 250], [1, 250, 1, 60], [250, 5, 5, 3]],
     [[200, 8, 60, 0], [128, 250, 129, 2], [127, 3, 255, 254]], [[200, 127, 128, 254], [129, 8, 129, 128], [1, 0, 129, 8]],
     [[60, 128, 60, 128], [127, 129, 255, 2], [127, 60, 8, 3]], [[60, 254, 1, 129], [127, 1, 250, 250], [60, 255, 128, 254]]], np.uint8)


def filter_cases():
    """name -> (image, row, what): `row` of the image is the row the case is about; `what` is ("strict", f), ("tie", a, b): a and b share the
    smallest sum and every other type lies above it, ("all_tie",), or ("margin", f, runner_up, by): f wins by exactly `by`"""
    out = {}
    for f in range(5):
        out["filter_strict_%d" % f] = (FILTER_STRICT, f + 1, ("strict", f))
    # None = Sub: per channel 1, 1, -1 has sum 3 and total variation 3; the upper row jumps, so Up, Average and Paeth pay for it
    out["filter_tie_0_1"] = (gray([[60, 200, 60], [1, 1, 255]]), 1, ("tie", 0, 1))
    # a first row has no upper row: Up is None and Paeth is Sub.  +1 / -1 alternating: None 1 a byte, Sub 2
    out["filter_tie_0_2"] = (gray([[1, 255, 1, 255]]), 0, ("tie", 0, 2))
    out["filter_tie_1_4"] = (gray([[100, 103, 106, 109]]), 0, ("tie", 1, 4))
    # the upper row is a ramp of step 10 and this row lies 1 off it: Paeth's nearest neighbour is the upper one everywhere
    out["filter_tie_2_4"] = (gray([[50, 60, 70, 80], [51, 59, 71, 79]]), 1, ("tie", 2, 4))
    # a falling ramp whose upper row is its left neighbour + 1: (left + up) >> 1 is the left neighbour, Up is one worse than Sub everywhere
    out["filter_tie_1_3"] = (gray([[1, 201, 198, 195], [200, 197, 194, 191]]), 1, ("tie", 1, 3))
    out["filter_all_tie_zero"] = (constant(3, 2, (0, 0, 0, 0)), 1, ("all_tie",))
    # residuals of 0x7f, 0x80, 0x81 decide by 1 a byte (4 a pixel): |0x80| = 128 is more than |0x7f| = |0x81| = 127
    out["filter_res_80"] = (gray([[1, 0x80]]), 0, ("margin", 1, 0, 4))        # None has 0x80, Sub 0x7f
    out["filter_res_81"] = (gray([[1, 0x81]]), 0, ("margin", 0, 1, 4))        # None has 0x81, Sub 0x80
    out["filter_res_7f"] = (gray([[3, 0x82]]), 0, ("margin", 0, 1, 4))        # None has 0x82 (126), Sub 0x7f
    # Without the last pixel all five sums are equal (per channel 1, 1, 0, ..., 0, 5: sum 7, variation 7) and None would win; the last
    # pixel repeats its neighbour: Sub adds nothing, None adds 5.  Its thread is 254, 255, 0 (second stride) and 0 (third stride).
    for cols in (255, 256, 257, 513):
        out["filter_last_pixel_%d" % cols] = (gray([[1, 1] + [0] * (cols - 4) + [5, 5]]), 0, ("margin", 1, 3, 12))
    return out


def filter_cols1():
    """one pixel a row: Sub is None and Paeth is Up.  Rows choose None (first row), Up, Up, Up, Average (50 = 100 >> 1), None"""
    return gray([[10], [11], [12], [100], [50], [1]])


def filter_first_row():
    """three equal rows: the first has no upper row and takes Sub, the others leave nothing under Up"""
    return gray([[100 + 3 * x for x in range(5)]] * 3)


class SubRow:
    """A one-row image from its filtered scanline.  The scanline is built byte by byte: the filter byte 1, then Sub residuals; the pixels
    are the running sums.  Residuals are small (1..12), so Sub's sum is far below None's and Average's (the pixels wander over all
    values), a first row's Up is None and its Paeth is Sub: the row is filtered with Sub, and the stream is the one built here."""
    PALETTE = tuple(range(1, 13))

    def __init__(self):
        self.s = [1]
        self.marks = {}

    def pos(self):
        return len(self.s)

    def lit(self, k=1):
        """k bytes that equal none of the four bytes before them: class 0, and whatever follows can be told from them"""
        for _ in range(k):
            self.s.append(next(v for v in self.PALETTE[len(self.s) % 5:] + self.PALETTE if v not in self.s[-4:]))
        return self

    def to(self, pos):
        assert pos >= len(self.s), (pos, len(self.s))
        return self.lit(pos - len(self.s))

    def run4(self, n, name=None):
        """n bytes that repeat the byte 4 back: class 4.  The four bytes before differ pairwise, so no position is class 1 as well."""
        if name:
            self.marks[name] = (len(self.s), n, 4)
        for _ in range(n):
            self.s.append(self.s[-4])
        return self

    def same(self, n, name=None, cls=None):
        """n bytes that repeat the byte 1 back: class 1 for the first three at most, class 4 from the fourth on (the byte 4 back is equal too)"""
        if name:
            self.marks[name] = (len(self.s), n if cls is None else cls[1], 1 if cls is None else cls[0])
        self.s.extend([self.s[-1]] * n)
        return self

    def image(self):
        while len(self.s) % 4 != 1:
            self.lit()
        res = np.array(self.s[1:], np.int64).reshape(-1, 4)
        rgba = (np.cumsum(res, 0) % 256).astype(np.uint8)
        return np.ascontiguousarray(rgba[None, :, [2, 1, 0, 3]])


RUN_LENGTHS = (2, 3, 4, 257, 258, 259, 260, 261, 516, 517)


def parse_runs():
    """class-4 runs of every length in RUN_LENGTHS, a literal between them, and class-1 runs of 1, 2 and 3 (a class-1 run cannot be
    longer: its fourth position would equal the byte 4 back, which is class 4) -> (image, marks)"""
    b = SubRow().lit(7)
    for n in RUN_LENGTHS:
        b.run4(n, "run4_%d" % n).lit(2)
    for n in (1, 2, 3):
        b.lit(4).same(n, "run1_%d" % n)
    b.lit(4).same(9, "both", cls=(4, 6))   # a constant stretch: class 0, 1, 1, 1, then 4: these bytes equal both neighbours
    b.marks["both"] = (b.marks["both"][0] + 3, 6, 4)
    b.lit(3)
    return b.image(), b.marks


def parse_chunks():
    """runs placed against the 64-position chunks a thread owns (positions inside the first segment) -> (image, marks)"""
    b = SubRow().lit(7)
    b.to(63).run4(9, "start_63").to(128).run4(9, "start_64").to(193).run4(9, "start_65")
    b.to(256 + 60).run4(4 + 192 + 10, "span3_short")                 # chunks 5, 6, 7 whole, ends in chunk 8: one match of 206
    b.to(640 + 10).run4(54 + 192 + 20, "span3_cut")                  # chunks 11, 12, 13 whole: 266 = 258 + 8, the cut lies in chunk 14
    b.to(1024 + 20).run4(43, "sep_last_a").lit().run4(30, "sep_last_b")      # the class-0 byte is position 1087, a chunk's last
    b.to(1280 + 20).run4(44, "sep_first_a").lit().run4(30, "sep_first_b")    # the class-0 byte is position 1344, a chunk's first
    b.to(1536 - 3).same(3 + 20, "change_1_4", cls=(1, 3))             # class 1 at 1533..1535, class 4 from 1536 on
    b.marks["change_4"] = (1536, 20, 4)
    b.to(1664 + 63).same(2, "pair_over_edge")                        # a class-1 run of 2 across a chunk edge: two literals
    b.to(1792 - 2).run4(64 + 4, "whole_chunk")                       # a chunk that is one run from end to end and no more
    b.lit(3)
    return b.image(), b.marks


def parse_segment_end():
    """a class-4 run that ends on the first segment's last byte; the second segment begins with literals -> (image, marks)"""
    b = SubRow().lit(9)
    b.to(16380 - 300).run4(300, "to_last_byte").lit(20)
    return b.image(), b.marks


def parse_segment_cross():
    """a class-4 run across the segment boundary: positions 0..3 of the second segment have nothing to match and are literals, the run
    goes on from position 4 -> (image, marks)"""
    b = SubRow().lit(9)
    b.to(16380 - 100).run4(100 + 150, "across").lit(5)
    return b.image(), b.marks


def parse_segment_cross_constant():
    """a constant stretch across the segment boundary: the second segment starts class 0, 1, 1, 1 and goes on at distance 4"""
    b = SubRow().lit(9)
    b.to(16380 - 100).same(100 + 150, "across").lit(5)
    return b.image(), b.marks


def _tail(cols, rows):
    img = smooth(cols, rows)
    img[-1, -1] = (200, 131, 77, 250)
    return img


def tail_cases():
    """name -> (image, bytes in the last segment): streams of one segment and 1, 3, 5 bytes, where the last dword load reads padding"""
    return {"tail_1_4095x1": (_tail(4095, 1), 1), "tail_3_32x127": (_tail(32, 127), 3), "tail_5_1x3277": (_tail(1, 3277), 5)}


def fibonacci_row(cols):
    """One row whose Sub residuals are the byte values 2, 3, 4, ... with Fibonacci counts 2, 3, 5, 8, ... (the last count takes what is left
    of 4 * cols), laid out greedily: always the most numerous value left that differs from the byte 1 back and the byte 4 back, so that
    no position matches and every token is a literal.  With the filter byte and the end-of-block symbol (one each) the histogram is
    1, 1, 2, 3, 5, ...: a Huffman tree as deep as it has symbols, less one."""
    total = 4 * cols
    counts, a, b = [], 2, 3
    while sum(counts) + a <= total:
        counts.append(a); a, b = b, a + b
    counts[-1] += total - sum(counts)
    return _no_match_row({v + 2: c for v, c in enumerate(counts)})


def _no_match_row(left):
    """one row whose Sub residuals are the values of `left` (value -> count, 4 * cols in all), laid out greedily so that nothing matches"""
    left = dict(left)
    total = sum(left.values())
    s = [1]
    for _ in range(total):
        v = max((v for v in left if left[v] and v != s[-1] and (len(s) < 4 or v != s[-4])), key=lambda v: (left[v], v))
        left[v] -= 1; s.append(v)
    res = np.array(s[1:], np.int64).reshape(-1, 4)
    return np.ascontiguousarray((np.cumsum(res, 0) % 256).astype(np.uint8)[None, :, [2, 1, 0, 3]])


# how many literal / length symbols get a code of each length in limit7_row: Kraft sum 1 at 11 bits, and as counts of code-length
# symbols (with 18 x 2, 0 x 3 and 1 x 2 from the unused symbols and the distance lengths) 1 1 2 2 2 3 3 5 8 21 34 68: a Huffman tree 8 deep
LIMIT7_LENGTH_COUNTS = {3: 2, 4: 1, 5: 1, 6: 21, 7: 34, 8: 3, 9: 5, 10: 8, 11: 68}


def limit7_row():
    """512 x 1: 141 residual values with counts 2 ** (11 - L), L distributed as LIMIT7_LENGTH_COUNTS says (found by a random search over such
    tables), so that the literal / length code has exactly these lengths: the filter byte and the end of the block take two of the 68
    counts of 1, and one of the two counts of 256 is 258 so that the row is whole pixels.  The values 2..72, 186..255 get the lengths in an
    order in which equal lengths are never neighbours (always the most numerous length left that differs from the one before), so no
    length is sent as a repeat, and the code-length code sees the counts above."""
    left = dict(LIMIT7_LENGTH_COUNTS)
    left[11] -= 2
    order, prev = [], None
    while any(left.values()):
        prev = max((l for l in left if left[l] and l != prev), key=lambda l: (left[l], l))
        left[prev] -= 1; order.append(prev)
    values = list(range(2, 73)) + list(range(186, 256))      # 141 residuals of small magnitude (at most 72), so that Sub wins the row
    counts = {v: 1 << (11 - l) for v, l in zip(values, order)}
    counts[min(v for v in counts if counts[v] == 256)] += 2
    return _no_match_row(counts)


def limit_cases():
    """name -> (image, which code, the depth of that code's unrestricted tree): 16 and 18 > 15 for the literal / length code, 8 > 7 for the
    code-length code"""
    return {"limit15_1045x1": (fibonacci_row(1045), "litlen", 16), "limit15_2736x1": (fibonacci_row(2736), "litlen", 18),
            "limit7_512x1": (limit7_row(), "cl", 8)}


def lengths_repeat_row():
    """26 x 1: 26 residual values, four of each, nothing matches.  Their code lengths are runs of 5s and 4s that go out as the length,
    then 16s: three full repeats of 6 with two 5s left over, and a repeat of 4"""
    return _no_match_row({2 + i: 4 for i in range(26)})


def threshold_cases():
    """name -> (image, coded bytes - stored bytes): three pixels of 0 / 1 noise, a stream of 13 bytes whose coded form is one byte
    smaller than the stored one (23), equal to it, and one byte larger; found by trying seeds.  Only the first is coded."""
    return {"threshold_%s" % nm: (_rng(seed).integers(0, 2, (1, 3, 4), dtype=np.uint8), d) for nm, seed, d in (("below", 2, -1), ("equal", 0, 0), ("above", 3, 1))}


def branch_cases():
    """name -> image: every case above, for the byte comparisons"""
    out = {k: v[0] for k, v in filter_cases().items() if not k.startswith("filter_strict")}
    out["filter_strict"] = FILTER_STRICT
    out["filter_cols1"] = filter_cols1()
    out["filter_first_row"] = filter_first_row()
    for fn in (parse_runs, parse_chunks, parse_segment_end, parse_segment_cross, parse_segment_cross_constant):
        out[fn.__name__] = fn()[0]
    out["lengths_repeat_26x1"] = lengths_repeat_row()
    for group in (tail_cases(), limit_cases(), threshold_cases()):
        out.update({k: v[0] for k, v in group.items()})
    return out
