"""The JPEG decoder's shared cases: files written by Pillow (libjpeg-turbo) and by the encoder's model
(tests/jpeg_model.py), each with the property it was made for, asserted on the model's trace (tests/jpegd_model.py) where it was
searched for.  Everything is generated from committed seeds; nothing is read from disk."""
import functools
import io

import numpy as np
from PIL import Image

import jpeg_model
import jpegd_model

S_PRODUCT = 64       # pf_common.hpp kJpegdSubseq
S_MIN = 32           # ... kJpegdSubseqMin
LANES = 256          # ... kJpegdLanes
SEED = 20261021      # the seed of every search below

SUBSAMPLING = {"444": 0, "422": 1, "420": 2}


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def ramp(w, h, seed=0):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 255 // max(1, w - 1)), (y * 255 // max(1, h - 1)), ((x + y + seed) * 3 % 256)], axis=2).astype(np.uint8)


def scene(w, h, seed):
    """photo-like: smooth gradients, a few hard edges and mild noise"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([128 + 100 * np.sin(x / 37.0 + seed) * np.cos(y / 23.0), 128 + 90 * np.cos(x / 51.0) * np.sin(y / 41.0 + 1), 100 + 0.1 * x + 0.07 * y], axis=2)
    for _ in range(6):
        cx, cy, r = rng.integers(0, w), rng.integers(0, h), rng.integers(4, max(5, min(w, h) // 3))
        img[(x - cx) ** 2 + (y - cy) ** 2 < r * r] = rng.integers(0, 256, 3)
    img += rng.normal(0, 3, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def pil_jpeg(rgb, quality=90, sub="420", optimize=False, restart=0, grey=False):
    """restart: MCUs per interval (Pillow's restart_marker_blocks), 0 none"""
    im = Image.fromarray(rgb)
    kw = dict(quality=quality, optimize=optimize)
    if grey:
        im = im.convert("L")
    else:
        kw["subsampling"] = SUBSAMPLING[sub]
    if restart:
        kw["restart_marker_blocks"] = restart
    f = io.BytesIO()
    im.save(f, "JPEG", **kw)
    return f.getvalue()


def pillow_bgra(data):
    rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    return jpegd_model.bgra(rgb)


def _mcu_row(w, sub):
    return -(-w // (8 if sub in ("444", "grey") else 16))


@functools.lru_cache(maxsize=None)
def grid_cases():
    """the grid the arithmetic was held to Pillow on, thinned so that every value of every axis occurs with every size: (name, file)"""
    sizes = [(1, 1), (8, 8), (7, 9), (17, 17), (16, 16), (31, 33), (64, 48), (35, 7), (3, 5), (4, 4)]
    out = []
    k = 0
    for (w, h) in sizes:
        for content in ("noise", "ramp"):
            img = noise(w, h, SEED + k) if content == "noise" else ramp(w, h, k)
            for sub in ("444", "422", "420", "grey"):
                q = (1, 50, 90, 100)[k % 4]; opt = bool((k // 4) % 2); rst = (0, 1, 3, _mcu_row(w, sub))[(k // 2) % 4]
                k += 1
                data = pil_jpeg(img, q, sub if sub != "grey" else "444", opt, rst, grey=sub == "grey")
                out.append(("%dx%d-%s-%s-q%d-%s-r%d" % (w, h, content, sub, q, "opt" if opt else "std", rst), data))
    return out


@functools.lru_cache(maxsize=None)
def interval_cases():
    """the encoder's own restart intervals (32 and 64 MCUs), more than 8 intervals so that the marker index wraps, and one long interval"""
    out = []
    img = scene(200, 120, SEED)
    bgra = jpegd_model.bgra(img)
    out.append(("enc-420-r32", jpeg_model.encode(bgra, 90, 1)))
    out.append(("enc-444-r64", jpeg_model.encode(bgra, 90, 0)))
    data = pil_jpeg(img, 85, "420", False, 5)
    info = jpegd_model.parse(data)
    mc, mr, _ = jpegd_model.geometry(info)
    assert -(-mc * mr // 5) > 8
    out.append(("wrap-420-r5", data))
    # one interval of more luma blocks than a workgroup of the DC pass sums (2048): the pass's chunk sums are used
    data = pil_jpeg(scene(520, 296, SEED + 1), 50, "420")
    mc, mr, _ = jpegd_model.geometry(jpegd_model.parse(data))
    assert 2048 < 4 * mc * mr <= 4096
    out.append(("dc-two-chunks-420", data))
    return out


def _has(result, S, what):
    """does the accepted decode `result` show the seam property `what` at subsequence size S?"""
    info = result["info"]; tr = result["trace"]
    seg = result["seg"]; n = len(seg)
    starts = np.array(tr["starts"], np.int64); lens = np.array(tr["lens"], np.int64)
    bounds = np.arange(S, n, S, dtype=np.int64)          # byte offsets of the subsequence boundaries inside the segment
    if what == "ff_split":
        return any(seg[b - 1] == 0xFF and seg[b] == 0x00 for b in bounds)
    if what == "rst_split":
        return any(seg[b - 1] == 0xFF and 0xD0 <= seg[b] <= 0xD7 for b in bounds)
    if what == "word_split":      # a code word of at least 20 bits with a boundary strictly inside it
        big = np.flatnonzero(lens >= 20)
        return any(((starts[k] // (8 * S)) != ((starts[k] + lens[k] - 1) // (8 * S))) for k in big)
    if what == "block_ends_on_boundary":
        st = tr["states"]
        first = [k for k in range(len(st)) if st[k][1] == 0]        # code words that start a block
        return any(starts[k] % (8 * S) == 0 and starts[k] > 0 for k in first)
    if what == "no_block_completes":
        st = tr["states"]
        done = np.array([s[2] for s in st], np.int64)               # blocks completed before each code word
        sub = starts // (8 * S)
        for i in range(1, n // S):
            sel = np.flatnonzero(sub == i)
            if len(sel) and done[sel[0]] == done[sel[-1]] and (sel[-1] + 1 < len(done) and done[sel[-1] + 1] == done[sel[0]]):
                return True
        return False
    if what == "several_intervals":
        ends = np.array(tr["piece_end_bits"], np.int64) // 8
        return any(np.count_nonzero((ends > i * S) & (ends <= (i + 1) * S)) >= 3 for i in range(-(-n // S)))
    if what == "last_one_byte":
        return n % S == 1
    if what == "one_subsequence":
        return n <= S
    if what == "more_than_lanes":
        return -(-n // S) == LANES + 1
    raise KeyError(what)


def _decode(data):
    r = jpegd_model.decode(data)
    r["seg"] = data[r["info"]["begin"]:r["info"]["end"]]
    return r


SEAMS = ("ff_split", "rst_split", "word_split", "block_ends_on_boundary", "no_block_completes", "several_intervals", "last_one_byte",
         "one_subsequence", "more_than_lanes")


def _candidates(what, S, k):
    """the k-th candidate file of the search for (what, S)"""
    seed = SEED + 1000 * SEAMS.index(what) + k
    if what == "no_block_completes":
        return pil_jpeg(noise(24, 16, seed), 100, "444")
    if what == "several_intervals":
        return pil_jpeg(ramp(64 + 8 * (k % 3), 32, k), 30, "420", False, 1)
    if what == "rst_split":
        return pil_jpeg(scene(72, 40 + 8 * (k % 5), seed), 75 + k % 20, "420", False, 1 + k % 3)
    if what == "one_subsequence":
        return pil_jpeg(ramp(8, 8, k), 20, "444")
    if what == "last_one_byte":
        return pil_jpeg(scene(40, 24 + (k % 7), seed), 60 + k % 35, "422")
    return pil_jpeg(scene(56 + 8 * (k % 3), 40, seed), 70 + k % 30, ("444", "422", "420")[k % 3], bool(k & 1))


@functools.lru_cache(maxsize=None)
def seam_case(what, S):
    """a file that shows seam property `what` at subsequence size S, found by a seeded search; asserts that it still does"""
    if what == "more_than_lanes":
        target = LANES * S + 1
        for k in range(4000):
            data = _trim_to(target, S, k)
            if data is not None:
                r = _decode(data)
                assert r["accept"] and _has(r, S, what)
                return data
        raise AssertionError("no %s case at S = %d" % (what, S))
    for k in range(3000):
        data = _candidates(what, S, k)
        r = _decode(data)
        if r["accept"] and _has(r, S, what):
            return data
    raise AssertionError("no %s case at S = %d" % (what, S))


def _trim_to(target, S, k):
    """a grey noise file whose segment has between LANES * S + 1 and (LANES + 1) * S bytes: width searched by bisection on the seed-k image"""
    lo, hi = 8, 8192
    h = 16
    best = None
    while lo <= hi:
        w = (lo + hi) // 2
        data = pil_jpeg(noise(w, h, SEED + 77 + k), 90, "444", grey=True)
        info = jpegd_model.parse(data)
        n = info["end"] - info["begin"]
        if n < target:
            lo = w + 1
        elif n > target + S - 1:
            hi = w - 1
        else:
            best = data; break
    return best


def seam_cases():
    """(name, S, file) for every seam at the product's S and at the smallest"""
    out = []
    for what in SEAMS:
        for S in (S_PRODUCT, S_MIN):
            out.append(("%s-S%d" % (what, S), S, seam_case(what, S)))
    return out


def all_valid_cases():
    return grid_cases() + interval_cases() + [(n, d) for n, _, d in seam_cases()]


def _patched(data, marker, offset, value):
    """`data` with the byte `offset` bytes behind the first `marker` segment's marker replaced"""
    k = data.index(bytes([0xFF, marker]))
    v = bytearray(data); v[k + offset] = value
    return bytes(v)


@functools.lru_cache(maxsize=None)
def refusals():
    """one patched header per refusal of the contract, a progressive and a CMYK file of Pillow's: name -> (file, a word of the reason)"""
    base = pil_jpeg(scene(32, 24, 1), 80, "420")
    grey = pil_jpeg(scene(32, 24, 1), 80, grey=True)
    sos = base.index(b"\xff\xda")
    f = io.BytesIO(); Image.fromarray(scene(32, 24, 1)).save(f, "JPEG", progressive=True); progressive = f.getvalue()
    f = io.BytesIO(); Image.fromarray(scene(32, 24, 1)).convert("CMYK").save(f, "JPEG"); cmyk = f.getvalue()
    adobe = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    no_jfif = base[:2] + base[2 + 18:]                       # without the APP0 segment
    assert base[2:4] == b"\xff\xe0" and base[4:6] == b"\x00\x10"
    rgb_ids = bytearray(no_jfif)
    k = rgb_ids.index(b"\xff\xc0"); rgb_ids[k + 10] = ord("R"); rgb_ids[k + 13] = ord("G"); rgb_ids[k + 16] = ord("B")
    k = rgb_ids.index(b"\xff\xda"); rgb_ids[k + 5] = ord("R"); rgb_ids[k + 7] = ord("G"); rgb_ids[k + 9] = ord("B")
    return {
        "SOF1": (_patched(base, 0xC0, 1, 0xC1), "SOF1"),
        "SOF2 patched": (_patched(base, 0xC0, 1, 0xC2), "SOF2"),
        "progressive": (progressive, "SOF2"),
        "12-bit": (_patched(base, 0xC0, 4, 12), "12-bit"),
        "four components": (cmyk, "four components"),
        "4:4:0": (_patched(base, 0xC0, 11, 0x12), "sampling"),
        "4:1:1": (_patched(base, 0xC0, 11, 0x41), "sampling"),
        "chroma 2x1": (_patched(base, 0xC0, 14, 0x21), "sampling"),
        "a second scan": (base[:sos] + base[sos:-2] + base[sos:], "several scans"),
        "DNL": (_patched(base, 0xC0, 5, 0) if base[base.index(b"\xff\xc0") + 6] == 0 else _patched(_patched(base, 0xC0, 5, 0), 0xC0, 6, 0), "height 0"),
        "Pq 1": (_patched(base, 0xDB, 4, 0x10), "16-bit quantisation"),
        "Adobe transform 0": (no_jfif[:2] + adobe + no_jfif[2:], "RGB"),
        "ids R G B": (bytes(rgb_ids), "RGB"),
        "a missing Huffman table": (_patched(base, 0xDA, 6, 0x33), "missing Huffman table"),
        "a bad Huffman table": (_patched(base, 0xC4, 5, 3), "bad Huffman table"),
        "no EOI": (base[:-2], "no EOI"),
        "grey 2x2": (_patched(grey, 0xC0, 11, 0x22), "sampling"),
    }


@functools.lru_cache(maxsize=None)
def handmade_long_block():
    """A grey 48 x 8 file no encoder writes, for the seam "a subsequence in which no block completes" at every S up to 256 bytes (an encoder-written block of
    8-bit samples holds at most 63 * 26 + 27 bits, 208 bytes before stuffing, so quality-100 noise shows the seam only at S = 32 and 64): its AC table
    gives the symbol (run 0, size 8) the 16-bit code 1111111111111110, and every AC coefficient is +255 (eight 1-bits), so that a block
    is 63 words of 24 bits in which every run of 23 ones holds two 0xFF bytes: more than 300 bytes with their stuffing.  The IDCT
    leaves libjpeg's range table, where the contract clamps and libjpeg wraps, so this file is held to the model, not to Pillow."""
    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body
    nblocks = 6
    head = b"\xff\xd8" + seg(0xDB, b"\x00" + bytes([1] * 64)) + seg(0xC0, b"\x08" + (8).to_bytes(2, "big") + (8 * nblocks).to_bytes(2, "big") + b"\x01\x01\x11\x00")
    head += seg(0xC4, b"\x00" + bytes([1] + [0] * 15) + b"\x00")                                       # DC: category 0 is '0'
    head += seg(0xC4, b"\x10" + bytes([1] * 16) + bytes([0x00] + list(range(0x11, 0x1F + 1))[:14] + [0x08]))   # AC: the last, 16-bit code is (0, 8)
    head += seg(0xDA, b"\x01\x01\x00\x00\x3f\x00")
    bits = ""
    for _ in range(nblocks):
        bits += "0" + ("1111111111111110" + "11111111") * 63
    bits += "1" * (-len(bits) % 8)
    raw = int(bits, 2).to_bytes(len(bits) // 8, "big")
    data = head + raw.replace(b"\xff", b"\xff\x00") + b"\xff\xd9"
    r = _decode(data)
    assert r["accept"] and _has(r, S_PRODUCT, "no_block_completes") and _has(r, 256, "no_block_completes")
    return data


def model_only_cases():
    """valid files that are held to the model alone: (name, file)"""
    return [("no_block_completes-S%d-handmade" % S_PRODUCT, handmade_long_block())]
