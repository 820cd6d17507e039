"""A deflate writer with every knob exposed, and the judge the device inflate kernel (csrc/kernels_tiff.hip k_tiff_inflate) is held to.

The writer: an LSB-first bit writer, stored / fixed / dynamic blocks from explicit tokens (an int is a literal, a (length, distance)
pair a match) and explicit code lengths, the zlib wrapper, and a TIFF made from per-strip streams through tiff_model.write_tiff.
The judge is libz's own uncompress through ctypes: a strip is accepted exactly when uncompress(dst, expect, strip) returns Z_OK or
Z_BUF_ERROR with `expect` bytes delivered.  The reason class of a refusal comes from the text of Python's zlib error."""
import ctypes
import ctypes.util
import struct
import zlib

import numpy as np

import tiff_model as tm

# kTiffZlibHeader ... kTiffDataCheck in csrc/pf_common.hpp
REASON_OK, REASON_ZLIB_HEADER, REASON_BLOCK_HEADER, REASON_CODE_LENGTHS, REASON_INVALID_SYMBOL, REASON_FAR_BACK, REASON_DATA_CHECK = 0, 4, 5, 6, 7, 8, 9
_TEXT = [("incorrect header check", 4), ("unknown compression method", 4), ("invalid window size", 4), ("Error 2 ", 4),
         ("invalid block type", 5), ("invalid stored block lengths", 5),
         ("too many length or distance symbols", 6), ("invalid code lengths set", 6), ("invalid bit length repeat", 6),
         ("invalid literal/lengths set", 6), ("invalid distances set", 6), ("invalid code -- missing end-of-block", 6),
         ("invalid literal/length code", 7), ("invalid distance code", 7), ("invalid distance too far back", 8), ("incorrect data check", 9)]

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):
        """n bits of value, lowest first"""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """a Huffman code: its first (most significant) bit goes out first"""
        self.bits(int(format(code, "0%db" % n)[::-1], 2) if n else 0, n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        self.align()
        self.out += bytes(data)

    def getvalue(self):
        self.align()
        return bytes(self.out)


def canonical(lengths):
    """{symbol: (code, length)} of RFC 1951's canonical assignment (the lengths need not be a complete set)"""
    codes, code = {}, 0
    for ln in range(1, 16):
        for sym, have in enumerate(lengths):
            if have == ln:
                codes[sym] = (code, ln)
                code += 1
        code <<= 1
    return codes


def flat_lengths(used, n):
    """a complete set over the symbols `used` (at least two), n entries: lengths m - 1 and m"""
    used = sorted(set(used))
    assert len(used) >= 2
    m = (len(used) - 1).bit_length()
    short = (1 << m) - len(used)
    lens = [0] * n
    for k, sym in enumerate(used):
        lens[sym] = m - 1 if k < short else m
    return lens


def kraft(lengths):
    """sum of 2^-length in units of 2^-15: 32768 is complete"""
    return sum(1 << (15 - ln) for ln in lengths if ln)


def length_symbol(length):
    k = max(i for i in range(29) if LBASE[i] <= length) if length < 258 else 28
    return 257 + k, LEXT[k], length - LBASE[k]


def distance_symbol(dist):
    k = max(i for i in range(30) if DBASE[i] <= dist)
    return k, DEXT[k], dist - DBASE[k]


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, tuple):
            ln, dist = t
            for _ in range(ln):
                out.append(out[-dist])
        else:
            out.append(t)
    return bytes(out)


def used_symbols(tokens):
    lit, dist = {256}, set()
    for t in tokens:
        if isinstance(t, tuple):
            lit.add(length_symbol(t[0])[0])
            dist.add(distance_symbol(t[1])[0])
        else:
            lit.add(t)
    return lit, dist


def write_tokens(w, tokens, lit_lens, dist_lens, eob=True):
    """tokens: an int literal, a (length, distance) match, or ("lit", symbol) / ("dist", length, symbol) for raw symbols (286, 30, ...)"""
    lit, dist = canonical(lit_lens), canonical(dist_lens)
    for t in tokens:
        if not isinstance(t, tuple):
            w.code(*lit[t])
        elif t[0] == "lit":
            w.code(*lit[t[1]])
        else:
            raw = t[0] == "dist"
            sym, xb, xv = length_symbol(t[1] if raw else t[0])
            w.code(*lit[sym])
            w.bits(xv, xb)
            if raw:
                w.code(*dist[t[2]])
            else:
                sym, xb, xv = distance_symbol(t[1])
                w.code(*dist[sym])
                w.bits(xv, xb)
    if eob:
        w.code(*lit[256])


def stored_block(w, data, final, nlen=None):
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.out += struct.pack("<HH", len(data), (len(data) ^ 0xffff) if nlen is None else nlen)
    w.out += bytes(data)


def fixed_block(w, tokens, final, eob=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    write_tokens(w, tokens, FIXED_LIT, FIXED_DIST, eob)


def rle_lengths(lens, rle=True):
    """the code-length symbols of `lens`: [(symbol, extra value, first index, how many lengths it sets)], zlib's greedy runs"""
    seq, i = [], 0
    while i < len(lens):
        v, run = lens[i], 1
        while i + run < len(lens) and lens[i + run] == v:
            run += 1
        if rle and v == 0 and run >= 3:
            take = min(run, 138)
            seq.append((17, take - 3, i, take) if take <= 10 else (18, take - 11, i, take))
            i += take
        elif rle and run >= 4:
            seq.append((v, 0, i, 1))
            take = min(run - 1, 6)
            seq.append((16, take - 3, i + 1, take))
            i += 1 + take
        else:
            seq.append((v, 0, i, 1))
            i += 1
    return seq


def dynamic_block(w, tokens, lit_lens, dist_lens, final, cl_lens=None, cl_seq=None, rle=True, hlit=None, hdist=None, hclen=None, eob=True):
    """lit_lens (257.. entries) and dist_lens (1.. entries) as written; cl_seq: explicit [(symbol, extra value, ...)] instead of the
    run-length coding of the lengths; cl_lens: the 19 lengths of the code-length code (default: a flat complete set over the symbols
    used).  Returns the code-length sequence written."""
    seq = rle_lengths(list(lit_lens) + list(dist_lens), rle) if cl_seq is None else cl_seq
    if cl_lens is None:
        used = {s[0] for s in seq}
        cl_lens = flat_lengths(used if len(used) > 1 else used | {(min(used) + 1) % 19}, 19)
    n = max(k for k in range(19) if cl_lens[CL_ORDER[k]]) + 1 if hclen is None and any(cl_lens) else (hclen or 4)
    n = max(n, 4)
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(len(lit_lens) - 257 if hlit is None else hlit, 5)
    w.bits(len(dist_lens) - 1 if hdist is None else hdist, 5)
    w.bits(n - 4, 4)
    for k in range(n):
        w.bits(cl_lens[CL_ORDER[k]], 3)
    cl = canonical(cl_lens)
    for item in seq:
        sym, extra = item[0], item[1]
        w.code(*cl[sym])
        if sym >= 16:
            w.bits(extra, {16: 2, 17: 3, 18: 7}[sym])
    if tokens is not None:
        write_tokens(w, tokens, lit_lens, dist_lens, eob)
    return seq


def zstream(deflate, payload, cmf=0x78, flg=None, adler=None):
    """RFC 1950 around a deflate stream; flg None: FLEVEL 2, no dictionary, FCHECK made valid"""
    if flg is None:
        flg = 0x80
        flg += 31 - ((cmf << 8) + flg) % 31
    return bytes([cmf, flg]) + bytes(deflate) + struct.pack(">I", zlib.adler32(bytes(payload)) if adler is None else adler)


def dynamic_stream(tokens, lit_lens=None, dist_lens=None, **kw):
    """one final dynamic block around `tokens`; default lengths: flat complete sets over the symbols used"""
    lit, dist = used_symbols(tokens)
    if lit_lens is None:
        lit_lens = flat_lengths(lit if len(lit) > 1 else lit | {0}, max(max(lit) + 1, 257))
    if dist_lens is None:
        dist_lens = flat_lengths(dist, max(dist) + 1) if len(dist) > 1 else ([0] * max(dist) + [1] if dist else [0])
    w = BitWriter()
    seq = dynamic_block(w, tokens, lit_lens, dist_lens, True, **kw)
    return zstream(w.getvalue(), expand(tokens)), seq


def fixed_stream(tokens, **kw):
    w = BitWriter()
    fixed_block(w, tokens, True)
    return zstream(w.getvalue(), expand(tokens), **kw)


def compressobj_stream(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(bytes(data)) + c.flush()


# ---------------------------------------------------------------------------------------------------------------- the judge
_libz = None


def libz():
    global _libz
    if _libz is None:
        _libz = ctypes.CDLL(ctypes.util.find_library("z") or "libz.so.1")
        _libz.uncompress.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulong), ctypes.c_char_p, ctypes.c_ulong]
    return _libz


def uncompress(src, expect):
    """libz's uncompress into a buffer of `expect` bytes: (return code, the bytes delivered)"""
    dst = ctypes.create_string_buffer(max(expect, 1))
    n = ctypes.c_ulong(expect)
    r = libz().uncompress(dst, ctypes.byref(n), bytes(src), len(src))
    return r, dst.raw[:n.value]


def judge(src, expect):
    """(accepted, the strip's bytes if accepted, reason class if refused): the device decoder's contract for one strip"""
    r, got = uncompress(src, expect)
    if r in (0, -5) and len(got) == expect:   # Z_OK, Z_BUF_ERROR
        return True, got, REASON_OK
    try:
        zlib.decompressobj().decompress(bytes(src))
    except zlib.error as e:
        for text, reason in _TEXT:
            if text in str(e):
                return False, None, reason
        raise
    return False, None, REASON_OK   # the stream ends, validly or cut, before the strip is full


# ---------------------------------------------------------------------------------------------------------------- files
def strip_raws(img, rows_per_strip, predictor):
    """the bytes each strip must decode to (after horizontal differencing for predictor 2)"""
    img = np.ascontiguousarray(img, np.uint8)
    out = []
    for y0 in range(0, img.shape[0], rows_per_strip):
        raw = img[y0:y0 + rows_per_strip].astype(np.int16)
        if predictor == 2:
            raw[:, 1:] -= raw[:, :-1].copy()
        out.append((raw & 0xff).astype(np.uint8).tobytes())
    return out


def write_tiff(img, encode, rows_per_strip=1, predictor=1, compression=8, big_endian=False, align=0, streams=None):
    """a deflate TIFF: strip s holds streams[s] if given, else encode(the strip's bytes)"""
    img = np.ascontiguousarray(img, np.uint8)
    rps = min(rows_per_strip or img.shape[0], img.shape[0])
    raws = strip_raws(img, rps, predictor)
    blobs = {s: (streams[s] if streams and s in streams else encode(raw)) for s, raw in enumerate(raws)}
    return tm.write_tiff(img, 1, big_endian, rps, predictor, align, strip_bytes=blobs, extra_tags=[(259, 3, [compression])])


def strips(data):
    """[(the strip's compressed bytes, its expected size)] of a file"""
    data = bytes(data)
    f = tm.parse(data)
    cols, rows, spp = f[256][0], f[257][0], f[277][0]
    rps = min(f.get(278, [rows])[0], rows)
    return [(data[off:off + cnt], min(rps, rows - s * rps) * cols * spp) for s, (off, cnt) in enumerate(zip(f[273], f[279]))]


def decode(data):
    """the judge on every strip of a file: (BGRA image with refused strips zero-filled, [(accepted, reason)] per strip)"""
    data = bytes(data)
    f = tm.parse(data)
    cols, rows, spp, pred = f[256][0], f[257][0], f[277][0], f.get(317, [1])[0]
    pix, verdicts = bytearray(), []
    for src, expect in strips(data):
        ok, got, reason = judge(src, expect)
        verdicts.append((ok, reason))
        strip = np.frombuffer(got if ok else bytes(expect), np.uint8).reshape(-1, cols, spp)
        if pred == 2:
            strip = np.cumsum(strip, axis=1, dtype=np.uint64).astype(np.uint8)
        pix += strip.tobytes()
    return tm.expected_bgra(np.frombuffer(bytes(pix), np.uint8).reshape(rows, cols, spp)), verdicts
