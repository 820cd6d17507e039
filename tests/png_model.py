"""A serial model of the device PNG encoder: numpy + stdlib only, written from DESIGN.md section 8.2, RFC 1951 and the constants of
csrc/png_frame.hpp.  encode(img) gives the file the encoder must give, byte for byte, and says how it got there.

Nothing here is parallel: the filter sums are whole planes, a segment's tokens come from one left-to-right scan, the Huffman code from
one two-queue merge.  It is slow (pure-Python token and bit loops), so the images whose every segment it encodes stay small (a few
dozen segments at the most).  Byte equality with the device is not limited to them: a stream of more than a thousand segments is
within the model's reach where the segments repeat, and encode(img, cache={}) encodes each distinct (segment, last) once.
"""
import heapq
import zlib

import numpy as np

import png_decode_ref as R

SEG = 16380          # png_frame::kSegBytes
OVERHEAD = 10        # png_frame::kSegOverhead: stored-block header 5 + sync marker 5
PIECE = 258          # the longest deflate match
N_LITLEN = 286       # literal / length codes sent (HLIT = 29)
DIST_LENS = (1, 0, 0, 1)   # distance codes sent (HDIST = 3): distance 1 is symbol 0, distance 4 is symbol 3, one bit each
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)   # RFC 1951, 3.2.7; all 19 are sent (HCLEN = 15)


# ---- filter ----------------------------------------------------------------------------------------------------------------------
def residual_planes(bgra):
    """(5, rows, cols, 4) uint8: the residuals of every filter type, in RGBA order"""
    v = np.asarray(bgra, np.uint8)[:, :, [2, 1, 0, 3]].astype(np.int32)
    a = np.zeros_like(v); a[:, 1:] = v[:, :-1]
    b = np.zeros_like(v); b[1:] = v[:-1]
    c = np.zeros_like(v); c[1:, 1:] = v[:-1, :-1]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    preds = [np.zeros_like(v), a, b, (a + b) >> 1, paeth]
    return np.stack([((v - q) & 255) for q in preds]).astype(np.uint8)


def filter_sums(bgra):
    """(rows, 5) int64: per row and type the sum of absolute residuals, the residual bytes read as signed"""
    return np.abs(residual_planes(bgra).view(np.int8).astype(np.int64)).sum(axis=(2, 3)).T


def filter_image(bgra):
    """-> (the filtered scanlines as bytes, the filter type per row, the sums)"""
    planes = residual_planes(bgra)
    sums = filter_sums(bgra)
    types = np.argmin(sums, axis=1)                  # the first of equal minima: the lowest type number
    rows, cols = planes.shape[1], planes.shape[2]
    lines = np.empty((rows, 1 + 4 * cols), np.uint8)
    lines[:, 0] = types
    lines[:, 1:] = planes[types, np.arange(rows)].reshape(rows, 4 * cols)
    return lines.tobytes(), types, sums


# ---- tokens ----------------------------------------------------------------------------------------------------------------------
def classes(seg):
    """class of every position of one segment: 4 if the byte equals the byte 4 back, else 1 if it equals the byte 1 back, else 0"""
    b = np.frombuffer(seg, np.uint8)
    cls = np.zeros(len(b), np.int64)
    cls[1:][b[1:] == b[:-1]] = 1
    cls[4:][b[4:] == b[:-4]] = 4
    return cls


def runs(cls):
    """[(start, length, class)] of the maximal runs of equal class, left to right"""
    out, i, n = [], 0, len(cls)
    edges = np.flatnonzero(np.diff(cls)) + 1
    for e in list(edges) + [n]:
        out.append((i, int(e) - i, int(cls[i])))
        i = int(e)
    return out


def parse(seg):
    """tokens of one segment: an int is a literal byte, (length, distance) a match"""
    toks = []
    for start, length, t in runs(classes(seg)):
        if t == 0:
            toks.extend(seg[start:start + length])
            continue
        for a in range(start, start + length, PIECE):
            piece = min(PIECE, start + length - a)
            if piece >= 3:
                toks.append((piece, t))
            else:
                toks.extend(seg[a:a + piece])
    return toks


def length_symbol(length):
    """(symbol, extra bits, their value) of a match length 3..258, RFC 1951 3.2.5's table built row by row"""
    if length == 258:
        return 285, 0, 0
    base, sym = 3, 257
    for extra in (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5):
        if length < base + (1 << extra):
            return sym, extra, length - base
        base += 1 << extra; sym += 1
    raise ValueError(length)


def histogram(toks):
    h = [0] * N_LITLEN
    for t in toks:
        h[t if isinstance(t, int) else length_symbol(t[0])[0]] += 1
    h[256] += 1                                      # the end of the block
    return h


# ---- Huffman ---------------------------------------------------------------------------------------------------------------------
def plain_huffman(freq):
    """(deepest leaf, sum of freq * depth) of a textbook heapq Huffman tree over the symbols in use; independent of code_lengths below.
    The cost is that of every optimal prefix code; the depth is this tree's."""
    heap = [(f, i, 0) for i, f in enumerate(freq) if f]     # (weight, tie-break, height)
    if len(heap) < 2:
        return len(heap), sum(freq)
    heapq.heapify(heap)
    cost, tie = 0, len(freq)
    while len(heap) > 1:
        w1, _, h1 = heapq.heappop(heap); w2, _, h2 = heapq.heappop(heap)
        cost += w1 + w2
        heapq.heappush(heap, (w1 + w2, tie, max(h1, h2) + 1)); tie += 1
    return heap[0][2], cost


def code_lengths(freq, maxbits):
    """-> (the code length per symbol, whether a depth had to be limited).  Symbols in use ordered by (freq, index); the tree by the
    two-queue merge, a leaf before an inner node of equal weight; depths beyond maxbits counted at maxbits, then miniz's fold: while the
    Kraft sum is too large, drop one code of the longest length and split one of the longest shorter length in two; the shortest lengths
    go to the most frequent symbols.  One symbol in use: it and one unused symbol (symbol 0, or 1 if it is symbol 0) get one bit each."""
    order = sorted((f, s) for s, f in enumerate(freq) if f)
    lens = [0] * len(freq)
    m = len(order)
    if m == 0:
        return lens, False
    if m == 1:
        s = order[0][1]
        lens[s] = 1; lens[1 if s == 0 else 0] = 1
        return lens, False
    leaves = [(f, ("leaf", k)) for k, (f, _) in enumerate(order)]
    inner = []
    li = ii = 0

    def take():
        nonlocal li, ii
        if li < m and (ii >= len(inner) or leaves[li][0] <= inner[ii][0]):
            li += 1
            return leaves[li - 1]
        ii += 1
        return inner[ii - 1]
    for _ in range(m - 1):
        x = take(); y = take()
        inner.append((x[0] + y[0], ("node", x[1], y[1])))
    depth = [0] * m
    stack = [(inner[-1][1], 0)]
    while stack:
        node, d = stack.pop()
        if node[0] == "leaf":
            depth[node[1]] = d
        else:
            stack.append((node[1], d + 1)); stack.append((node[2], d + 1))
    limited = max(depth) > maxbits
    count = [0] * (maxbits + 1)
    for d in depth:
        count[min(d, maxbits)] += 1
    total = sum(count[l] << (maxbits - l) for l in range(1, maxbits + 1))
    while total > 1 << maxbits:
        count[maxbits] -= 1
        for l in range(maxbits - 1, 0, -1):
            if count[l]:
                count[l] -= 1; count[l + 1] += 2
                break
        total -= 1
    k = m
    for l in range(1, maxbits + 1):
        for _ in range(count[l]):
            k -= 1
            lens[order[k][1]] = l
    return lens, limited


def canonical_codes(lens):
    """RFC 1951 3.2.2, then bit-reversed: deflate sends Huffman codes from their most significant bit"""
    maxl = max(lens)
    count = [0] * (maxl + 2)
    for l in lens:
        if l:
            count[l] += 1
    nxt, code = [0] * (maxl + 2), 0
    for l in range(1, maxl + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            out[s] = int(format(nxt[l], "0%db" % l)[::-1], 2)
            nxt[l] += 1
    return out


def run_length_code(lens):
    """the code lengths as (code-length symbol, extra value): maximal runs of one value; a run of zeros goes out as 18s (11..138) while 11
    or more remain, then one 17 (3..10) if 3 or more remain, then single zeros; a run of another value as the value, then 16s (3..6, as
    many as possible first) while 3 or more remain, then the value itself"""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, run = lens[i], 1
        while i + run < n and lens[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                k = min(run, 138); out.append((18, k - 11)); run -= k
            if run >= 3:
                out.append((17, run - 3)); run = 0
            out.extend([(0, 0)] * run)
        else:
            out.append((v, 0)); run -= 1
            while run >= 3:
                k = min(run, 6); out.append((16, k - 3)); run -= k
            out.extend([(v, 0)] * run)
    return out


# ---- a segment's bytes -----------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self):
        self.out = bytearray(); self.acc = 0; self.n = 0; self.total = 0

    def put(self, v, n):
        self.acc |= v << self.n; self.n += n; self.total += n
        while self.n >= 8:
            self.out.append(self.acc & 255); self.acc >>= 8; self.n -= 8

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)


def _marker(last):
    """an empty stored block: its three header bits (in a byte of their own here), LEN = 0, NLEN = 0xFFFF"""
    return bytes([1 if last else 0, 0, 0, 0xff, 0xff])


def encode_segment(seg, last):
    """-> (bytes, info) of one segment: one dynamic block (or one stored block where that is not larger) and the sync marker"""
    n = len(seg)
    toks = parse(seg)
    hist = histogram(toks)
    lens, lim15 = code_lengths(hist, 15)
    seq = run_length_code(lens + list(DIST_LENS))
    cl_hist = [0] * 19
    for s, _ in seq:
        cl_hist[s] += 1
    cl_lens, lim7 = code_lengths(cl_hist, 7)
    codes, cl_codes = canonical_codes(lens), canonical_codes(cl_lens)
    w = _Bits()
    w.put(0, 1); w.put(2, 2)                         # BFINAL = 0, BTYPE = dynamic
    w.put(N_LITLEN - 257, 5); w.put(len(DIST_LENS) - 1, 5); w.put(19 - 4, 4)
    for s in CL_ORDER:
        w.put(cl_lens[s], 3)
    for s, extra in seq:
        w.put(cl_codes[s], cl_lens[s])
        if s >= 16:
            w.put(extra, {16: 2, 17: 3, 18: 7}[s])
    header_bits = w.total
    body_bits = sum(h * l for h, l in zip(hist, lens)) + sum(length_symbol(t[0])[1] + 1 for t in toks if not isinstance(t, int))
    coded_bytes = (header_bits + body_bits + 3 + 7) // 8 + 4
    stored = not coded_bytes < n + OVERHEAD
    info = {"n": n, "stored": stored, "tokens": toks, "coded_bytes": coded_bytes, "limited15": lim15, "limited7": lim7,
            "depth_litlen": plain_huffman(hist)[0], "depth_cl": plain_huffman(cl_hist)[0], "lens": lens, "cl_lens": cl_lens, "hist": hist, "cl_hist": cl_hist}
    if stored:
        return bytes([0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + seg + _marker(last), info
    for t in toks:
        if isinstance(t, int):
            w.put(codes[t], lens[t])
        else:
            sym, nextra, extra = length_symbol(t[0])
            w.put(codes[sym], lens[sym]); w.put(extra, nextra); w.put(1 if t[1] == 4 else 0, 1)
    w.put(codes[256], lens[256])
    w.put(1 if last else 0, 3)                       # the marker's BFINAL and BTYPE = stored
    w.align()
    out = bytes(w.out) + b"\0\0\xff\xff"
    assert len(out) == coded_bytes
    return out, info


ADLER_BY_DEFINITION_MAX = 1 << 20   # stream bytes up to which encode() also sums the Adler-32 by its definition, byte by byte in Python


def encode(img, cache=None):
    """BGRA (rows, cols, 4) -> (the PNG file, info).  cache: a dict that keeps encode_segment's result per (segment bytes, last), for
    streams whose segments repeat.  info["types"]: the filter type per row, info["sums"]: the five sums per row,
    info["segments"]: per segment n, stored, tokens, coded_bytes, limited15 / limited7 (the two-queue tree went beyond the limit),
    depth_litlen / depth_cl (the deepest leaf of a plain heapq Huffman tree), the two length vectors and the histograms."""
    img = np.asarray(img, np.uint8)
    rows, cols, _ = img.shape
    stream, types, sums = filter_image(img)
    deflate, segs = bytearray(), []
    for at in range(0, len(stream), SEG):
        seg = stream[at:at + SEG]
        key = (seg, at + SEG >= len(stream))
        if cache is None:
            data, info = encode_segment(*key)
        else:
            if key not in cache:
                cache[key] = encode_segment(*key)
            data, info = cache[key]
        deflate += data; segs.append(info)
    adler = zlib.adler32(stream)
    if len(stream) <= ADLER_BY_DEFINITION_MAX:       # Adler-32 by its definition, over the whole stream
        a = (1 + sum(stream)) % 65521
        b = (len(stream) + sum((len(stream) - p) * v for p, v in enumerate(stream))) % 65521
        assert adler == (b << 16) | a
    z = b"\x78\x01" + bytes(deflate) + adler.to_bytes(4, "big")
    return R.frame(cols, rows, z), {"types": types, "sums": sums, "segments": segs, "stream": stream}


# ---- what a file promises whatever the model says (read with png_decode_ref.inflate_trace) ----------------------------------------
def check_stream(data):
    """Asserts, from the file alone: the deflate stream is, per segment of SEG stream bytes, one dynamic or one stored block and then one
    empty stored block; every segment begins on a byte boundary; BFINAL is set on the last marker only; a dynamic block sends 286 + 4
    lengths with distance lengths 1 0 0 1 and all 19 code-length lengths, both codes are complete (Kraft sum exactly 1) within 15 and 7
    bits, and wherever a plain Huffman tree over the block's own symbol counts fits the limit, the code costs what that tree costs; a
    dynamic block with its marker is smaller than n + 10 bytes, a stored one is n + 10.
    -> per segment {n, stored, tokens, bytes}"""
    raw, blocks = R.inflate_trace(R.zlib_stream(data))
    assert len(blocks) % 2 == 0 and len(blocks) == 2 * ((len(raw) + SEG - 1) // SEG)
    segs, at = [], 0
    for k in range(0, len(blocks), 2):
        blk, mark = blocks[k], blocks[k + 1]
        n = min(SEG, len(raw) - at)
        last = k + 2 == len(blocks)
        assert blk["start_bit"] % 8 == 0 and blk["bfinal"] == 0 and blk["btype"] in (0, 2)
        assert (mark["btype"], mark["tokens"], mark["bfinal"]) == (0, [], 1 if last else 0)
        assert mark["start_bit"] == blk["end_bit"] and mark["end_bit"] % 8 == 0
        size = (mark["end_bit"] - blk["start_bit"]) // 8
        out = bytearray()
        for t in blk["tokens"]:
            if isinstance(t, int):
                out.append(t)
            else:
                assert t[1] in (1, 4) and 3 <= t[0] <= PIECE and t[1] <= len(out)      # no match reaches back before the segment
                R.copy_match(out, t[0], t[1])
        assert bytes(out) == raw[at:at + n]
        if blk["btype"] == 0:
            assert size == n + OVERHEAD
        else:
            assert size < n + OVERHEAD
            ll, cl = blk["litlen_lens"], blk["cl_lens"]
            assert len(ll) == N_LITLEN and tuple(blk["dist_lens"]) == DIST_LENS
            assert R.kraft(ll, 15) == 1 << 15 and max(ll) <= 15
            assert R.kraft(cl, 7) == 1 << 7 and max(cl) <= 7
            hist = histogram(blk["tokens"])
            assert all((h > 0) == (l > 0) for h, l in zip(hist, ll))
            depth, cost = plain_huffman(hist)
            if depth <= 15:
                assert sum(h * l for h, l in zip(hist, ll)) == cost
            cl_hist = [blk["cl_symbols"].count(s) for s in range(19)]
            depth, cost = plain_huffman(cl_hist)
            if depth <= 7 and sum(1 for h in cl_hist if h) >= 2:
                assert sum(h * l for h, l in zip(cl_hist, cl)) == cost
        segs.append({"n": n, "stored": blk["btype"] == 0, "tokens": blk["tokens"], "bytes": size})
        at += n
    assert at == len(raw)
    return segs


def check_against_model(data, info):
    """check_stream, then against the model's account: stored where the model stores (which is where its coded form, sized from its own
    parse and codes, would not be smaller than n + 10), the tokens the model's parse, a stored segment's bytes the segment"""
    segs = check_stream(data)
    assert len(segs) == len(info["segments"])
    for got, want in zip(segs, info["segments"]):
        assert got["n"] == want["n"] and got["stored"] == want["stored"] == (want["coded_bytes"] >= want["n"] + OVERHEAD)
        if got["stored"]:
            assert all(isinstance(t, int) for t in got["tokens"])
        else:
            assert got["tokens"] == want["tokens"] and got["bytes"] == want["coded_bytes"]
    return segs
