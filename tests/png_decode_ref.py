"""A strict PNG reader for the device encoder's tests: stdlib zlib + numpy only.

decode(data) -> (rows, cols, 4) uint8 BGRA.  It accepts exactly what the encoder promises (8-bit RGBA, no interlace) and raises
PngError on anything else: a wrong signature, a chunk CRC that zlib.crc32 does not confirm, IHDR fields other than (8, 6, 0, 0, 0),
a zlib stream that zlib refuses (which covers the Adler-32), does not end or has bytes behind it, a filter type above 4, bytes after IEND.

inflate_trace(z) is an inflate of its own that reports every block: its header, its code lengths, its tokens.
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


class PngError(ValueError):
    pass


def chunks(data):
    """[(type, payload)] of every chunk, CRCs checked; the file must end with IEND"""
    if data[:8] != SIGNATURE:
        raise PngError("bad signature")
    out, pos = [], 8
    while pos < len(data):
        if pos + 12 > len(data):
            raise PngError("truncated chunk header")
        (length,) = struct.unpack(">I", data[pos:pos + 4])
        ctype = data[pos + 4:pos + 8]
        if length > 0x7fffffff or pos + 12 + length > len(data):
            raise PngError("truncated chunk %r" % ctype)
        payload = data[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        if zlib.crc32(ctype + payload) & 0xffffffff != crc:
            raise PngError("bad CRC in chunk %r" % ctype)
        out.append((ctype, payload))
        pos += 12 + length
        if ctype == b"IEND":
            break
    if not out or out[-1][0] != b"IEND" or out[-1][1] != b"":
        raise PngError("no IEND")
    if pos != len(data):
        raise PngError("bytes after IEND")
    return out


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def unfilter(raw, cols, rows):
    """filtered scanlines (rows x (1 + 4 cols) bytes) -> (rows, cols, 4) uint8 RGBA; also returns the filter types"""
    stride = 4 * cols
    if len(raw) != rows * (stride + 1):
        raise PngError("scanline data is %d bytes, expected %d" % (len(raw), rows * (stride + 1)))
    lines = np.frombuffer(raw, np.uint8).reshape(rows, stride + 1)
    types = lines[:, 0].copy()
    if types.max() > 4:
        raise PngError("filter type %d" % types.max())
    res = lines[:, 1:].astype(np.int32).reshape(rows, cols, 4)
    # A pixel needs its left, upper and upper-left neighbours, which lie on the two anti-diagonals before its own: one vectorised step per
    # anti-diagonal, every row with its own filter type.  `out` carries a zero row above and a zero column to the left.
    out = np.zeros((rows + 1, cols + 1, 4), np.int32)
    for d in range(rows + cols - 1):
        ys = np.arange(max(0, d - cols + 1), min(rows - 1, d) + 1)
        xs = d - ys
        a, b, c = out[ys + 1, xs], out[ys, xs + 1], out[ys, xs]
        f = types[ys][:, None]
        pred = np.where(f == 0, 0, np.where(f == 1, a, np.where(f == 2, b, np.where(f == 3, (a + b) >> 1, _paeth(a, b, c)))))
        out[ys + 1, xs + 1] = (res[ys, xs] + pred) & 255
    return out[1:, 1:].astype(np.uint8), types


def inflate(z):
    """the whole zlib stream and nothing but it: zlib checks the Adler-32; a stream that does not end, or bytes after its end, are refused
    here (zlib.decompress alone lets trailing bytes pass)"""
    d = zlib.decompressobj()
    try:
        raw = d.decompress(z) + d.flush()
    except zlib.error as e:
        raise PngError("zlib: %s" % e)
    if not d.eof:
        raise PngError("zlib stream does not end")
    if d.unused_data:
        raise PngError("%d bytes after the zlib stream" % len(d.unused_data))
    return raw


# ---- a block-level inflate (RFC 1951), for streams of a few segments: slow, and strict ----
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def kraft(lens, maxbits=15):
    """the Kraft sum of a code, in units of 2 ** -maxbits: a complete code gives exactly 2 ** maxbits"""
    return sum(1 << (maxbits - l) for l in lens if l)


def _decoder(lens, what, may_be_lone=False):
    """{(length, code): symbol} of the canonical code with these lengths.  An over-subscribed code is refused, and so is an incomplete one,
    but for what RFC 1951 3.2.7 allows the distance code: one code of one bit, or none at all (a block of literals only)."""
    if max(lens, default=0) > 15:
        raise PngError("%s code: a length above 15" % what)
    k, used = kraft(lens), [l for l in lens if l]
    if k > 1 << 15:
        raise PngError("%s code is over-subscribed" % what)
    if k < 1 << 15 and not (may_be_lone and (used == [] or used == [1])):
        raise PngError("%s code is incomplete" % what)
    count = [0] * 17
    for l in used:
        count[l] += 1
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    table = {}
    for s, l in enumerate(lens):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def copy_match(out, length, dist):
    """append `length` bytes from `dist` back, a byte at a time in effect: the bytes a match appends may be ones it has just appended"""
    tail = bytes(out[-dist:])
    out += (tail * (length // dist + 1))[:length]


class _BitReader:
    def __init__(self, data):
        self.d = data; self.pos = 0

    def bits(self, n):
        v = 0
        for i in range(n):
            if self.pos >> 3 >= len(self.d):
                raise PngError("the deflate stream ends inside a block")
            v |= ((self.d[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v

    def symbol(self, table, what):
        code = 0
        for l in range(1, 16):
            code = code << 1 | self.bits(1)
            s = table.get((l, code))
            if s is not None:
                return s
        raise PngError("no %s code matches" % what)


def inflate_trace(z):
    """a zlib stream -> (the bytes, blocks).  Per block a dict: bfinal, btype, start_bit / end_bit (offsets into the deflate data, which
    begins behind the two header bytes), tokens (an int is a literal, (length, distance) a match; a stored block's bytes count as
    literals) and, for a dynamic block, cl_lens (19), litlen_lens (HLIT + 257), dist_lens (HDIST + 1) and cl_symbols (the code-length
    symbols as read); for a stored block data_byte,
    the offset of its first data byte.  Raises PngError on what RFC 1950 / 1951 forbid: a bad header or Adler-32, block type 3,
    LEN != ~NLEN, a code that is over-subscribed or incomplete, a repeat with nothing before it or past the end of the lengths, no code
    for the end of the block, length symbols 286 / 287, distance symbols 30 / 31, a distance beyond the output, a stream that ends
    early, bytes behind it."""
    z = bytes(z)
    if len(z) < 6 or z[0] & 15 != 8 or z[0] >> 4 > 7 or (z[0] << 8 | z[1]) % 31 or z[1] & 32:
        raise PngError("bad zlib header")
    r = _BitReader(z[2:-4])
    out, blocks = bytearray(), []
    while True:
        blk = {"start_bit": r.pos, "bfinal": r.bits(1), "btype": r.bits(2), "tokens": []}
        toks = blk["tokens"]
        if blk["btype"] == 3:
            raise PngError("block type 3")
        if blk["btype"] == 0:
            r.pos = (r.pos + 7) & ~7
            n, nn = r.bits(16), r.bits(16)
            if n != nn ^ 0xffff:
                raise PngError("LEN != ~NLEN")
            at = r.pos >> 3
            if at + n > len(r.d):
                raise PngError("the deflate stream ends inside a stored block")
            blk["data_byte"] = at
            toks.extend(r.d[at:at + n]); out += r.d[at:at + n]
            r.pos += 8 * n
        else:
            if blk["btype"] == 1:
                ll = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8; dl = [5] * 32
            else:
                hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
                if hlit > 286 or hdist > 30:
                    raise PngError("HLIT / HDIST out of range")
                cl = [0] * 19
                for i in range(hclen):
                    cl[_CL_ORDER[i]] = r.bits(3)
                cl_table = _decoder(cl, "code-length")
                lens, blk["cl_symbols"] = [], []
                while len(lens) < hlit + hdist:
                    s = r.symbol(cl_table, "code-length")
                    blk["cl_symbols"].append(s)
                    if s < 16:
                        lens.append(s); continue
                    if s == 16:
                        if not lens:
                            raise PngError("repeat with no length before it")
                        v, k = lens[-1], 3 + r.bits(2)
                    else:
                        v, k = 0, (3 + r.bits(3)) if s == 17 else (11 + r.bits(7))
                    if len(lens) + k > hlit + hdist:
                        raise PngError("repeat past the end of the code lengths")
                    lens += [v] * k
                ll, dl = lens[:hlit], lens[hlit:]
                blk["cl_lens"], blk["litlen_lens"], blk["dist_lens"] = cl, ll, dl
                if not ll[256]:
                    raise PngError("no code for the end of the block")
            lt, dt = _decoder(ll, "literal / length"), _decoder(dl, "distance", may_be_lone=True)
            while True:
                s = r.symbol(lt, "literal / length")
                if s < 256:
                    toks.append(s); out.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise PngError("length symbol %d" % s)
                    length = _LEN_BASE[s - 257] + r.bits(_LEN_EXTRA[s - 257])
                    ds = r.symbol(dt, "distance")
                    if ds > 29:
                        raise PngError("distance symbol %d" % ds)
                    dist = _DIST_BASE[ds] + r.bits(_DIST_EXTRA[ds])
                    if dist > len(out):
                        raise PngError("distance %d beyond the output (%d bytes)" % (dist, len(out)))
                    toks.append((length, dist))
                    copy_match(out, length, dist)
        blk["end_bit"] = r.pos
        blocks.append(blk)
        if blk["bfinal"]:
            break
    if (r.pos + 7) >> 3 != len(r.d):
        raise PngError("%d bytes behind the last block" % (len(r.d) - ((r.pos + 7) >> 3)))
    if zlib.adler32(bytes(out)) != int.from_bytes(z[-4:], "big"):
        raise PngError("wrong Adler-32")
    return bytes(out), blocks


def zlib_stream(data):
    """the zlib stream of a file: its IDAT payloads joined"""
    return b"".join(p for t, p in chunks(bytes(data)) if t == b"IDAT")


def decode(data, want_types=False):
    cks = chunks(bytes(data))
    if cks[0][0] != b"IHDR" or len(cks[0][1]) != 13:
        raise PngError("first chunk is not a 13-byte IHDR")
    cols, rows, depth, ctype, comp, filt, inter = struct.unpack(">IIBBBBB", cks[0][1])
    if (depth, ctype, comp, filt, inter) != (8, 6, 0, 0, 0) or cols == 0 or rows == 0:
        raise PngError("IHDR fields %r" % ((cols, rows, depth, ctype, comp, filt, inter),))
    names = [c[0] for c in cks]
    idat = [i for i, nm in enumerate(names) if nm == b"IDAT"]
    if not idat or idat != list(range(idat[0], idat[-1] + 1)):
        raise PngError("IDAT chunks missing or not consecutive")
    if any(nm not in (b"IHDR", b"IDAT", b"IEND") for nm in names):
        raise PngError("unexpected chunk")
    raw = inflate(b"".join(c[1] for c in cks if c[0] == b"IDAT"))
    rgba, types = unfilter(raw, cols, rows)
    bgra = np.ascontiguousarray(rgba[:, :, [2, 1, 0, 3]])
    return (bgra, types) if want_types else bgra


def filtered_stream(data):
    """the filtered scanlines of a file (for size checks)"""
    return inflate(b"".join(p for t, p in chunks(bytes(data)) if t == b"IDAT"))


def frame(cols, rows, zdata, idat_max=None):
    """a PNG around a finished zlib stream (the tests' own writer, for hand-built files and the parent writer's size)"""
    def chunk(t, p):
        return struct.pack(">I", len(p)) + t + p + struct.pack(">I", zlib.crc32(t + p) & 0xffffffff)
    idat_max = idat_max or len(zdata) or 1
    body = b"".join(chunk(b"IDAT", zdata[i:i + idat_max]) for i in range(0, max(len(zdata), 1), idat_max))
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, 8, 6, 0, 0, 0)) + body + chunk(b"IEND", b"")


def filter_rows(bgra, types):
    """filtered scanlines of a BGRA image with the given filter type per row (the tests' own, slow, forward filter)"""
    rgba = np.asarray(bgra, np.uint8)[:, :, [2, 1, 0, 3]].astype(np.int32)
    rows, cols, _ = rgba.shape
    out = bytearray()
    zero = np.zeros((cols, 4), np.int32)
    for y in range(rows):
        f = int(types[y]); cur = rgba[y]; up = rgba[y - 1] if y else zero
        left = np.vstack([np.zeros((1, 4), np.int32), cur[:-1]])
        upleft = np.vstack([np.zeros((1, 4), np.int32), up[:-1]])
        pred = [0 * cur, left, up, (left + up) >> 1, _paeth(left, up, upleft)][f]
        out.append(f)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)
