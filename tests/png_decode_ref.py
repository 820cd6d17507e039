"""A strict PNG reader for the device encoder's tests: stdlib zlib + numpy only.

decode(data) -> (rows, cols, 4) uint8 BGRA.  It accepts exactly what the encoder promises (8-bit RGBA, no interlace) and raises
PngError on anything else: a wrong signature, a chunk CRC that zlib.crc32 does not confirm, IHDR fields other than (8, 6, 0, 0, 0),
a zlib stream that zlib refuses (which covers the Adler-32), does not end or has bytes behind it, a filter type above 4, bytes after IEND.
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
