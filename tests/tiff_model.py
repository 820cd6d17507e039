"""A serial TIFF writer and decoder: the model the device TIFF decoder (csrc/kernels_tiff.hip) is held to, in the role png_model.py plays
for the PNG encoder.  The decoder follows tools/image_io.hpp read_tiff step for step (lzw_decode, packbits_decode, the predictor, the
RGB(A) -> BGRA swizzle) and reports per strip how many bytes decoded and why it stopped.  The writer controls what Pillow's does not:
byte order, strip placement down to the file offset mod 4, and for LZW the policy -- a Clear at the start or not, a Clear every N codes,
never a Clear (the table stays full), the EOI present, absent or followed by padding.

The closed form the kernel extracts codes by: code j after a Clear (j = 0 is the first; the strip's start counts as a Clear) is read while
the table holds min(4096, 258 + max(0, j - 1)) entries.  "Early change" steps the width up after the code that brings the table to 511,
1023 and 2047 entries, i.e. after j = 253, 765, 1789.  So
    width(j)  = 9 + [j >= 254] + [j >= 766] + [j >= 1790]
    offset(j) = 9 j + max(0, j - 254) + max(0, j - 766) + max(0, j - 1790)        (bits from the first bit after the Clear)
and a full table (j >= 3839) keeps reading 12-bit codes without adding entries."""
import struct

import numpy as np

CLEAR, EOI, TABLE = 256, 257, 4096
REASON_OK, REASON_BAD_CODE, REASON_BAD_TABLE_FULL, REASON_CUT_PACKET = 0, 1, 2, 3   # kTiffBadCode ... in csrc/pf_common.hpp


def lzw_width(j):
    return 9 + (j >= 254) + (j >= 766) + (j >= 1790)


def lzw_offset(j):
    return 9 * j + max(0, j - 254) + max(0, j - 766) + max(0, j - 1790)


# ---------------------------------------------------------------------------------------------------------------- LZW
def lzw_codes(data, clear_at_start=True, clear_every=None, never_clear=False):
    """the code sequence (without EOI) of `data`.  clear_every=N: a Clear after every N data codes; otherwise a Clear when the table
    reaches 4094 entries (libtiff's rule) unless never_clear, under which the table fills up and stays full"""
    codes = []
    table, nxt, since = {}, 258, 0
    if clear_at_start:
        codes.append(CLEAR)
    w = None
    for b in bytes(data):
        if w is None:
            w = b
            continue
        if (w, b) in table:
            w = table[(w, b)]
            continue
        codes.append(w)
        since += 1
        if nxt < TABLE:
            table[(w, b)] = nxt
            nxt += 1
        w = b
        if (clear_every and since >= clear_every) or (not clear_every and not never_clear and nxt > 4094):
            codes.append(CLEAR)
            table, nxt, since = {}, 258, 0
    if w is not None:
        codes.append(w)
    return codes


def lzw_pack(codes):
    """codes -> bytes, MSB first, each at the width its index since the last Clear gives it; the last byte is padded with zero bits"""
    acc, nacc, j, out = 0, 0, 0, bytearray()
    for c in codes:
        wd = lzw_width(j)
        acc = (acc << wd) | c
        nacc += wd
        j = 0 if c == CLEAR else j + 1
        while nacc >= 8:
            out.append((acc >> (nacc - 8)) & 0xff)
            nacc -= 8
        acc &= (1 << nacc) - 1
    if nacc:
        out.append((acc << (8 - nacc)) & 0xff)
    return bytes(out)


def lzw_encode(data, clear_at_start=True, clear_every=None, never_clear=False, eoi="present"):
    """eoi: 'present', 'absent', or 'padded' (EOI followed by four bytes of 0xA5)"""
    codes = lzw_codes(data, clear_at_start, clear_every, never_clear)
    if eoi != "absent":
        codes.append(EOI)
    return lzw_pack(codes) + (b"\xa5" * 4 if eoi == "padded" else b"")


def lzw_walk(src):
    """a serial walk of the code stream, as lzw_decode reads it but without a table: [(bit position, width, code, index since Clear)]
    up to and including the EOI or the last whole code"""
    pos, j, out = 0, 0, []
    src = bytes(src)
    while True:
        wd = 9 if j < 254 else 10 if j < 766 else 11 if j < 1790 else 12
        if pos + wd > 8 * len(src):
            return out
        v = int.from_bytes(src[pos // 8: pos // 8 + 3].ljust(3, b"\0"), "big")
        code = (v >> (24 - pos % 8 - wd)) & ((1 << wd) - 1)
        out.append((pos, wd, code, j))
        pos += wd
        if code == EOI:
            return out
        j = 0 if code == CLEAR else j + 1


def lzw_decode(src, expect):
    """tools/image_io.hpp lzw_decode: (bytes produced, clamped to expect; reason)"""
    src = bytes(src)
    prefix, suffix, first, length = [-1] * TABLE, [0] * TABLE, [0] * TABLE, [1] * TABLE
    for i in range(256):
        suffix[i] = first[i] = i
    nxt, bits, old, acc, nacc, pos, reason = 258, 9, -1, 0, 0, 0, REASON_OK
    out = bytearray()

    def emit(code):
        s = bytearray(length[code])
        c = code
        for i in range(length[code] - 1, -1, -1):
            s[i] = suffix[c]
            c = prefix[c]
        out.extend(s)

    while len(out) < expect:
        while nacc < bits and pos < len(src):
            acc = ((acc << 8) | src[pos]) & 0xffffffff
            pos += 1
            nacc += 8
        if nacc < bits:
            break
        code = (acc >> (nacc - bits)) & ((1 << bits) - 1)
        nacc -= bits
        if code == EOI:
            break
        if code == CLEAR:
            nxt, bits, old = 258, 9, -1
            continue
        if old < 0:
            if code >= 256:
                reason = REASON_BAD_CODE
                break
            emit(code)
            old = code
            continue
        if code > nxt or code >= TABLE:
            reason = REASON_BAD_CODE
            break
        if code < nxt:
            emit(code)
            if nxt < TABLE:
                prefix[nxt], suffix[nxt], first[nxt], length[nxt] = old, first[code], first[old], length[old] + 1
                nxt += 1
        else:
            if nxt >= TABLE:
                reason = REASON_BAD_TABLE_FULL
                break
            prefix[nxt], suffix[nxt], first[nxt], length[nxt] = old, first[old], first[old], length[old] + 1
            nxt += 1
            emit(nxt - 1)
        old = code
        if nxt + 1 >= (1 << bits) and bits < 12:
            bits += 1
    return bytes(out[:expect]), reason


# ---------------------------------------------------------------------------------------------------------------- PackBits
def packbits_encode(data, noop_every=0):
    """runs of two or more equal bytes become repeat packets (up to 128), the rest literal packets (up to 128); noop_every=N puts the
    no-op header byte -128 in front of every N-th packet"""
    data, out, i, k = bytes(data), bytearray(), 0, 0
    while i < len(data):
        run = 1
        while i + run < len(data) and run < 128 and data[i + run] == data[i]:
            run += 1
        if noop_every and k % noop_every == 0:
            out.append(0x80)
        k += 1
        if run >= 2:
            out += bytes([(1 - run) & 0xff, data[i]])
            i += run
            continue
        j = i + 1
        while j < len(data) and j - i < 128 and not (j + 1 < len(data) and data[j] == data[j + 1]):
            j += 1
        out += bytes([j - i - 1]) + data[i:j]
        i = j
    return bytes(out)


def packbits_decode(src, expect):
    """tools/image_io.hpp packbits_decode: (bytes produced, clamped to expect; reason)"""
    src, out, i, reason = bytes(src), bytearray(), 0, REASON_OK
    while i < len(src) and len(out) < expect:
        c = src[i] - 256 if src[i] >= 128 else src[i]
        i += 1
        if c >= 0:
            take = min(c + 1, len(src) - i)
            out += src[i:i + take]
            i += take
            if take < c + 1 and len(out) < expect:
                reason = REASON_CUT_PACKET
        elif c != -128:
            if i >= len(src):
                reason = REASON_CUT_PACKET
                break
            out += bytes([src[i]]) * (1 - c)
            i += 1
    return bytes(out[:expect]), reason


# ---------------------------------------------------------------------------------------------------------------- files
def expected_bgra(img):
    """(rows, cols, 3 | 4) RGB(A) samples -> what the decoders deliver: (rows, cols, 4) BGRA, alpha 255 for RGB"""
    img = np.asarray(img, np.uint8)
    out = np.empty(img.shape[:2] + (4,), np.uint8)
    out[..., 0], out[..., 1], out[..., 2] = img[..., 2], img[..., 1], img[..., 0]
    out[..., 3] = img[..., 3] if img.shape[2] == 4 else 255
    return out


def write_tiff(img, compression=1, big_endian=False, rows_per_strip=None, predictor=1, align=0, lzw=None, packbits=None, strip_bytes=None,
               extra_tags=()):
    """img: (rows, cols, 3 | 4) uint8 RGB(A).  align: every strip starts at a file offset = align mod 4.  lzw / packbits: keyword
    arguments of lzw_encode / packbits_encode.  strip_bytes: {strip index: bytes} replaces a strip's compressed bytes (malformed
    streams).  extra_tags: (tag, type, [values]) entries added to or replacing the IFD's."""
    img = np.ascontiguousarray(img, np.uint8)
    rows, cols, spp = img.shape
    rps = rows if rows_per_strip is None else min(rows_per_strip, rows)
    e = ">" if big_endian else "<"
    data = bytearray((b"MM" if big_endian else b"II") + struct.pack(e + "HI", 42, 0))
    offsets, counts = [], []
    for s, y0 in enumerate(range(0, rows, rps)):
        raw = img[y0:y0 + rps].astype(np.int16)
        if predictor == 2:
            raw[:, 1:] -= raw[:, :-1].copy()
        raw = (raw & 0xff).astype(np.uint8).tobytes()
        if strip_bytes and s in strip_bytes:
            blob = bytes(strip_bytes[s])
        elif compression == 1:
            blob = raw
        elif compression == 5:
            blob = lzw_encode(raw, **(lzw or {}))
        elif compression == 32773:
            blob = packbits_encode(raw, **(packbits or {}))
        else:
            raise ValueError("the model writes compression 1, 5 and 32773")
        while len(data) % 4 != align:
            data.append(0x5a)
        offsets.append(len(data))
        counts.append(len(blob))
        data += blob
    tags = {256: (4, [cols]), 257: (4, [rows]), 258: (3, [8] * spp), 259: (3, [compression]), 262: (3, [2]), 273: (4, offsets), 277: (3, [spp]),
            278: (4, [rps]), 279: (4, counts), 284: (3, [1])}
    if predictor != 1:
        tags[317] = (3, [predictor])
    if spp == 4:
        tags[338] = (3, [2])   # unassociated alpha
    for tag, typ, vals in extra_tags:
        tags[tag] = (typ, list(vals))
    entries = bytearray()
    for tag in sorted(tags):
        typ, vals = tags[tag]
        fmt = {1: "B", 3: "H", 4: "I"}[typ]
        packed = struct.pack(e + fmt * len(vals), *vals)
        if len(packed) > 4:
            while len(data) % 2:
                data.append(0)
            where = len(data)
            data += packed
            packed = struct.pack(e + "I", where)
        entries += struct.pack(e + "HHI", tag, typ, len(vals)) + packed.ljust(4, b"\0")
    while len(data) % 2:
        data.append(0)
    ifd = len(data)
    data += struct.pack(e + "H", len(tags)) + entries + struct.pack(e + "I", 0)
    data[4:8] = struct.pack(e + "I", ifd)
    return bytes(data)


def parse(data):
    """the fields read_tiff reads from the first IFD (a well-formed file is assumed)"""
    data = bytes(data)
    e = "<" if data[:2] == b"II" else ">"
    ifd, = struct.unpack_from(e + "I", data, 4)
    n, = struct.unpack_from(e + "H", data, ifd)
    f = {}
    for i in range(n):
        tag, typ, cnt = struct.unpack_from(e + "HHI", data, ifd + 2 + 12 * i)
        fmt, sz = {1: ("B", 1), 3: ("H", 2), 4: ("I", 4)}.get(typ, (None, 0))
        if fmt is None:
            continue
        at = ifd + 2 + 12 * i + 8
        if sz * cnt > 4:
            at, = struct.unpack_from(e + "I", data, at)
        f[tag] = list(struct.unpack_from(e + fmt * cnt, data, at))
    return f


def decode(data):
    """read_tiff on a file's bytes: (BGRA image with short strips zero-filled, [(bytes decoded, expected, reason)] per strip)"""
    data = bytes(data)
    f = parse(data)
    cols, rows, spp, comp = f[256][0], f[257][0], f[277][0], f.get(259, [1])[0]
    rps = min(f.get(278, [rows])[0], rows)
    pred = f.get(317, [1])[0]
    pix, status = bytearray(), []
    for s, (off, cnt) in enumerate(zip(f[273], f[279])):
        n = min(rps, rows - s * rps)
        expect = n * cols * spp
        src = data[off:off + cnt]
        if comp == 1:
            got, reason = src[:expect], REASON_OK
        elif comp == 5:
            got, reason = lzw_decode(src, expect)
        elif comp == 32773:
            got, reason = packbits_decode(src, expect)
        else:
            raise ValueError("the model decodes compression 1, 5 and 32773")
        status.append((len(got), expect, reason))
        strip = np.frombuffer(got.ljust(expect, b"\0"), np.uint8).reshape(n, cols, spp)
        if pred == 2:
            strip = np.cumsum(strip, axis=1, dtype=np.uint64).astype(np.uint8)
        pix += strip.tobytes()
    return expected_bgra(np.frombuffer(bytes(pix), np.uint8).reshape(rows, cols, spp)), status
