"""The device JPEG decoder's specification as a serial program: libjpeg's integer path, restated.  parse() accepts and
refuses what csrc/jpeg_parse.hpp does; decode() gives the pixels of Image.open(file).convert("RGB") for every file the contract accepts
(held to that by tests/test_jpegd_model.py), the coefficient plane (64 int16 per block in MCU order and zigzag order, the DC summed), the
component planes at their block-padded sizes, and a trace of the true decode: the raw bit at which every code word starts (stuffing
bytes counted, so the positions are the file's), how long it is, and the decoder's state there.  entry_states() turns the trace into what
the synchronisation kernels must arrive at for a subsequence size S.

A scan is accepted exactly when its true decode meets no event; `event` names the first one and the MCU at which decoding stopped.
The rules at a damaged stream are the device's, not libjpeg's (which warns and goes on): see `_scan`."""
import numpy as np

ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

MAX_SEGMENT = 1 << 28   # bytes of entropy-coded data the device's 32-bit bit positions hold


class Refused(Exception):
    """the header is outside the contract; str() names the reason"""


def _ceil(a, b):
    return -(-a // b)


def derive_table(bits, vals, is_dc):
    """jpeg_make_d_derived_tbl: -> (maxcode[18], valoff[17]) or Refused"""
    if sum(bits) > 256 or sum(bits) != len(vals):
        raise Refused("bad Huffman table")
    sizes = [l for l in range(1, 17) for _ in range(bits[l - 1])]
    codes, code, p = [], 0, 0
    si = sizes[0] if sizes else 0
    while p < len(sizes):
        while p < len(sizes) and sizes[p] == si:
            codes.append(code); code += 1; p += 1
        if code >= (1 << si):
            raise Refused("bad Huffman table")
        code <<= 1; si += 1
    maxcode = [-1] * 18; valoff = [0] * 17
    p = 0
    for l in range(1, 17):
        if bits[l - 1]:
            valoff[l] = p - codes[p]
            p += bits[l - 1]
            maxcode[l] = codes[p - 1]
    maxcode[17] = 0xFFFFF
    if is_dc and any(v > 15 for v in vals):
        raise Refused("bad Huffman table")
    return maxcode, valoff


def parse(data):
    """the markers up to the scan's first byte -> a dict, or Refused"""
    d = bytes(data); n = len(d)
    if n < 2 or d[0] != 0xFF or d[1] != 0xD8:
        raise Refused("not a JPEG")
    pos = 2
    qt = {}; huff = {}; frame = None; restart = 0; jfif = False; adobe = None
    while True:
        if pos >= n:
            raise Refused("truncated JPEG")
        if d[pos] != 0xFF:
            raise Refused("no marker where one is expected")
        while pos < n and d[pos] == 0xFF:
            pos += 1
        if pos >= n:
            raise Refused("truncated JPEG")
        m = d[pos]; pos += 1
        if m == 0xD9:
            raise Refused("no scan before EOI")
        if m == 0xD8 or m == 0x01 or m == 0x00 or 0xD0 <= m <= 0xD7:
            raise Refused("unexpected marker")
        if pos + 2 > n:
            raise Refused("truncated JPEG")
        L = (d[pos] << 8) | d[pos + 1]
        if L < 2 or pos + L > n:
            raise Refused("truncated JPEG")
        body = d[pos + 2:pos + L]; pos += L
        if m == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                if pq != 0:
                    raise Refused("16-bit quantisation table")
                if tq > 3 or k + 65 > len(body):
                    raise Refused("bad quantisation table")
                qt[tq] = np.frombuffer(body[k + 1:k + 65], np.uint8).astype(np.int32)
                k += 65
        elif m == 0xC4:
            k = 0
            while k < len(body):
                if k + 17 > len(body):
                    raise Refused("bad Huffman table")
                tc, th = body[k] >> 4, body[k] & 15
                bits = list(body[k + 1:k + 17]); cnt = sum(bits)
                if tc > 1 or th > 3 or cnt > 256 or k + 17 + cnt > len(body):
                    raise Refused("bad Huffman table")
                vals = list(body[k + 17:k + 17 + cnt])
                maxcode, valoff = derive_table(bits, vals, tc == 0)
                huff[(tc, th)] = dict(bits=bits, vals=vals, maxcode=maxcode, valoff=valoff)
                k += 17 + cnt
        elif m == 0xC0:
            if frame is not None:
                raise Refused("two frame headers")
            if len(body) < 6:
                raise Refused("bad frame header")
            prec = body[0]; rows = (body[1] << 8) | body[2]; cols = (body[3] << 8) | body[4]; nf = body[5]
            if prec != 8:
                raise Refused("%d-bit samples" % prec)
            if rows == 0:
                raise Refused("height 0 (DNL)")
            if cols == 0:
                raise Refused("width 0")
            if len(body) != 6 + 3 * nf:
                raise Refused("bad frame header")
            comps = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(nf)]
            if nf == 4:
                raise Refused("four components")
            if nf not in (1, 3):
                raise Refused("%d components" % nf)
            frame = dict(rows=rows, cols=cols, comps=comps)
        elif 0xC1 <= m <= 0xCF and m != 0xC4 and m != 0xCC:
            raise Refused("frame type SOF%d (only baseline SOF0 is decoded)" % (m - 0xC0))
        elif m == 0xCC:
            raise Refused("arithmetic coding")
        elif m == 0xDD:
            if len(body) != 2:
                raise Refused("bad DRI")
            restart = (body[0] << 8) | body[1]
        elif m == 0xDC:
            raise Refused("DNL")
        elif m == 0xE0:
            if len(body) >= 14 and body[:5] == b"JFIF\0":
                jfif = True
        elif m == 0xEE:
            if len(body) >= 12 and body[:5] == b"Adobe":
                adobe = body[11]
        elif m == 0xDA:
            if frame is None:
                raise Refused("scan before the frame header")
            comps = frame["comps"]
            if len(body) < 1 or len(body) != 4 + 2 * body[0]:
                raise Refused("bad scan header")
            ns = body[0]
            if ns != len(comps):
                raise Refused("several scans (the scan holds %d of %d components)" % (ns, len(comps)))
            tabs = []
            for i in range(ns):
                if body[1 + 2 * i] != comps[i][0]:
                    raise Refused("scan components out of frame order")
                td, ta = body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15
                if td > 3 or ta > 3 or (0, td) not in huff or (1, ta) not in huff:
                    raise Refused("the scan refers to a missing Huffman table")
                tabs.append((td, ta))
            if body[1 + 2 * ns] != 0 or body[2 + 2 * ns] != 63 or body[3 + 2 * ns] != 0:
                raise Refused("several scans (spectral selection or successive approximation)")
            break
        # every other segment (APPn, COM, ...) is skipped
    comps = frame["comps"]
    if len(comps) == 1:
        if comps[0][1] != 1 or comps[0][2] != 1:
            raise Refused("sampling %dx%d of a grey file" % (comps[0][1], comps[0][2]))
        hs = vs = 1
    else:
        hs, vs = comps[0][1], comps[0][2]
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any(c[1] != 1 or c[2] != 1 for c in comps[1:]):
            raise Refused("sampling " + ",".join("%dx%d" % (c[1], c[2]) for c in comps) + " (4:4:4, 4:2:2 and 4:2:0 are decoded)")
        ids = bytes(c[0] for c in comps)
        if not jfif and ((adobe is not None and adobe == 0) or (adobe is None and ids == b"RGB")):
            raise Refused("an RGB file (no YCbCr transform)")
    for c in comps:
        if c[3] > 3 or c[3] not in qt:
            raise Refused("the frame refers to a missing quantisation table")
    begin = pos
    # the entropy segment runs up to EOI; only stuffing and RSTn may stand in it
    end = None; k = begin
    while k < n:
        k = d.find(b"\xff", k)
        if k < 0 or k + 1 >= n:
            break
        nb = d[k + 1]
        if nb == 0 or 0xD0 <= nb <= 0xD7:
            k += 2; continue
        if nb == 0xD9:
            end = k; break
        if nb == 0xFF:
            raise Refused("fill bytes in the scan")
        if nb == 0xDC:
            raise Refused("DNL")
        raise Refused("several scans (marker 0x%02X after the scan)" % nb)
    if end is None:
        raise Refused("truncated JPEG: no EOI")
    if end - begin >= MAX_SEGMENT:
        raise Refused("scan too large")
    return dict(cols=frame["cols"], rows=frame["rows"], ncomp=len(comps), hs=hs, vs=vs, restart=restart, begin=begin, end=end,
                quant=[qt[c[3]] for c in comps], dc=[huff[(0, t[0])] for t in tabs], ac=[huff[(1, t[1])] for t in tabs])


def geometry(info):
    hs, vs = info["hs"], info["vs"]
    mcu_cols = _ceil(info["cols"], 8 * hs); mcu_rows = _ceil(info["rows"], 8 * vs)
    bpm = hs * vs + 2 if info["ncomp"] == 3 else 1
    return mcu_cols, mcu_rows, bpm


class _Event(Exception):
    def __init__(self, what, mcu):
        Exception.__init__(self, what); self.what = what; self.mcu = mcu


def _scan(d, info, trace):
    """The true decode of the entropy segment: (nblocks, 64) int32 coefficients in zigzag order, the DC still a difference.
    The segment is cut at its RSTn markers.  In every piece MCUs are decoded until a piece stands at an MCU boundary with fewer than 8
    bits left; then the piece must have held exactly its MCUs and be followed by its own RSTn (or, the last one, by EOI).  Events: an
    invalid code, a run past the block's end, bits running out inside an MCU, a block beyond the last, a wrong count or marker."""
    mcu_cols, mcu_rows, bpm = geometry(info)
    nmcu = mcu_cols * mcu_rows; restart = info["restart"]
    nint = _ceil(nmcu, restart) if restart else 1
    comp_of = [0] * (bpm - 2) + [1, 2] if info["ncomp"] == 3 else [0]
    coef = np.zeros((nmcu * bpm, 64), np.int32)
    seg = d[info["begin"]:info["end"]]
    # pieces between markers: (raw offset, raw length, marker byte or None)
    pieces = []; k = 0; start = 0
    while True:
        k = seg.find(b"\xff", k)
        if k < 0 or k + 1 >= len(seg):
            pieces.append((start, len(seg) - start, None)); break
        if seg[k + 1] == 0:
            k += 2; continue
        pieces.append((start, k - start, seg[k + 1])); k += 2; start = k
    starts = trace["starts"]; lens = trace["lens"]; states = trace["states"]
    B = 0          # blocks completed
    for pi, (off, ln, marker) in enumerate(pieces):
        raw = np.frombuffer(seg[off:off + ln], np.uint8)
        keep = np.ones(ln, bool)
        if ln > 1:
            keep[1:] = ~((raw[1:] == 0) & (raw[:-1] == 0xFF))
        rawidx = np.flatnonzero(keep) + off
        u = raw[keep].tobytes() + b"\0" * 8
        nbits = 8 * int(keep.sum()); bp = 0
        blk = 0
        while True:
            if blk == 0 and nbits - bp < 8:
                break
            for blk in range(blk, bpm):
                if B >= nmcu * bpm:
                    raise _Event("data beyond the last MCU", nmcu)
                c = comp_of[blk]; z = 0
                while True:
                    tab = info["dc"][c] if z == 0 else info["ac"][c]
                    w = int.from_bytes(u[bp >> 3:(bp >> 3) + 7], "big")
                    w = (w >> (56 - (bp & 7) - 32)) & 0xFFFFFFFF      # the next 32 bits
                    peek = w >> 16
                    mc = tab["maxcode"]
                    l = 1
                    while l <= 16 and (peek >> (16 - l)) > mc[l]:
                        l += 1
                    raw_bp = (int(rawidx[bp >> 3]) * 8 + (bp & 7)) if (bp >> 3) < len(rawidx) else (off + ln) * 8
                    if l > 16:
                        raise _Event("an invalid Huffman code", B // bpm)
                    sym = tab["vals"][((peek >> (16 - l)) + tab["valoff"][l]) & 255]
                    s = sym & 15; r = sym >> 4
                    if z == 0:
                        s = sym
                    total = l + s
                    if bp + total > nbits:
                        raise _Event("the bits run out inside an MCU", B // bpm)
                    starts.append(raw_bp); lens.append(total); states.append((blk, z, B, pi))
                    v = 0
                    if s:
                        v = (w >> (32 - l - s)) & ((1 << s) - 1)
                        if v < (1 << (s - 1)):
                            v = v - (1 << s) + 1
                    bp += total
                    if z == 0:
                        coef[B, 0] = v; z = 1
                    elif s:
                        if z + r > 63:
                            raise _Event("a run past the block's end", B // bpm)
                        z += r; coef[B, z] = v; z += 1
                    elif r == 15:
                        if z + 16 > 64:
                            raise _Event("a run past the block's end", B // bpm)
                        z += 16
                    else:
                        z = 64
                    if z >= 64:
                        break
                B += 1
            blk = 0
        c = B // bpm
        if marker is None:
            if pi != nint - 1 or c != nmcu:
                raise _Event("the scan ends after %d of %d MCUs" % (c, nmcu), c)
        else:
            if pi >= nint - 1 or c != (pi + 1) * restart or marker != 0xD0 + (pi & 7):
                raise _Event("a restart marker out of place", c)
        trace["piece_end_bits"].append((off + ln + (2 if marker is not None else 0)) * 8)
    return coef


def _idct_pass(c, shift):
    """one pass of jidctint over the last axis of c (..., 8), int32 with wrap-around"""
    c = c.astype(np.int32)
    z2 = c[..., 2]; z3 = c[..., 6]
    z1 = (z2 + z3) * np.int32(4433)
    t2 = z1 + z3 * np.int32(-15137); t3 = z1 + z2 * np.int32(6270)
    t0 = (c[..., 0] + c[..., 4]) << 13; t1 = (c[..., 0] - c[..., 4]) << 13
    t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2
    t0 = c[..., 7]; t1 = c[..., 5]; t2 = c[..., 3]; t3 = c[..., 1]
    z1 = t0 + t3; z2 = t1 + t2; z3 = t0 + t2; z4 = t1 + t3; z5 = (z3 + z4) * np.int32(9633)
    t0 = t0 * np.int32(2446); t1 = t1 * np.int32(16819); t2 = t2 * np.int32(25172); t3 = t3 * np.int32(12299)
    z1 = z1 * np.int32(-7373); z2 = z2 * np.int32(-20995); z3 = z3 * np.int32(-16069) + z5; z4 = z4 * np.int32(-3196) + z5
    t0 = t0 + z1 + z3; t1 = t1 + z2 + z4; t2 = t2 + z2 + z3; t3 = t3 + z1 + z4
    rnd = np.int32(1 << (shift - 1))
    out = np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], axis=-1)
    return (out + rnd) >> shift


def idct_blocks(coef_zz, quant_zz):
    """(n, 64) coefficients and a table, both in zigzag order -> (n, 8, 8) samples 0..255"""
    with np.errstate(over="ignore"):
        nat = np.zeros((coef_zz.shape[0], 64), np.int32)
        nat[:, ZIGZAG] = coef_zz.astype(np.int16).astype(np.int32) * quant_zz.astype(np.int32)
        blk = nat.reshape(-1, 8, 8)
        ws = _idct_pass(blk.transpose(0, 2, 1), 11).transpose(0, 2, 1)     # columns first
        px = _idct_pass(ws, 18)
        return np.clip(px + 128, 0, 255).astype(np.uint8)


def upsample_h2v1(p):
    """libjpeg's fancy h2v1 over the real samples p (rows, cw); cw <= 2: plain replication, as libjpeg chooses there"""
    p = p.astype(np.int32); cw = p.shape[1]
    if cw <= 2:
        return np.repeat(p, 2, axis=1)
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1); right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out = np.empty((p.shape[0], 2 * cw), np.int32)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    return out


def upsample_h2v2(p):
    p = p.astype(np.int32); ch, cw = p.shape
    if cw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    up = np.concatenate([p[:1], p[:-1]], axis=0); down = np.concatenate([p[1:], p[-1:]], axis=0)
    s = np.empty((2 * ch, cw), np.int32)
    s[0::2] = 3 * p + up; s[1::2] = 3 * p + down
    left = np.concatenate([s[:, :1], s[:, :-1]], axis=1); right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
    out = np.empty((2 * ch, 2 * cw), np.int32)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def colour(y, cb, cr):
    y = y.astype(np.int32); cb = cb.astype(np.int32) - 128; cr = cr.astype(np.int32) - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb - _fix(0.71414) * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def planes_from_coef(info, coef):
    """coefficient plane (DC summed) -> the component planes at their block-padded sizes"""
    mcu_cols, mcu_rows, bpm = geometry(info)
    hs, vs = info["hs"], info["vs"]
    c4 = coef.reshape(mcu_rows, mcu_cols, bpm, 64)
    out = []
    for ci in range(info["ncomp"]):
        if ci == 0:
            nb = hs * vs
            b = idct_blocks(c4[:, :, :nb].reshape(-1, 64), info["quant"][0]).reshape(mcu_rows, mcu_cols, vs, hs, 8, 8)
            out.append(b.transpose(0, 2, 4, 1, 3, 5).reshape(mcu_rows * vs * 8, mcu_cols * hs * 8))
        else:
            b = idct_blocks(c4[:, :, bpm - 3 + ci].reshape(-1, 64), info["quant"][ci]).reshape(mcu_rows, mcu_cols, 8, 8)
            out.append(b.transpose(0, 2, 1, 3).reshape(mcu_rows * 8, mcu_cols * 8))
    return out


def pixels_from_planes(info, planes):
    H, W = info["rows"], info["cols"]
    y = planes[0][:H, :W]
    if info["ncomp"] == 1:
        return np.repeat(y[..., None], 3, axis=2)
    hs, vs = info["hs"], info["vs"]
    cw, ch = _ceil(W, hs), _ceil(H, vs)
    ups = []
    for p in planes[1:]:
        p = p[:ch, :cw]
        if hs == 2 and vs == 2:
            p = upsample_h2v2(p)
        elif hs == 2:
            p = upsample_h2v1(p)
        ups.append(p[:H, :W])
    return colour(y, ups[0], ups[1])


def sum_dc(info, coef):
    """DC differences -> values: per component, restarting at every interval; int16 wrap-around as the device stores them"""
    mcu_cols, mcu_rows, bpm = geometry(info)
    nmcu = mcu_cols * mcu_rows; restart = info["restart"] or nmcu
    out = coef.copy()
    comp_of = np.array([0] * (bpm - 2) + [1, 2] if info["ncomp"] == 3 else [0])
    dc = coef[:, 0].reshape(nmcu, bpm).astype(np.int64)
    for ci in range(info["ncomp"]):
        sel = np.flatnonzero(comp_of == ci)
        v = dc[:, sel]
        for m0 in range(0, nmcu, restart):
            part = v[m0:m0 + restart]
            v[m0:m0 + restart] = np.cumsum(part.reshape(-1)).reshape(part.shape)
        dc[:, sel] = v
    out[:, 0] = dc.reshape(-1).astype(np.int16)
    return out


def decode(data, want_planes=True):
    """-> dict: info, accept, event / event_mcu, rgb (rows, cols, 3), coef (nblocks, 64) int16, planes, trace.  Raises Refused for a
    header outside the contract; a refused scan returns accept False and no pixels"""
    d = bytes(data)
    info = parse(d)
    trace = dict(starts=[], lens=[], states=[], piece_end_bits=[])
    out = dict(info=info, trace=trace, accept=True, event=None, event_mcu=None)
    try:
        coef = _scan(d, info, trace)
    except _Event as e:
        out.update(accept=False, event=e.what, event_mcu=e.mcu)
        return out
    coef = sum_dc(info, coef).astype(np.int16)
    out["coef"] = coef
    planes = planes_from_coef(info, coef)
    out["planes"] = planes
    out["rgb"] = pixels_from_planes(info, planes)
    return out


def bgra(rgb):
    out = np.empty(rgb.shape[:2] + (4,), np.uint8)
    out[..., 0] = rgb[..., 2]; out[..., 1] = rgb[..., 1]; out[..., 2] = rgb[..., 0]; out[..., 3] = 255
    return out


def n_subsequences(info, S):
    return max(1, _ceil(info["end"] - info["begin"], S))


def entry_states(result, S):
    """what the synchronisation must arrive at: for subsequence i >= 1 the state at the first code word that starts at or beyond bit
    i * S * 8 -> (n - 1, 3) array of (bit, block in MCU, zigzag index); subsequence 0 enters at (0, 0, 0).  A state past the last
    code word is the segment's end (bit = 8 * bytes, block 0, index 0)."""
    info = result["info"]; tr = result["trace"]
    _, _, bpm = geometry(info)
    n = n_subsequences(info, S)
    starts = np.array(tr["starts"], np.int64)
    seg_bits = 8 * (info["end"] - info["begin"])
    out = np.zeros((n - 1, 3), np.int64)
    for i in range(1, n):
        k = int(np.searchsorted(starts, i * S * 8, "left"))
        if k >= len(starts):
            out[i - 1] = (seg_bits, 0, 0)
        else:
            blk, z, _, _ = tr["states"][k]
            out[i - 1] = (starts[k], blk, z)
    return out
