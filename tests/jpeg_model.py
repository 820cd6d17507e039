"""The device JPEG encoder's specification as a serial numpy program: libjpeg's integer path, restated.  encode() gives
the whole file, byte for byte what libjpeg(-turbo) writes for the same image, quality, subsampling and restart interval (held to that by
tests/test_jpeg_model.py), and a trace of the symbols it sent, which the branch cases (tests/jpeg_cases.py) are checked against.
Per restart interval the trace also gives the coder's geometry before stuffing: the bit count, the padded bytes, the byte offsets of
every 0xFF, and where each code word starts and how long it is (a code word as the device coder sends it: a Huffman code and the
value's bits as one word of up to 26 bits).
Input is packed BGRA (rows, cols, 4) uint8; alpha is dropped and the colour bytes are encoded as stored."""
import numpy as np

# ---- Annex K ----
QBASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
QBASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa]

# the product's restart intervals in MCUs (pf_jpeg_restart_interval), by subsampling: 0 = 4:4:4, 1 = 4:2:0
RESTART = {0: 64, 1: 32}

XMP_ID = b"http://ns.adobe.com/xap/1.0/\0"


def quant_table(base, quality):
    """jpeg_set_quality's scaling (baseline: entries clamped to 1..255), in natural order"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * scale + 50) // 100, 1, 255)


def huff_codes(bits, vals):
    """symbol -> (code, length), the canonical assignment of a DHT"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1; k += 1
        code <<= 1
    return out


def _fix(x):
    return int(x * 65536 + 0.5)


def colour_planes(img):
    b = img[..., 0].astype(np.int64); g = img[..., 1].astype(np.int64); r = img[..., 2].astype(np.int64)
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(p, rows, cols):
    """replicate the last column, then the last row"""
    p = np.concatenate([p, np.repeat(p[:, -1:], cols - p.shape[1], axis=1)], axis=1) if cols > p.shape[1] else p
    return np.concatenate([p, np.repeat(p[-1:], rows - p.shape[0], axis=0)], axis=0) if rows > p.shape[0] else p


def _ceil(a, b):
    return -(-a // b)


def downsample420(p):
    """full-resolution chroma plane -> the padded downsampled plane, in the order DESIGN.md 8.4 gives"""
    h, w = p.shape
    cw = 8 * _ceil(_ceil(w, 2), 8)
    p = _pad(p, h + (h & 1), 2 * cw)
    bias = np.where(np.arange(cw) % 2 == 0, 1, 2)
    d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    return _pad(d, 8 * _ceil(d.shape[0], 8), cw)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(d, first):
    """one pass of jfdctint over the last axis of d (..., 8)"""
    t0 = d[..., 0] + d[..., 7]; t7 = d[..., 0] - d[..., 7]; t1 = d[..., 1] + d[..., 6]; t6 = d[..., 1] - d[..., 6]
    t2 = d[..., 2] + d[..., 5]; t5 = d[..., 2] - d[..., 5]; t3 = d[..., 3] + d[..., 4]; t4 = d[..., 3] - d[..., 4]
    t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2
    n = 11 if first else 15
    out = np.empty_like(d)
    out[..., 0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    out[..., 4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[..., 2] = _descale(z1 + t13 * 6270, n)
    out[..., 6] = _descale(z1 - t12 * 15137, n)
    z1 = t4 + t7; z2 = t5 + t6; z3 = t4 + t6; z4 = t5 + t7; z5 = (z3 + z4) * 9633
    t4 = t4 * 2446; t5 = t5 * 16819; t6 = t6 * 25172; t7 = t7 * 12299
    z1 = z1 * -7373; z2 = z2 * -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5
    out[..., 7] = _descale(t4 + z1 + z3, n)
    out[..., 5] = _descale(t5 + z2 + z4, n)
    out[..., 3] = _descale(t6 + z2 + z3, n)
    out[..., 1] = _descale(t7 + z1 + z4, n)
    return out


def fdct_quant(plane, q, ties=None):
    """padded sample plane -> (block rows, block cols, 64) quantised coefficients in zigzag order"""
    h, w = plane.shape
    blk = (plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3) - 128).astype(np.int64)
    c = _pass(blk, True)
    c = _pass(c.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2).reshape(h // 8, w // 8, 64)
    qv = 8 * q
    a = np.abs(c)
    if ties is not None:
        ties.append(int(((c < 0) & ((a + (qv >> 1)) % qv == 0) & (qv % 2 == 0)).sum()))
    v = (a + (qv >> 1)) // qv
    return (np.where(c < 0, -v, v))[..., ZIGZAG]


def mcu_blocks(img, quality, subsampling, info=None):
    """(n MCUs, blocks per MCU, 64) coefficients in MCU order, dummy blocks included, and the MCU grid"""
    h, w = img.shape[:2]
    y, cb, cr = colour_planes(img)
    ql = quant_table(QBASE_LUMA, quality); qc = quant_table(QBASE_CHROMA, quality)
    ties = []
    if subsampling == 0:
        mr, mc = _ceil(h, 8), _ceil(w, 8)
        planes = [fdct_quant(_pad(p, 8 * mr, 8 * mc), q, ties) for p, q in ((y, ql), (cb, qc), (cr, qc))]
        out = np.stack(planes, axis=2).reshape(mr * mc, 3, 64)
    else:
        mr, mc = _ceil(h, 16), _ceil(w, 16)
        br, bc = _ceil(h, 8), _ceil(w, 8)
        yc = fdct_quant(_pad(y, 8 * br, 8 * bc), ql, ties)
        full = np.zeros((2 * mr, 2 * mc, 64), np.int64)
        full[:br, :bc] = yc
        cbc = fdct_quant(downsample420(cb), qc, ties); crc = fdct_quant(downsample420(cr), qc, ties)
        assert cbc.shape[:2] == (mr, mc), (cbc.shape, mr, mc)
        out = np.zeros((mr, mc, 6, 64), np.int64)
        for j in range(4):
            out[:, :, j] = full[j // 2::2, j % 2::2]
        # dummy luma blocks: all AC zero, DC of the block that precedes them in MCU order
        if bc & 1:
            out[:, -1, 1, 0] = out[:, -1, 0, 0]
            out[:, -1, 3, 0] = out[:, -1, 2, 0]
        if br & 1:
            out[-1, :, 2, 0] = out[-1, :, 1, 0]
            out[-1, :, 3, 0] = out[-1, :, 1, 0]
        out[:, :, 4] = cbc; out[:, :, 5] = crc
        out = out.reshape(mr * mc, 6, 64)
        if info is not None:
            info["dummy_right"] = bool(bc & 1); info["dummy_bottom"] = bool(br & 1)
    if info is not None:
        info["negative_ties"] = sum(ties); info["mcu_rows"] = mr; info["mcu_cols"] = mc
    return out, mr, mc


def _category(v):
    return int(abs(v)).bit_length()


class _Bits:
    def __init__(self):
        self.acc = 0; self.n = 0

    def put(self, code, length):
        self.acc = (self.acc << length) | code; self.n += length

    def flush(self):
        """pad with 1-bits to a byte; -> the unstuffed bytes"""
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        return self.acc.to_bytes(self.n // 8, "big"), pad


def entropy(blocks, subsampling, restart, info=None):
    """the entropy-coded segment: intervals of `restart` MCUs, stuffed, RSTn between them"""
    dc_tab = [huff_codes(DC_LUMA_BITS, DC_VALS), huff_codes(DC_CHROMA_BITS, DC_VALS)]
    ac_tab = [huff_codes(AC_LUMA_BITS, AC_LUMA_VALS), huff_codes(AC_CHROMA_BITS, AC_CHROMA_VALS)]
    n, bpm, _ = blocks.shape
    comp = [0, 1, 2] if bpm == 3 else [0, 0, 0, 0, 1, 2]
    out = bytearray()
    tr = dict(zrl=0, zrl_pairs=0, no_eob=0, all_zero=0, max_dc_cat=0, max_ac_cat=0, ff_inside=0, ff_last=0, exact_byte=0, max_block_bits=0,
              intervals=0, interval_bytes=[], interval_bits=[], interval_raw=[], ff_offsets=[], word_starts=[], word_lens=[])
    nint = _ceil(n, restart)
    for i in range(nint):
        bits = _Bits(); pred = [0, 0, 0]
        starts = []          # the bit at which every code word starts, and (a sentinel) the interval's bit count
        for m in range(i * restart, min(n, (i + 1) * restart)):
            for j in range(bpm):
                c = blocks[m, j]; k = comp[j]; t = min(k, 1); start = bits.n
                d = int(c[0]) - pred[k]; pred[k] = int(c[0])
                s = _category(d)
                starts.append(bits.n)
                bits.put(*dc_tab[t][s])
                if s:
                    bits.put((d if d >= 0 else d - 1) & ((1 << s) - 1), s)
                tr["max_dc_cat"] = max(tr["max_dc_cat"], s)
                run = 0; nz = np.flatnonzero(c[1:]) + 1
                last = 0
                for z in nz:
                    v = int(c[z]); run = z - last - 1; last = z
                    nzrl = run // 16
                    for _ in range(nzrl):
                        starts.append(bits.n)
                        bits.put(*ac_tab[t][0xF0])
                    tr["zrl"] += nzrl; tr["zrl_pairs"] += nzrl >= 2
                    s = _category(v)
                    starts.append(bits.n)
                    bits.put(*ac_tab[t][((run & 15) << 4) | s])
                    bits.put((v if v >= 0 else v - 1) & ((1 << s) - 1), s)
                    tr["max_ac_cat"] = max(tr["max_ac_cat"], s)
                if last != 63:
                    starts.append(bits.n)
                    bits.put(*ac_tab[t][0])
                else:
                    tr["no_eob"] += 1
                tr["all_zero"] += (d == 0 and len(nz) == 0)
                tr["max_block_bits"] = max(tr["max_block_bits"], bits.n - start)
        starts.append(bits.n)
        tr["interval_bits"].append(bits.n)
        tr["word_starts"].append(np.array(starts[:-1], np.int64)); tr["word_lens"].append(np.diff(np.array(starts, np.int64)))
        raw, pad = bits.flush()
        tr["interval_raw"].append(raw)
        tr["ff_offsets"].append(np.flatnonzero(np.frombuffer(raw, np.uint8) == 0xFF))
        tr["exact_byte"] += pad == 0
        tr["ff_inside"] += raw[:-1].count(0xFF)
        tr["ff_last"] += raw[-1:] == b"\xff"
        seg = raw.replace(b"\xff", b"\xff\x00")
        if i + 1 < nint:
            seg += bytes([0xFF, 0xD0 + (i & 7)])
        tr["interval_bytes"].append(len(seg))
        out += seg
    tr["intervals"] = nint
    if info is not None:
        info.update(tr)
    return bytes(out)


def _seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body


def xmp_packet(cols, rows):
    return ('<x:xmpmeta xmlns:x="adobe:ns:meta/"><rdf:RDF xmlns:rdf="http://www.w3.org/1999/02/22-rdf-syntax-ns#">'
            '<rdf:Description rdf:about="" xmlns:GPano="http://ns.google.com/photos/1.0/panorama/" '
            'GPano:ProjectionType="equirectangular" GPano:UsePanoramaViewer="True" '
            'GPano:FullPanoWidthPixels="%d" GPano:FullPanoHeightPixels="%d" '
            'GPano:CroppedAreaImageWidthPixels="%d" GPano:CroppedAreaImageHeightPixels="%d" '
            'GPano:CroppedAreaLeftPixels="0" GPano:CroppedAreaTopPixels="0"/></rdf:RDF></x:xmpmeta>' % (cols, rows, cols, rows)).encode()


def header(cols, rows, quality, subsampling, restart, gpano=0):
    ql = quant_table(QBASE_LUMA, quality)[ZIGZAG]; qc = quant_table(QBASE_CHROMA, quality)[ZIGZAG]
    h = b"\xff\xd8" + _seg(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if gpano:
        h += _seg(0xE1, XMP_ID + xmp_packet(cols, rows))
    h += _seg(0xDB, b"\x00" + bytes(int(v) for v in ql)) + _seg(0xDB, b"\x01" + bytes(int(v) for v in qc))
    h += _seg(0xC0, b"\x08" + rows.to_bytes(2, "big") + cols.to_bytes(2, "big") + b"\x03\x01" + (b"\x22" if subsampling else b"\x11") + b"\x00\x02\x11\x01\x03\x11\x01")
    for tc, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS), (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        h += _seg(0xC4, bytes([tc]) + bytes(bits) + bytes(vals))
    h += _seg(0xDD, restart.to_bytes(2, "big"))
    h += _seg(0xDA, b"\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00")
    return h


def encode(img, quality=90, subsampling=1, restart=None, gpano=0, want_info=False):
    """the file; restart = MCUs per interval (default: the product's RESTART[subsampling]); want_info: (file, trace)"""
    img = np.asarray(img, np.uint8)
    rows, cols = img.shape[:2]
    restart = RESTART[subsampling] if restart is None else restart
    info = {}
    blocks, _, _ = mcu_blocks(img, quality, subsampling, info)
    data = header(cols, rows, quality, subsampling, restart, gpano) + entropy(blocks, subsampling, restart, info) + b"\xff\xd9"
    return (data, info) if want_info else data
