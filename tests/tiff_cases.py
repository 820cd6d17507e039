"""The files the device TIFF decoder is tested on, shared by the host-run kernels (test_tiff_kernels_host.py) and the GPU tier
(test_gpu_tiff.py): name -> Case(file bytes, the RGB(A) image it was made from, whether libtiff must read it).  Shapes are the smallest
at which each mechanism can go wrong.  malformed(): streams the kernels must refuse; only `early_eoi` goes to the GPU."""
import collections
import io

import numpy as np

import tiff_model as tm

Case = collections.namedtuple("Case", "file img pillow")


def noise(rows, cols, spp, seed):
    return np.random.RandomState(seed).randint(0, 256, (rows, cols, spp)).astype(np.uint8)


def smooth(rows, cols, spp, seed=0):
    y, x, c = np.meshgrid(np.arange(rows), np.arange(cols), np.arange(spp), indexing="ij")
    return ((3 * y + 2 * x + 50 * c + seed + ((x * 7 + y * 3) % 5)) & 0xff).astype(np.uint8)


def pillow_tiff(img, compression, rows_per_strip=None, predictor=None):
    from PIL import Image
    info = {}
    if rows_per_strip is not None:
        info[278] = rows_per_strip
    if predictor is not None:
        info[317] = predictor
    buf = io.BytesIO()
    Image.fromarray(img, "RGBA" if img.shape[2] == 4 else "RGB").save(buf, format="TIFF", compression=compression, tiffinfo=info)
    return buf.getvalue()


def pillow_read(data):
    """libtiff's decode of a file, as RGB(A) samples"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im)


def stitch_image(synth, cols=480, rows=320):
    """image 1 of synth.make_stitch_set as RGBA samples: texture in a window, transparent black elsewhere (Hugin's border)"""
    _, imgs = synth.make_stitch_set(cols, rows, 1234)
    bgra = imgs[0].numpy()
    return np.ascontiguousarray(bgra[..., [2, 1, 0, 3]])


# (cols, rows, spp, rows per strip, big endian, strip offset mod 4)
GEOMETRY = [(1, 1, 3, 1, False, 0), (1, 2, 4, None, True, 1), (3, 37, 3, 5, False, 2), (3, 1, 4, 1, True, 3),
            (64, 37, 4, 5, True, 0), (64, 2, 3, 1, False, 1), (65, 37, 3, None, True, 2), (65, 37, 4, 1, False, 3),
            (257, 2, 4, None, False, 1), (257, 37, 3, 5, True, 3), (1025, 37, 4, 5, False, 2), (1025, 1, 3, 1, True, 1),
            (1025, 37, 3, None, False, 3)]


def packbits_samples():
    """600 samples (2 rows of 100 RGB pixels): a literal of 1, a repeat of 2, a literal of 128, a repeat of 128, a repeat across the row end"""
    s = [5, 7, 7] + list(range(10, 138)) + [9] * 128 + [200 + (i % 2) * 3 + i for i in range(31)] + [33] * 20
    s += [(i * 7) % 251 for i in range(600 - len(s))]
    return np.array(s, np.uint8).reshape(2, 100, 3)


def cases(synth):
    out = {}
    for k, (cols, rows, spp, rps, be, align) in enumerate(GEOMETRY):
        img = smooth(rows, cols, spp, k) if k % 2 else noise(rows, cols, spp, k)
        tag = "%dx%d_s%d_rps%s_%s_a%d" % (cols, rows, spp, rps, "be" if be else "le", align)
        for comp, cname in ((1, "none"), (5, "lzw")):
            out["geom_%s_%s" % (cname, tag)] = Case(tm.write_tiff(img, comp, be, rps, 1, align), img, True)
    # LZW: the table fills (widths change at 511 / 1023 / 2047 entries, Clear at 4094); the same with the table left full
    big = noise(3, 1000, 4, 77)   # one strip of 12,000 bytes
    out["lzw_noise"] = Case(tm.write_tiff(big, 5), big, True)
    out["lzw_noise_never_clear"] = Case(tm.write_tiff(big, 5, lzw=dict(never_clear=True)), big, False)   # (libtiff refuses a table past 4096 + 1023)
    const = np.full((10, 1000, 4), 7, np.uint8)   # one strip of 40,000 equal bytes: every code is the entry just made
    out["lzw_const"] = Case(tm.write_tiff(const, 5), const, True)
    border = np.empty((10, 1000, 4), np.uint8)
    border[...] = (10, 20, 30, 0)                  # a constant pixel of four distinct bytes
    out["lzw_period4"] = Case(tm.write_tiff(border, 5), border, True)
    sm = smooth(2, 257, 3, 9)
    for n in (1, 63, 64, 65):
        out["lzw_clear_every_%d" % n] = Case(tm.write_tiff(sm, 5, rows_per_strip=1, lzw=dict(clear_every=n)), sm, True)
    out["lzw_no_leading_clear"] = Case(tm.write_tiff(sm, 5, rows_per_strip=1, lzw=dict(clear_at_start=False)), sm, False)   # (read_tiff tolerates it, libtiff does not)
    out["lzw_no_eoi"] = Case(tm.write_tiff(sm, 5, rows_per_strip=1, lzw=dict(eoi="absent")), sm, False)   # (libtiff warns or refuses)
    out["lzw_eoi_padded"] = Case(tm.write_tiff(sm, 5, rows_per_strip=1, lzw=dict(eoi="padded")), sm, True)
    st = stitch_image(synth)
    out["lzw_pillow_stitch_480x320"] = Case(pillow_tiff(st, "tiff_lzw", 1), st, True)
    # predictor 2
    for spp in (3, 4):
        for cols in (1, 65, 1025):
            img = smooth(2, cols, spp, cols)
            for comp, cname in ((1, "none"), (5, "lzw")):
                # (libtiff ignores the predictor tag on uncompressed strips; read_tiff honours it)
                out["pred2_%s_%d_s%d" % (cname, cols, spp)] = Case(tm.write_tiff(img, comp, rows_per_strip=1, predictor=2, align=spp % 4), img, comp == 5)
    out["pred2_pillow_lzw"] = Case(pillow_tiff(st[100:140, :130], "tiff_lzw", 1, 2), st[100:140, :130], True)
    # PackBits
    pb = packbits_samples()
    out["packbits_runs"] = Case(tm.write_tiff(pb, 32773), pb, True)
    out["packbits_noop"] = Case(tm.write_tiff(pb, 32773, rows_per_strip=1, packbits=dict(noop_every=3)), pb, True)
    out["packbits_pillow"] = Case(pillow_tiff(st[100:140, :130], "packbits"), st[100:140, :130], True)
    return out


def malformed():
    """name -> file bytes.  Every strip of these is refused or short; the model (tiff_model.decode) says how many bytes each gives."""
    img = smooth(2, 20, 3, 1)   # strips of 60 bytes at one row per strip
    good = tm.lzw_encode(img[0].tobytes())
    full = tm.lzw_codes(noise(1, 2000, 3, 5).tobytes(), never_clear=True)   # fills the table ...
    out = {
        "code_above_next": tm.write_tiff(img, 5, rows_per_strip=1, strip_bytes={0: tm.lzw_pack([256, 65, 300, 257])}),
        "first_code_not_literal": tm.write_tiff(img, 5, rows_per_strip=1, strip_bytes={1: tm.lzw_pack([256, 65, 66, 256, 258, 257])}),
        "cut_code": tm.write_tiff(img, 5, rows_per_strip=1, strip_bytes={0: good[:len(good) // 2]}),
        "early_eoi": tm.write_tiff(img, 5, rows_per_strip=1, strip_bytes={1: tm.lzw_pack([256, 65, 66, 257])}),
        "packbits_cut_literal": tm.write_tiff(img, 32773, rows_per_strip=1, strip_bytes={0: bytes([9, 1, 2, 3])}),
        "packbits_cut_repeat": tm.write_tiff(img, 32773, rows_per_strip=1, strip_bytes={1: bytes([2, 1, 2, 3, 0xfd])}),
    }
    # ... so that 4095, the last entry, is the highest code a stream can carry: "code == next" cannot be written on a full table
    # (next is 4096 and a code has 12 bits); the strip below ends in codes at and just under the limit and then stops short
    wide = noise(1, 4000, 3, 6)
    out["full_table_last_codes"] = tm.write_tiff(wide, 5, strip_bytes={0: tm.lzw_pack(full[:4000] + [4095, 4094, 257])})
    rnd = np.random.RandomState(2024)
    tall = smooth(200, 20, 3, 2)
    out["random_lzw_strips"] = tm.write_tiff(tall, 5, rows_per_strip=1, strip_bytes={s: rnd.randint(0, 256, 40).astype(np.uint8).tobytes() for s in range(200)})
    return out
