"""The device TIFF decoder (pf_tiff_*): every well-formed file of tests/tiff_cases.py decodes to exactly the image it was made from
(and libtiff, through Pillow, agrees on that image); the forms agree with each other; refusals are error returns.  The only malformed
stream sent to the GPU is the early-EOI strip, which cannot index anything; the others stay with the host-run kernels
(test_tiff_kernels_host.py)."""
import ctypes as C

import numpy as np
import pytest

import png_decode_ref as R
import tiff_cases
import tiff_model as tm
from conftest import load_pkg_module

pytestmark = pytest.mark.gpu

PF_ERR_ARG = -1
PCT = 20
CASES = tiff_cases.cases(load_pkg_module("synth"))


@pytest.fixture(scope="module")
def ctx(pf):
    c = pf.Context(0)
    yield c
    c.close()


def test_the_list_covers_what_it_should():
    geo = [k for k in CASES if k.startswith("geom_none")]
    assert {k.rsplit("_a", 1)[1] for k in geo} == {"0", "1", "2", "3"}               # every strip alignment on the uncompressed path
    assert {c.img.shape[1] for c in CASES.values()} >= {1, 3, 64, 65, 257, 1025} and {c.img.shape[0] for c in CASES.values()} >= {1, 2, 37}
    assert any("_be_" in k for k in geo) and any("_le_" in k for k in geo)


@pytest.mark.parametrize("name", sorted(CASES))
def test_file_decodes_to_its_image(pf, ctx, name):
    c = CASES[name]
    want = tm.expected_bgra(c.img)
    info = pf.tiff_probe(c.file)
    assert (info.rows, info.cols, info.samples) == c.img.shape and info.device_decodable == 1
    got = ctx.tiff_decode(c.file)
    assert got.shape == want.shape and np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    if c.pillow:
        assert np.array_equal(tiff_cases.pillow_read(c.file), c.img)


def _to_device(ctx, datas, cols, rows, batch):
    ptrs = [ctx.dev_alloc(cols * rows * 4) for _ in datas]
    try:
        if batch:
            ctx.tiff_decode_batch_dev(datas, cols, rows, ptrs)
        else:
            for d, p in zip(datas, ptrs):
                ctx.tiff_decode_dev(d, cols, rows, p)
        return [ctx.download(np.empty((rows, cols, 4), np.uint8), p) for p in ptrs]
    finally:
        for p in ptrs:
            ctx.dev_free(p)


def test_two_decodes_give_the_same_bytes(ctx):
    data = CASES["lzw_pillow_stitch_480x320"].file
    assert np.array_equal(ctx.tiff_decode(data), ctx.tiff_decode(data))


def test_batch_equals_single_calls(ctx):
    imgs = [tiff_cases.noise(37, 65, 4, 1), tiff_cases.smooth(37, 65, 3, 2), tiff_cases.smooth(37, 65, 4, 3)]
    datas = [tm.write_tiff(imgs[0], 5, rows_per_strip=1), tm.write_tiff(imgs[1], 1, rows_per_strip=5, align=1), tm.write_tiff(imgs[2], 32773, big_endian=True)]
    singles = _to_device(ctx, datas, 65, 37, False)
    batch = _to_device(ctx, datas, 65, 37, True)
    for im, a, b in zip(imgs, singles, batch):
        assert np.array_equal(a, tm.expected_bgra(im)) and np.array_equal(a, b)


def test_host_form_leaves_row_padding_untouched(ctx):
    c = CASES["geom_lzw_65x37_s3_rpsNone_be_a2"]
    step = (65 + 11) * 4
    out = np.full((37, step), 0xEE, np.uint8)
    got = ctx.tiff_decode(c.file, row_step=step, out=out)
    assert np.array_equal(got, tm.expected_bgra(c.img)) and (out[:, 65 * 4:] == 0xEE).all()


def test_file_in_file_out(ctx):
    """pf_tiff_decode_dev -> pf_png_encode_dev: no raw image crosses the link in either direction"""
    c = CASES["lzw_pillow_stitch_480x320"]
    p = ctx.dev_alloc(480 * 320 * 4)
    try:
        ctx.tiff_decode_dev(c.file, 480, 320, p)
        png = ctx.png_encode_dev(p, 480, 320)
    finally:
        ctx.dev_free(p)
    assert np.array_equal(R.decode(png), tm.expected_bgra(c.img))


def _raw_decode(ctx, data, cols, rows, p):
    buf = np.frombuffer(data, np.uint8)
    return ctx.l.pf_tiff_decode_dev(ctx.h, buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.size), cols, rows, C.c_void_p(p))


def test_refusals(pf, ctx):
    img = tiff_cases.smooth(37, 65, 4, 3)
    p = ctx.dev_alloc(65 * 37 * 4)
    try:
        deflate = tiff_cases.pillow_tiff(img, "tiff_adobe_deflate")
        assert pf.tiff_probe(deflate).device_decodable == 0
        assert _raw_decode(ctx, deflate, 65, 37, p) == PF_ERR_ARG and b"deflate" in ctx.l.pf_last_error(ctx.h)
        tiled = tm.write_tiff(img, 1, extra_tags=[(322, 4, [16]), (323, 4, [16]), (324, 4, [8])])
        wide = tm.write_tiff(img, 1, extra_tags=[(258, 3, [16, 16, 16, 16])])
        for bad in (tiled, wide, b"II*\0", b""):
            with pytest.raises(pf.PanoflowError):
                pf.tiff_probe(bad)
        good = tm.write_tiff(img, 5, rows_per_strip=1)
        assert _raw_decode(ctx, good, 64, 37, p) == PF_ERR_ARG and _raw_decode(ctx, good, 65, 36, p) == PF_ERR_ARG   # before any work
        assert _raw_decode(ctx, good, 65, 37, p) == 0
    finally:
        ctx.dev_free(p)


def test_early_eoi_is_refused_and_the_output_zeroed(pf, ctx):
    data = tiff_cases.malformed()["early_eoi"]   # 20 x 2 RGB, one row per strip; strip 1 ends after two bytes
    p = ctx.dev_alloc(20 * 2 * 4)
    try:
        ctx.upload(p, np.full((2, 20, 4), 0xEE, np.uint8))
        assert _raw_decode(ctx, data, 20, 2, p) == PF_ERR_ARG
        msg = ctx.l.pf_last_error(ctx.h).decode()
        assert "strip 1" in msg and "2 of 60" in msg, msg
        assert not ctx.download(np.empty((2, 20, 4), np.uint8), p).any()
        host = np.full((2, 80), 0xEE, np.uint8)   # the host form writes nothing
        with pytest.raises(pf.PanoflowError):
            ctx.tiff_decode(data, out=host)
        assert (host == 0xEE).all()
    finally:
        ctx.dev_free(p)


def test_a_decode_between_two_steps_changes_nothing(pf, synth):
    cols, rows = 384, 300
    top, imgs = synth.make_stitch_set(cols, rows, 77, 5)
    top = top.numpy(); imgs = [im.numpy() for im in imgs]
    data = CASES["lzw_pillow_stitch_480x320"].file
    c = pf.Context(0); plain = pf.Context(0)
    try:
        out1 = c.stitch_step(imgs[0], top, PCT)
        panels = c.stitch_visualize()
        assert np.array_equal(c.tiff_decode(data), tm.expected_bgra(CASES["lzw_pillow_stitch_480x320"].img))
        again = c.stitch_visualize()
        assert np.array_equal(panels[0], again[0]) and np.array_equal(panels[1], again[1])
        out2 = c.stitch_step(imgs[1], None, PCT)
        ref1 = plain.stitch_step(imgs[0], top, PCT); ref2 = plain.stitch_step(imgs[1], None, PCT)
        assert np.array_equal(out1, ref1) and np.array_equal(out2, ref2)
    finally:
        c.close(); plain.close()


def test_profile_names_the_kernel_families(pf):
    c = pf.Context(0)
    try:
        c.profile_enable(1)
        c.tiff_decode(CASES["lzw_noise"].file); c.tiff_decode(CASES["packbits_runs"].file)
        prof = c.profile()
        assert {"tiff_lzw", "tiff_packbits", "tiff_finish"} <= set(prof) and prof["tiff_finish"][1] == 2 and prof["tiff_lzw"][1] == 1
    finally:
        c.close()
