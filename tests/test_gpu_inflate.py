"""The device TIFF decoder with the inflate switch on (pf_tiff_set_inflate): every well-formed deflate file of tests/inflate_cases.py
decodes to exactly the image it was made from; the forms agree with each other and mix with the other compressions in a batch; with the
switch off the same file is refused as before.  Two malformed streams go to the GPU, neither of which can index anything: a valid
stream that is 10 bytes short and a flipped trailer; the others stay with the host-run kernel (test_tiff_inflate_host.py)."""
import ctypes as C

import numpy as np
import pytest

import inflate_cases as ic
import png_decode_ref as R
import tiff_cases
import tiff_model as tm
from conftest import load_pkg_module

pytestmark = pytest.mark.gpu

PF_ERR_ARG = -1
PCT = 20
CASES = ic.cases(load_pkg_module("synth"))


@pytest.fixture(scope="module")
def ctx(pf):
    c = pf.Context(0)
    c.tiff_set_inflate(1)
    yield c
    c.close()


@pytest.mark.parametrize("name", sorted(CASES))
def test_file_decodes_to_its_image(pf, ctx, name):
    c = CASES[name]
    want = tm.expected_bgra(c.img)
    info = pf.tiff_probe(c.file)
    assert (info.rows, info.cols, info.samples) == c.img.shape and info.compression in (8, 32946)
    assert info.device_decodable == 0 and not pf.tiff_device_decodable(info) and pf.tiff_device_decodable(info, ctx)
    got = ctx.tiff_decode(c.file)
    assert got.shape == want.shape and np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())


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
    data = CASES["pillow_stitch_480x320"].file
    assert np.array_equal(ctx.tiff_decode(data), ctx.tiff_decode(data))


def test_batch_of_mixed_compressions_equals_single_calls(ctx):
    imgs = [tiff_cases.noise(37, 65, 4, 1), tiff_cases.smooth(37, 65, 3, 2), tiff_cases.smooth(37, 65, 4, 3), tiff_cases.smooth(37, 65, 4, 4)]
    datas = [tiff_cases.pillow_tiff(imgs[0], "tiff_adobe_deflate", 1), tm.write_tiff(imgs[1], 5, rows_per_strip=1),
             tm.write_tiff(imgs[2], 1, rows_per_strip=5, align=1), tiff_cases.pillow_tiff(imgs[3], "tiff_adobe_deflate", 5, 2)]
    singles = _to_device(ctx, datas, 65, 37, False)
    batch = _to_device(ctx, datas, 65, 37, True)
    for img, a, b in zip(imgs, singles, batch):
        assert np.array_equal(a, tm.expected_bgra(img)) and np.array_equal(a, b)


def test_host_form_leaves_row_padding_untouched(ctx):
    c = CASES["pillow_65x37_pred2"]
    step = (65 + 11) * 4
    out = np.full((37, step), 0xEE, np.uint8)
    got = ctx.tiff_decode(c.file, row_step=step, out=out)
    assert np.array_equal(got, tm.expected_bgra(c.img)) and (out[:, 65 * 4:] == 0xEE).all()


def test_file_in_file_out(ctx):
    """pf_tiff_decode_dev -> pf_png_encode_dev: no raw image crosses the link in either direction"""
    c = CASES["pillow_stitch_480x320_pred2"]
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


def test_the_switch_is_off_by_default_and_can_be_turned_off_again(pf):
    c = CASES["pillow_65x37"]
    ctx = pf.Context(0)
    p = ctx.dev_alloc(65 * 37 * 4)
    try:
        assert _raw_decode(ctx, c.file, 65, 37, p) == PF_ERR_ARG and b"deflate" in ctx.l.pf_last_error(ctx.h)
        ctx.tiff_set_inflate(1)
        assert pf.tiff_device_decodable(pf.tiff_probe(c.file), ctx) and _raw_decode(ctx, c.file, 65, 37, p) == 0
        assert np.array_equal(ctx.download(np.empty((37, 65, 4), np.uint8), p), tm.expected_bgra(c.img))
        ctx.tiff_set_inflate(0)
        assert not pf.tiff_device_decodable(pf.tiff_probe(c.file), ctx)
        assert _raw_decode(ctx, c.file, 65, 37, p) == PF_ERR_ARG and b"deflate" in ctx.l.pf_last_error(ctx.h)
    finally:
        ctx.dev_free(p); ctx.close()


@pytest.mark.parametrize("name,said", [("ten_bytes_short", "decoded 50 of 60 bytes (the stream ends early)"),
                                       ("trailer_bit_flipped", "decoded 60 of 60 bytes (the Adler-32 does not match)")])
def test_a_bad_strip_is_refused_and_the_output_zeroed(pf, ctx, name, said):
    bad = ic.malformed()[name]   # 20 x 2 RGB, one row per strip
    p = ctx.dev_alloc(20 * 2 * 4)
    try:
        ctx.upload(p, np.full((2, 20, 4), 0xEE, np.uint8))
        assert _raw_decode(ctx, bad.file, 20, 2, p) == PF_ERR_ARG
        msg = ctx.l.pf_last_error(ctx.h).decode()
        assert "strip %d" % bad.strip in msg and said in msg, msg
        assert not ctx.download(np.empty((2, 20, 4), np.uint8), p).any()
        host = np.full((2, 80), 0xEE, np.uint8)   # the host form writes nothing
        with pytest.raises(pf.PanoflowError):
            ctx.tiff_decode(bad.file, out=host)
        assert (host == 0xEE).all()
    finally:
        ctx.dev_free(p)


def test_a_decode_between_two_steps_changes_nothing(pf, synth):
    cols, rows = 384, 300
    top, imgs = synth.make_stitch_set(cols, rows, 77, 5)
    top = top.numpy(); imgs = [img.numpy() for img in imgs]
    case = CASES["pillow_stitch_480x320"]
    c = pf.Context(0); plain = pf.Context(0)
    try:
        c.tiff_set_inflate(1)
        out1 = c.stitch_step(imgs[0], top, PCT)
        panels = c.stitch_visualize()
        assert np.array_equal(c.tiff_decode(case.file), tm.expected_bgra(case.img))
        again = c.stitch_visualize()
        assert np.array_equal(panels[0], again[0]) and np.array_equal(panels[1], again[1])
        out2 = c.stitch_step(imgs[1], None, PCT)
        ref1 = plain.stitch_step(imgs[0], top, PCT); ref2 = plain.stitch_step(imgs[1], None, PCT)
        assert np.array_equal(out1, ref1) and np.array_equal(out2, ref2)
    finally:
        c.close(); plain.close()


def test_profile_names_the_kernel_family(pf):
    c = pf.Context(0)
    try:
        c.tiff_set_inflate(1)
        c.profile_enable(1)
        c.tiff_decode(CASES["pillow_65x37"].file)
        prof = c.profile()
        assert {"tiff_inflate", "tiff_finish"} <= set(prof) and prof["tiff_inflate"][1] == 1 and "tiff_lzw" not in prof
    finally:
        c.close()
