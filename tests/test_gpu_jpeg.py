"""The device JPEG encoder (pf_jpeg_*, pf_stitch_result_jpeg, pf_stitch_batch_result_jpeg): the bytes are the function of the image and
the three parameters that DESIGN.md 8.4 specifies, which tests/jpeg_model.py computes serially (and tests/test_jpeg_model.py holds to
libjpeg's own file); the device's files are compared with the model's for equality."""
import ctypes as C
import io
import os

import numpy as np
import pytest
from PIL import Image

import jpeg_cases
import jpeg_model as M

pytestmark = pytest.mark.gpu

PF_ERR_ARG = -1
PCT = 20
QUALITIES = (1, 50, 90, 100)
IMAGES = {"branch_" + k: v.img for k, v in jpeg_cases.branch_cases().items()}
IMAGES.update({"small_" + k: v for k, v in jpeg_cases.small_shapes().items()})


@pytest.fixture(scope="module")
def ctx(pf):
    c = pf.Context(0)
    yield c
    c.close()


def _first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return "%d and %d bytes, first difference at byte %d" % (len(got), len(want), k)


def _decode(data, shape):
    im = Image.open(io.BytesIO(data))
    assert im.format == "JPEG" and im.mode == "RGB" and im.size == (shape[1], shape[0])
    return np.array(im)


def _medium():
    img = jpeg_cases.smooth(1000, 600)
    img[100:300, 200:700] = jpeg_cases.noise(500, 200, 21)
    return img


@pytest.fixture(scope="module")
def medium():
    img = _medium()
    return img, M.encode(img)


def test_restart_interval_is_pinned(pf):
    assert pf.jpeg_restart_interval(0) == M.RESTART[0] == 64
    assert pf.jpeg_restart_interval(1) == M.RESTART[1] == 32
    assert pf.jpeg_restart_interval(2) == 0


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_file_equals_the_serial_model(pf, ctx, name):
    img = IMAGES[name]
    for sub in (0, 1):
        for q in QUALITIES:
            want = M.encode(img, q, sub)
            got = ctx.jpeg_encode(img, pf.jpeg_params(quality=q, subsampling=sub))
            assert got == want, "subsampling %d quality %d: %s" % (sub, q, _first_difference(got, want))
            assert len(got) <= pf.jpeg_bound(img.shape[1], img.shape[0], pf.jpeg_params(subsampling=sub))
        assert np.array_equal(_decode(got, img.shape), _decode(want, img.shape))


def test_medium_shape_host_dev_batch_and_determinism(pf, ctx, medium):
    img, want = medium
    got = ctx.jpeg_encode(img)                                # params NULL: quality 90, 4:2:0
    assert got == want, _first_difference(got, want)
    assert ctx.jpeg_encode(img) == got                        # determinism
    assert np.array_equal(_decode(got, img.shape), _decode(want, img.shape))
    others = [np.ascontiguousarray(img[::-1]), np.ascontiguousarray(img[:, ::-1])]
    ptrs = [ctx.dev_alloc(img.nbytes) for _ in range(3)]
    try:
        for p, im in zip(ptrs, [img] + others):
            ctx.upload(p, im)
        singles = [ctx.jpeg_encode_dev(p, 1000, 600) for p in ptrs]
        assert singles[0] == want and len(set(singles)) == 3
        assert ctx.jpeg_encode_batch_dev(ptrs, 1000, 600) == singles
    finally:
        for p in ptrs:
            ctx.dev_free(p)


def test_row_stride(pf, ctx):
    img = jpeg_cases.noise(65, 37, 4)
    padded = np.full((37, 65 + 11, 4), 0xEE, np.uint8); padded[:, :65] = img
    view = padded[:, :65]
    assert view.strides[0] == (65 + 11) * 4
    assert ctx.jpeg_encode(view) == M.encode(img)


def test_bound_holds_on_noise_at_quality_100(pf, ctx):
    img = jpeg_cases.noise(300, 200, 12)
    for sub in (0, 1):
        p = pf.jpeg_params(quality=100, subsampling=sub)
        data = ctx.jpeg_encode(img, p)
        assert data == M.encode(img, 100, sub)
        assert len(data) <= pf.jpeg_bound(300, 200, p)


def test_capacity(pf, ctx):
    img = jpeg_cases.smooth(300, 200)
    whole = ctx.jpeg_encode(img)
    size = len(whole)
    buf = np.full(size + 64, 0xA5, np.uint8); need = C.c_size_t(0)
    a = np.ascontiguousarray(img)
    call = lambda cap: ctx.l.pf_jpeg_encode(ctx.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(300 * 4), 300, 200, None, buf.ctypes.data_as(C.c_void_p), C.c_size_t(cap), C.byref(need))
    assert call(size - 1) == PF_ERR_ARG
    assert need.value == size
    assert (buf == 0xA5).all()                               # nothing is written
    assert call(need.value) == 0 and need.value == size
    assert buf[:size].tobytes() == whole and (buf[size:] == 0xA5).all()
    with pytest.raises(pf.PngCapacityError) as e:
        ctx.jpeg_encode(img, cap=100)
    assert e.value.needed == size


def test_refusals(pf, ctx):
    img = np.ascontiguousarray(jpeg_cases.smooth(200, 120))
    buf = np.zeros(1 << 20, np.uint8); n = C.c_size_t(0)

    def call(params, cols=200, rows=120):
        return ctx.l.pf_jpeg_encode(ctx.h, img.ctypes.data_as(C.c_void_p), C.c_size_t(200 * 4), cols, rows, C.byref(params), buf.ctypes.data_as(C.c_void_p),
                                    C.c_size_t(buf.size), C.byref(n))

    assert call(pf.jpeg_params()) == 0
    for q in (0, 101, -5):
        assert call(pf.jpeg_params(quality=q)) == PF_ERR_ARG
    for s in (2, -1, 420):
        assert call(pf.jpeg_params(subsampling=s)) == PF_ERR_ARG
    assert call(pf.jpeg_params(gpano=1)) == PF_ERR_ARG        # 200 x 120 is not 2:1
    assert call(pf.jpeg_params(gpano=2)) == PF_ERR_ARG
    # a side above 65535 (the pointer is never followed: the shape is refused first)
    assert call(pf.jpeg_params(), cols=65536, rows=1) == PF_ERR_ARG
    assert call(pf.jpeg_params(), cols=1, rows=65536) == PF_ERR_ARG
    assert pf.jpeg_bound(65536, 1) == 0 and pf.jpeg_bound(65535, 65535) > 0
    bad = pf.jpeg_params(); bad.struct_size = 4
    assert call(bad) == PF_ERR_ARG


def test_gpano(pf, ctx):
    img = jpeg_cases.smooth(200, 100)
    plain = ctx.jpeg_encode(img)
    pano = ctx.jpeg_encode(img, pf.jpeg_params(gpano=1))
    assert plain == M.encode(img) and pano == M.encode(img, gpano=1)
    im = Image.open(io.BytesIO(pano))
    assert [name for name, _ in im.applist[:2]] == ["APP0", "APP1"]
    body = im.applist[1][1]
    assert body.startswith(M.XMP_ID)
    xmp = body[len(M.XMP_ID):].decode()
    for field in ('GPano:ProjectionType="equirectangular"', 'GPano:UsePanoramaViewer="True"', 'GPano:FullPanoWidthPixels="200"', 'GPano:FullPanoHeightPixels="100"',
                  'GPano:CroppedAreaImageWidthPixels="200"', 'GPano:CroppedAreaImageHeightPixels="100"', 'GPano:CroppedAreaLeftPixels="0"', 'GPano:CroppedAreaTopPixels="0"'):
        assert field in xmp, field
    at = pano.index(b"\xff\xe1")
    assert at == 20                                          # directly behind SOI and APP0
    length = int.from_bytes(pano[at + 2:at + 4], "big")
    assert length == len(body) + 2
    assert pano[:at] + pano[at + 2 + length:] == plain
    assert np.array_equal(_decode(pano, img.shape), _decode(plain, img.shape))


def _golden_pair():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stitch_240x200.npz"))
    return np.ascontiguousarray(g["L"]), np.ascontiguousarray(g["R"])


def test_resident_composite_of_a_lone_step(pf, ctx):
    L, R = _golden_pair()
    buf = np.zeros(1 << 20, np.uint8); n = C.c_size_t(0)
    c = pf.Context(0); plain = pf.Context(0)
    try:
        assert c.l.pf_stitch_result_jpeg(c.h, None, buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.size), C.byref(n)) == PF_ERR_ARG
        out1 = c.stitch_step(L, R, PCT)
        panels = c.stitch_visualize()
        data = c.stitch_result_jpeg()
        assert data == c.jpeg_encode(out1) == M.encode(out1)
        # the encode changed nothing: the composite comes down the same, the panels too, and a chained step gives what it gives without it
        again = c.stitch_visualize()
        assert np.array_equal(panels[0], again[0]) and np.array_equal(panels[1], again[1])
        out2 = c.stitch_step(L, None, PCT)
        ref1 = plain.stitch_step(L, R, PCT); ref2 = plain.stitch_step(L, None, PCT)
        assert np.array_equal(ref1, out1) and np.array_equal(ref2, out2)
        assert c.stitch_result_jpeg() == M.encode(ref2)
        # a 3 * cols panel goes through the same encoder
        assert c.jpeg_encode(panels[0]) == M.encode(panels[0])
    finally:
        c.close(); plain.close()


def test_resident_composites_of_a_batch(pf, ctx):
    L, R = _golden_pair()
    Ls, Rs = [L, np.ascontiguousarray(L[:, ::-1])], [R, np.ascontiguousarray(R[:, ::-1])]
    rows, cols = L.shape[:2]
    c = pf.Context(0)
    try:
        buf = np.zeros(1 << 20, np.uint8); n = C.c_size_t(0)
        slot = lambda k: c.l.pf_stitch_batch_result_jpeg(c.h, k, None, buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.size), C.byref(n))
        assert slot(0) == PF_ERR_ARG                          # no batch has run
        outs = c.stitch_step_batch(Ls, Rs, PCT)
        for k in range(2):
            assert c.stitch_batch_result_jpeg(k, (rows, cols)) == c.jpeg_encode(outs[k])
        assert slot(2) == PF_ERR_ARG and slot(-1) == PF_ERR_ARG
        # the slots are still what the next call chains on
        nxt = c.stitch_step_batch([Ls[1], Ls[0]], None, PCT)
        ref = pf.Context(0)
        try:
            ref.stitch_step_batch(Ls, Rs, PCT)
            want = ref.stitch_step_batch([Ls[1], Ls[0]], None, PCT)
        finally:
            ref.close()
        for k in range(2):
            assert np.array_equal(nxt[k], want[k])
    finally:
        c.close()
