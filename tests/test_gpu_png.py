"""The device PNG encoder (pf_png_*, pf_stitch_result_png, pf_stitch_batch_result_png): every file decodes, with the strict reader of
tests/png_decode_ref.py, to exactly the pixels that went in; the sizes hold their bounds; the bytes are a function of the image: the
function DESIGN.md 8.2 specifies, which tests/png_model.py computes serially, and the files are compared with the model's for equality."""
import ctypes as C
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import png_cases
import png_decode_ref as R
import png_model as M

pytestmark = pytest.mark.gpu

PF_ERR_ARG = -1
PCT = 20
SEG = 16380   # pf_png_segment_bytes(), needed when the cases are collected; test_segment_constant pins it
SMALL = png_cases.small_cases(SEG)


@pytest.fixture(scope="module")
def ctx(pf):
    c = pf.Context(0)
    yield c
    c.close()


def _check_file(pf, data, img, with_pil=False):
    rows, cols, _ = img.shape
    got, types = R.decode(data, want_types=True)
    assert got.shape == img.shape and np.array_equal(got, img), "%d bytes differ after decoding" % int((got != img).sum())
    raw = img.nbytes
    print("%dx%d: file %d bytes, %.4f of raw; filter types %s" % (cols, rows, len(data), len(data) / raw, np.bincount(types, minlength=5).tolist()))
    assert len(data) <= raw * 1.001 + 4096 and len(data) <= pf.png_bound(cols, rows)
    if with_pil:
        pil = np.array(Image.open(io.BytesIO(data)))
        assert pil.shape == img.shape and np.array_equal(pil[..., [2, 1, 0, 3]], img)
    return types


def test_segment_constant(pf):
    assert pf.png_segment_bytes() == SEG


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_shapes(pf, ctx, name):
    img = SMALL[name]
    data = ctx.png_encode(img)
    _check_file(pf, data, img)
    assert ctx.png_encode(img) == data                       # determinism
    if name.startswith("fit"):                               # the stream really is k segments, give or take a row
        k = int(name[3]); n = len(R.filtered_stream(data))
        assert n in (k * SEG - png_cases.FIT_ROW_BYTES, k * SEG, k * SEG + png_cases.FIT_ROW_BYTES)


def test_noise_is_stored_and_never_expands(pf, ctx):
    img = png_cases.noise(300, 200, 1)
    data = ctx.png_encode(img)
    _check_file(pf, data, img, with_pil=True)
    assert len(data) > img.nbytes                            # nothing to gain: stored blocks, a few bytes per segment
    assert ctx.png_encode(img) == data


@pytest.mark.parametrize("bgra", [(0, 0, 0, 0), (7, 7, 7, 255)])
def test_constant_images(pf, ctx, bgra):
    img = png_cases.constant(300, 200, bgra)
    data = ctx.png_encode(img)
    _check_file(pf, data, img, with_pil=True)
    assert len(data) <= 0.02 * img.nbytes


def test_ramp_where_sub_wins(pf, ctx):
    img = png_cases.ramp_sub()
    types = _check_file(pf, ctx.png_encode(img), img)
    assert (types == 1).all()


def test_ramp_where_up_wins(pf, ctx):
    img = png_cases.ramp_up()
    types = _check_file(pf, ctx.png_encode(img), img)
    assert (types[1:] == 2).all()


def test_alpha_noise_over_flat_colour(pf, ctx):
    img = png_cases.alpha_noise(300, 200, 2)
    data = ctx.png_encode(img)
    _check_file(pf, data, img, with_pil=True)
    # three of four bytes are flat (residual 0 under any filter but None: at most 2 bits each in a Huffman code that also holds 256 alpha
    # values), the alpha byte is noise (at most 9 bits): 0.75 * 2 / 8 + 0.25 * 9 / 8 = 0.47 of raw, plus headers
    assert len(data) <= 0.5 * img.nbytes


def test_synth_image_beats_the_default_writer(pf, ctx, synth):
    img = synth.make_pair_np(1800, 800, 1234)[0]
    data = ctx.png_encode(img)
    _check_file(pf, data, img, with_pil=True)
    # the default writer (tools/image_io.hpp write_png): filter type 0 on every row, one zlib level-1 stream, one IDAT
    parent = len(R.frame(1800, 800, zlib.compress(R.filter_rows(img, [0] * 800), 1)))
    print("default writer %d bytes (%.4f of raw), device encoder %d bytes (%.4f of raw)" % (parent, parent / img.nbytes, len(data), len(data) / img.nbytes))
    assert len(data) <= parent
    assert ctx.png_encode(img) == data


def test_batch_equals_single_calls(pf, ctx):
    imgs = [png_cases.smooth(300, 200), png_cases.noise(300, 200, 5), png_cases.alpha_noise(300, 200, 6)]
    ptrs = [ctx.dev_alloc(im.nbytes) for im in imgs]
    try:
        for p, im in zip(ptrs, imgs):
            ctx.upload(p, im)
        singles = [ctx.png_encode_dev(p, 300, 200) for p in ptrs]
        assert len(set(singles)) == 3
        assert ctx.png_encode_batch_dev(ptrs, 300, 200) == singles
        for s, im in zip(singles, imgs):
            assert np.array_equal(R.decode(s), im)
    finally:
        for p in ptrs:
            ctx.dev_free(p)


def test_host_form_with_padded_rows_equals_device_form(pf, ctx):
    img = png_cases.smooth(65, 37); img[3:9, 5:40, :] = png_cases.noise(35, 6, 9)
    padded = np.full((37, 65 + 11, 4), 0xEE, np.uint8); padded[:, :65] = img
    view = padded[:, :65]
    assert view.strides[0] == (65 + 11) * 4
    p = ctx.dev_alloc(img.nbytes)
    try:
        ctx.upload(p, img)
        dev = ctx.png_encode_dev(p, 65, 37)
    finally:
        ctx.dev_free(p)
    assert ctx.png_encode(view) == dev
    assert np.array_equal(R.decode(dev), img)


def test_capacity(pf, ctx):
    img = png_cases.smooth(300, 200)
    whole = ctx.png_encode(img)
    size = len(whole)
    buf = np.full(size + 64, 0xA5, np.uint8); need = C.c_size_t(0)
    a = np.ascontiguousarray(img)
    call = lambda cap: ctx.l.pf_png_encode(ctx.h, a.ctypes.data_as(C.c_void_p), C.c_size_t(300 * 4), 300, 200, buf.ctypes.data_as(C.c_void_p), C.c_size_t(cap), C.byref(need))
    assert call(size - 1) == PF_ERR_ARG
    assert need.value == size
    assert (buf[size - 1:] == 0xA5).all()                    # the byte the file lacks room for, and the 64 behind it
    assert call(need.value) == 0 and need.value == size
    assert buf[:size].tobytes() == whole and (buf[size:] == 0xA5).all()
    with pytest.raises(pf.PngCapacityError) as e:
        ctx.png_encode(img, cap=100)
    assert e.value.needed == size


def test_resident_composite_of_a_lone_step(pf, synth):
    cols, rows = 384, 300
    top, imgs = synth.make_stitch_set(cols, rows, 77, 5)
    top = top.numpy(); imgs = [im.numpy() for im in imgs]
    buf = np.zeros(pf.png_bound(cols, rows), np.uint8); n = C.c_size_t(0)
    c = pf.Context(0); plain = pf.Context(0)
    try:
        # a context that has not stitched has nothing to encode
        assert c.l.pf_stitch_result_png(c.h, buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.size), C.byref(n)) == PF_ERR_ARG
        out1 = c.stitch_step(imgs[0], top, PCT)
        panels = c.stitch_visualize()
        data = c.stitch_result_png()
        assert np.array_equal(R.decode(data), out1)
        assert np.array_equal(np.array(Image.open(io.BytesIO(data)))[..., [2, 1, 0, 3]], out1)
        assert c.stitch_result_png() == data
        # the encode changed nothing: the panels still come out the same, and a chained step gives the bytes it gives without it
        again = c.stitch_visualize()
        assert np.array_equal(panels[0], again[0]) and np.array_equal(panels[1], again[1])
        out2 = c.stitch_step(imgs[1], None, PCT, want_out=False)
        assert out2 is None
        ref1 = plain.stitch_step(imgs[0], top, PCT); ref2 = plain.stitch_step(imgs[1], None, PCT)
        assert np.array_equal(ref1, out1)
        assert np.array_equal(R.decode(c.stitch_result_png()), ref2)      # the second composite never came down raw
        # a 3 * cols panel goes through the same encoder
        assert np.array_equal(R.decode(c.png_encode(panels[0])), panels[0])
    finally:
        c.close(); plain.close()


def test_resident_composites_of_a_batch(pf, synth):
    cols, rows = 200, 160
    Ls, Rs = [], []
    for k in range(3):
        top, imgs = synth.make_stitch_set(cols, rows, 300 + k, 5)
        Ls.append(imgs[k].numpy()); Rs.append(top.numpy())
    c = pf.Context(0)
    try:
        buf = np.zeros(pf.png_bound(cols, rows), np.uint8); n = C.c_size_t(0)
        slot = lambda k: c.l.pf_stitch_batch_result_png(c.h, k, buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.size), C.byref(n))
        assert slot(0) == PF_ERR_ARG                          # no batch has run
        outs = c.stitch_step_batch(Ls, Rs, PCT)
        files = [c.stitch_batch_result_png(k, (rows, cols)) for k in range(3)]
        for k in range(3):
            assert np.array_equal(R.decode(files[k]), outs[k])
        assert slot(3) == PF_ERR_ARG and slot(-1) == PF_ERR_ARG
        # the slots are still what the next call chains on
        nxt = c.stitch_step_batch([Ls[1], Ls[2], Ls[0]], None, PCT)
        ref = pf.Context(0)
        try:
            ref.stitch_step_batch(Ls, Rs, PCT)
            want = ref.stitch_step_batch([Ls[1], Ls[2], Ls[0]], None, PCT)
        finally:
            ref.close()
        for k in range(3):
            assert np.array_equal(nxt[k], want[k])
            assert np.array_equal(R.decode(c.stitch_batch_result_png(k, (rows, cols))), want[k])
    finally:
        c.close()


# ---- byte for byte against the serial model ----
def _model_images():
    out = {"small_" + k: v for k, v in SMALL.items()}
    out.update({"branch_" + k: v for k, v in png_cases.branch_cases().items()})
    out.update({"constant_zero": png_cases.constant(300, 200, (0, 0, 0, 0)), "constant_7": png_cases.constant(300, 200, (7, 7, 7, 255)),
                "ramp_sub": png_cases.ramp_sub(), "ramp_up": png_cases.ramp_up(), "noise_300x200": png_cases.noise(300, 200, 1),
                "alpha_noise_300x200": png_cases.alpha_noise(300, 200, 2), "smooth_300x200": png_cases.smooth(300, 200)})
    return out


MODEL_IMAGES = _model_images()
_MODEL = {}


def _model(img):
    key = (img.shape, img.tobytes())
    if key not in _MODEL:
        _MODEL[key] = M.encode(img)
    return _MODEL[key]


def _first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return "%d and %d bytes, first difference at byte %d" % (len(got), len(want), k)


@pytest.mark.parametrize("name", sorted(MODEL_IMAGES))
def test_file_equals_the_serial_model(ctx, name):
    img = MODEL_IMAGES[name]
    want, info = _model(img)
    got = ctx.png_encode(img)
    if got != want:                                          # say where they part before failing: the filter, the parse or the codes
        types = R.decode(got, want_types=True)[1]
        print("filter types differ in rows", np.flatnonzero(types != info["types"]).tolist()[:10])
    assert got == want, _first_difference(got, want)
    if name.startswith("branch_"):                           # the stream's promises, read back from the device's own bytes
        M.check_against_model(got, info)


def test_padded_host_rows_equal_the_serial_model(ctx):
    img = png_cases.smooth(65, 37); img[3:9, 5:40, :] = png_cases.noise(35, 6, 9)
    padded = np.full((37, 65 + 11, 4), 0xEE, np.uint8); padded[:, :65] = img
    assert ctx.png_encode(padded[:, :65]) == _model(img)[0]


def _batch(ctx, imgs):
    rows, cols, _ = imgs[0].shape
    ptrs = [ctx.dev_alloc(im.nbytes) for im in imgs]
    try:
        for p, im in zip(ptrs, imgs):
            ctx.upload(p, im)
        return ctx.png_encode_batch_dev(ptrs, cols, rows)
    finally:
        for p in ptrs:
            ctx.dev_free(p)


def test_batch_of_equal_shapes_equals_the_serial_model(ctx):
    groups = {}
    for name, img in png_cases.branch_cases().items():
        groups.setdefault(img.shape, []).append((name, img))
    groups = {k: v for k, v in groups.items() if len(v) > 1}
    assert {(1, 2, 4), (1, 3, 4), (1, 4, 4), (2, 4, 4), (1, 4134, 4)} <= set(groups)
    for shape, members in sorted(groups.items()):
        files = _batch(ctx, [im for _, im in members])
        for (name, im), got in zip(members, files):
            assert got == _model(im)[0], name


def test_batch_of_one_row_cases_at_a_common_width_equals_the_serial_model(ctx):
    """every one-row case, zero pixels behind it up to the widest: other images than the cases themselves (the filter may choose
    otherwise), of mixed content and one shape, in one call; the model encodes the padded images"""
    rows1 = {k: v for k, v in png_cases.branch_cases().items() if v.shape[0] == 1}
    width = max(v.shape[1] for v in rows1.values())
    assert len(rows1) >= 20 and width == 4134
    imgs = []
    for name in sorted(rows1):
        im = np.zeros((1, width, 4), np.uint8); im[:, :rows1[name].shape[1]] = rows1[name]
        imgs.append(im)
    files = _batch(ctx, imgs)
    assert len(set(files)) == len(files)
    for name, im, got in zip(sorted(rows1), imgs, files):
        assert got == _model(im)[0], name


def test_synth_image_filter_types_equal_the_models(ctx, synth):
    img = synth.make_pair_np(1800, 800, 1234)[0]
    types = R.decode(ctx.png_encode(img), want_types=True)[1]
    want = M.filter_image(img)[1]
    print("filter types %s" % np.bincount(want, minlength=5).tolist())
    assert np.array_equal(types, want), "rows %s" % np.flatnonzero(types != want).tolist()[:10]


def test_more_than_1024_segments_equal_the_serial_model(pf, ctx):
    """341 x 12300 is 1025 segments of 12 rows: k_png_scan's threads sum two sizes each and the last of them none (every other image
    of the suite has at most 352 segments, one per thread).  The image repeats every seven segments, of sizes from 76 bytes to a stored
    16390, so an offset that is wrong anywhere moves bytes; the model encodes the nine distinct segments once each."""
    img = png_cases.many_segments(SEG)
    cache = {}
    want, info = M.encode(img, cache=cache)
    sizes = [s["n"] + M.OVERHEAD if s["stored"] else s["coded_bytes"] for s in info["segments"]]
    assert len(sizes) == 1025 and len(cache) == 9 and len(set(sizes)) >= 7 and len(set(sizes[1:8])) == 7
    assert sum(sizes) + 2 + 4 == len(R.zlib_stream(want))
    got = ctx.png_encode(img)
    assert got == want, _first_difference(got, want)
    M.check_against_model(got, info)                         # check_stream, and the model's account of every segment
    assert np.array_equal(R.decode(got), img)
    assert len(got) <= pf.png_bound(img.shape[1], img.shape[0])
