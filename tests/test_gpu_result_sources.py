"""What the file-and-image entry points share (csrc/pf_api_image.inl), held at the C ABI:
the refusals of the eight entry points that read a stitch result in place (pf_stitch_result_* and pf_stitch_batch_result_* of PNG, JPEG,
resize and reprojection), word for word; and the tables the resize, the reprojection and the lens remap keep resident in the arena, which
must follow the arguments of every call -- also when a size comes back, and after a call that outgrew the slot.  The pictures are held to
the models (tests/resize_model.py, reproject_model.py, lens_model.py) for equality, as the families' own case tests hold them."""
import ctypes as C
import os

import numpy as np
import pytest

import lens_cases
import lens_model
import reproject_cases
import reproject_model
import resize_cases
import resize_model

pytestmark = pytest.mark.gpu

PF_ERR_ARG = -1
PCT = 20
FAMILIES = ["png", "jpeg", "resized_dev", "reprojected_dev"]
CAP = 4096   # of the files' buffer: no call here gets as far as writing one


def _name(family, frame):
    return ("pf_stitch_result_" if frame is None else "pf_stitch_batch_result_") + family


def _call(pf, c, family, frame, d_dst, null_dst=False):
    """(rc, message) of the family's entry point on context c: the lone step's result (frame None) or frame slot `frame`.  Every argument
    is valid but what the test is about; the destination is a host buffer for the files, the device buffer d_dst for the images"""
    fn = getattr(c.l, _name(family, frame))
    head = (c.h,) if frame is None else (c.h, int(frame))
    buf = np.zeros(CAP, np.uint8); size = C.c_size_t(0)
    host = None if null_dst else buf.ctypes.data_as(C.c_void_p)
    dev = None if null_dst else C.c_void_p(d_dst)
    if family == "png":
        rc = fn(*head, host, C.c_size_t(CAP), C.byref(size))
    elif family == "jpeg":
        rc = fn(*head, None, host, C.c_size_t(CAP), C.byref(size))
    elif family == "resized_dev":
        rc = fn(*head, 20, 15, resize_model.LANCZOS, dev)
    else:
        rc = fn(*head, 16, 16, C.byref(pf.reproject_params()), dev)
    return rc, c.l.pf_last_error(c.h).decode()


@pytest.fixture(scope="module")
def fresh(pf):
    """a context no stitch call ran on, and device memory of its own for the largest image _call asks for (20 x 15 and 16 x 16)"""
    c = pf.Context(0)
    d = c.dev_alloc(20 * 16 * 4)
    yield c, d
    c.dev_free(d); c.close()


@pytest.fixture(scope="module")
def batched(pf):
    """a context after one stitch_step_batch of two frames: the golden pair and its mirror"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stitch_240x200.npz"))
    L, R = np.ascontiguousarray(g["L"]), np.ascontiguousarray(g["R"])
    c = pf.Context(0)
    d = c.dev_alloc(20 * 16 * 4)
    c.stitch_step_batch([L, np.ascontiguousarray(L[:, ::-1])], [R, np.ascontiguousarray(R[:, ::-1])], PCT)
    yield c, d
    c.dev_free(d); c.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_no_result_on_a_fresh_context(pf, fresh, family):
    c, d = fresh
    assert _call(pf, c, family, None, d) == (PF_ERR_ARG, "%s: no stitch step result in HBM" % _name(family, None))
    assert _call(pf, c, family, 0, d) == (PF_ERR_ARG, "%s: no batch result in frame slot 0 (0 slots hold one)" % _name(family, 0))


@pytest.mark.parametrize("family", FAMILIES)
def test_frames_outside_a_batch_of_two(pf, batched, family):
    c, d = batched
    for frame in (2, -1):
        assert _call(pf, c, family, frame, d) == (PF_ERR_ARG, "%s: no batch result in frame slot %d (2 slots hold one)" % (_name(family, frame), frame))
    # the batch left no lone step's result behind
    assert _call(pf, c, family, None, d) == (PF_ERR_ARG, "%s: no stitch step result in HBM" % _name(family, None))


@pytest.mark.parametrize("family", FAMILIES)
def test_a_null_destination_is_refused_before_the_result_is_looked_for(pf, fresh, family):
    c, d = fresh
    for frame in (None, 0):
        rc, msg = _call(pf, c, family, frame, d, null_dst=True)
        assert rc == PF_ERR_ARG and "null pointer" in msg and "result" not in msg, (frame, rc, msg)


def _differing(got, want):
    return "%d of %d bytes differ" % (int((got != want).sum()), want.size)


def _follow(steps, run, model):
    """run(step) for every step of the sequence: each picture is the model's, and a step that comes back gives what it gave first"""
    first = {}
    for i, step in enumerate(steps):
        got = run(step)
        want = first[step][1] if step in first else model(step)
        assert np.array_equal(got, want), "step %d %r: %s" % (i, step, _differing(got, want))
        if step in first:
            assert np.array_equal(got, first[step][0]), "step %d %r differs from its first occurrence" % (i, step)
        else:
            first[step] = (got, want)
    assert len(first) < len(steps)


def test_resize_tables_follow_the_arguments(pf):
    L, B = resize_model.LANCZOS, resize_model.BILINEAR
    img = resize_cases.image(40, 30)
    # two sizes and two filters in turn, one that comes back, then a call that outgrows both axes' slots, then the first again
    steps = [(20, 15, L), (21, 15, L), (20, 15, B), (20, 15, L), (200, 150, L), (20, 15, L)]
    c = pf.Context(0)
    d_src = c.dev_alloc(img.nbytes)
    try:
        c.upload(d_src, img)

        def run(step):
            out_cols, out_rows, f = step
            host = c.resize(img, out_cols, out_rows, f)
            dev = np.empty_like(host)
            d_dst = c.dev_alloc(dev.nbytes)
            try:
                c.resize_dev(d_src, 40, 30, d_dst, out_cols, out_rows, f)
                c.download(dev, d_dst)
            finally:
                c.dev_free(d_dst)
            assert np.array_equal(dev, host), "device form and host form: " + _differing(dev, host)
            return host
        _follow(steps, run, lambda s: resize_model.resize(img, s[0], s[1], s[2]))
    finally:
        c.dev_free(d_src); c.close()


def test_reproject_tables_follow_the_arguments(pf):
    M = reproject_model
    img = reproject_cases.source_cached("64x32")
    rot = M.rotation(37.0, -21.0, 11.0)
    sizes = [(40, 20), (41, 20), (40, 21), (40, 20), (400, 200), (40, 20)]   # the fifth outgrows the slot of the sines and cosines
    steps = [(w, h, M.BICUBIC if i % 2 == 0 else M.BILINEAR) for i, (w, h) in enumerate(sizes)]
    c = pf.Context(0)
    try:
        run = lambda s: c.reproject(img, s[0], s[1], pf.reproject_params(projection=M.EQUIRECT, filter=s[2], rot=rot))
        _follow(steps, run, lambda s: M.reproject(img, s[0], s[1], M.EQUIRECT, filter=s[2], rot=rot))
    finally:
        c.close()


def test_lens_tables_follow_the_arguments(pf):
    M = lens_model
    photo = lens_cases.photo_cached("64x48")
    lens = lens_cases.make_lens(64, 48, M.EQUIDISTANT, 190.0, "generic", 0, 0, 0, M.BICUBIC)
    p = pf.lens(lens.model, filter=lens.filter, rot=lens.rot, focal_px=lens.focal_px, a=lens.a, b=lens.b, c=lens.c, dd=lens.dd, shift_x=lens.shift_x,
                shift_y=lens.shift_y, min_cos=lens.min_cos, crop_cx256=lens.crop[0], crop_cy256=lens.crop[1], crop_r256=lens.crop[2])
    steps = [(64, 32), (66, 32), (64, 32), (256, 128), (64, 32)]   # the fourth outgrows the slot of the canvas's sines and cosines
    c = pf.Context(0)
    try:
        _follow(steps, lambda s: c.lens_remap(photo, s[0], s[1], p), lambda s: M.remap(photo, s[0], s[1], lens))
    finally:
        c.close()
