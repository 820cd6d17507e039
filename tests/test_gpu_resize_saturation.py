"""The byte packing of the device resize where it saturates (csrc/kernels_resize.hip: RzAcc::pack, rz_unpremultiply's min(255, ...)).
The random images of tests/test_gpu_resize.py hardly ever leave [0, 255] upward in a colour channel, so a pack() that lost an upper clamp,
or an un-premultiply that mishandled colour above alpha, would pass there.  Here:
  * the ringing image (resize_cases.ringing) makes the negative lobes of LANCZOS and BICUBIC overshoot in all four channels; the model
    (tests/resize_model.py) must clamp at least 10 outputs from below 0 and 10 from above 255 per channel in every pass that runs -- a
    condition on the inputs, asserted on the model alone -- and pf_resize / pf_resize_dev must give the model's bytes, for the opaque image
    and for the translucent one, whose overshoot is colour above alpha;
  * pf_stage_resize_pass runs one pass alone with its fusions chosen, for each of the two kernels: the un-premultiply and the premultiply
    over all 65536 (colour, alpha) pairs in all three byte positions, and the clamp's raw bytes with neither fusion behind it.
A mismatch is reported per channel and per class of the model's last pass (clamped low, clamped high, unclamped)."""
import ctypes as C

import numpy as np
import pytest

import resize_cases
import resize_model as M

pytestmark = pytest.mark.gpu

PF_ERR_ARG = -1


@pytest.fixture(scope="module")
def ctx(pf):
    c = pf.Context(0)
    yield c
    c.close()


def _resize_dev(ctx, img, out_cols, out_rows, f):
    rows, cols = img.shape[:2]
    out = np.empty((out_rows, out_cols, 4), np.uint8)
    d_src, d_dst = ctx.dev_alloc(img.nbytes), ctx.dev_alloc(out.nbytes)
    try:
        ctx.upload(d_src, img)
        ctx.resize_dev(d_src, cols, rows, d_dst, out_cols, out_rows, f)
        return ctx.download(out, d_dst)
    finally:
        ctx.dev_free(d_src); ctx.dev_free(d_dst)


@pytest.mark.parametrize("rest_alpha", [255, 128], ids=["opaque", "translucent"])
@pytest.mark.parametrize("f", resize_cases.RINGING_FILTERS)
@pytest.mark.parametrize("shape", resize_cases.RINGING_SHAPES, ids=lambda s: "%dx%d_to_%dx%d_b%dx%d" % s)
def test_ringing_image_host_and_dev(ctx, shape, f, rest_alpha):
    img, want, cls = resize_cases.ringing_case(shape, f, rest_alpha)   # asserts the clamp counts of the model
    got = ctx.resize(img, shape[2], shape[3], f)
    assert np.array_equal(got, want), "pf_resize: " + resize_cases.differing_by_class(got, want, cls)
    got = _resize_dev(ctx, img, shape[2], shape[3], f)
    assert np.array_equal(got, want), "pf_resize_dev: " + resize_cases.differing_by_class(got, want, cls)


@pytest.mark.parametrize("k", range(8), ids=lambda k: resize_cases.pass_cases()[k][0])
def test_one_pass_alone(ctx, k):
    name, img, axis, n_out, f, premul, unpremul, want, cls = resize_cases.pass_cases()[k]
    ctx.profile_enable(1); ctx.profile_reset()
    try:
        got = ctx.stage_resize_pass(img, axis, n_out, f, premul, unpremul)
        prof = ctx.profile()
    finally:
        ctx.profile_enable(0)
    assert np.array_equal(got, want), resize_cases.differing_by_class(got, want, cls)
    # exactly one launch, of the kernel of that axis
    ran, other = ("resize_v", "resize_h") if axis else ("resize_h", "resize_v")
    assert prof[ran][1] == 1 and prof.get(other, (0.0, 0))[1] == 0 and all(n.startswith("resize_") for n in prof), prof


def test_one_pass_refusals(ctx):
    img = resize_cases.image(40, 30)
    out = np.zeros((30, 40, 4), np.uint8)

    def run(src=img, cols=40, rows=30, axis=0, n_out=20, f=M.LANCZOS, dst=out):
        sp = src.ctypes.data_as(C.c_void_p) if src is not None else None
        dp = dst.ctypes.data_as(C.c_void_p) if dst is not None else None
        return ctx.l.pf_stage_resize_pass(ctx.h, sp, cols, rows, axis, n_out, f, 1, 1, dp)

    def refused(rc, word):
        msg = ctx.l.pf_last_error(ctx.h).decode()
        assert rc == PF_ERR_ARG and word in msg, (rc, word, msg)

    assert run() == 0 and run(axis=1) == 0
    refused(run(src=None), "null"); refused(run(dst=None), "null")
    refused(run(axis=2), "axis"); refused(run(axis=-1), "axis")
    refused(run(cols=0), "bad image size"); refused(run(rows=-1), "bad image size")
    refused(run(n_out=0), "bad output size"); refused(run(axis=1, n_out=-3), "bad output size")
    refused(run(cols=50000, rows=50000), "too large"); refused(run(n_out=2000000000), "too large")
    for f in (0, 6, -1):
        refused(run(f=f), "unknown filter")
    refused(run(cols=3000000, rows=1, n_out=1), "coefficients"); refused(run(cols=1, rows=3000000, axis=1, n_out=1), "coefficients")
    both = np.zeros((60, 40, 4), np.uint8)
    refused(run(src=both[:30], dst=both[15:]), "overlaps")
    # a pass to the size the axis has still runs, and BOX then returns the image
    assert np.array_equal(ctx.stage_resize_pass(img, 0, 40, M.BOX, 0, 0), img) and np.array_equal(ctx.stage_resize_pass(img, 1, 30, M.BOX, 0, 0), img)
