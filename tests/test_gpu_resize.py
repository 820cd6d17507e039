"""The device resize (pf_resize*, pf_stitch_result_resized_dev, pf_stitch_batch_result_resized_dev): the bytes are the function of the image,
the size and the filter that DESIGN.md 8.5 specifies, which tests/resize_model.py computes serially (and tests/test_resize_model.py holds
to Pillow's Image.resize); the device's images are compared with the model's for equality."""
import ctypes as C
import os

import numpy as np
import pytest

import jpeg_model
import resize_cases
import resize_model as M

pytestmark = pytest.mark.gpu

PF_ERR_ARG = -1
PCT = 20


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


def _differing(got, want):
    return "%d of %d bytes differ" % (int((got != want).sum()), want.size)


@pytest.mark.parametrize("f", resize_cases.FILTER_IDS)
@pytest.mark.parametrize("shape", resize_cases.MODEL_SHAPES + [resize_cases.PIECE_SHAPE], ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_model_shapes_host_and_dev(ctx, shape, f):
    cols, rows, out_cols, out_rows = shape
    img = resize_cases.image(cols, rows)
    want = resize_cases.model(shape, img, out_cols, out_rows, f)
    got = ctx.resize(img, out_cols, out_rows, f)
    assert np.array_equal(got, want), _differing(got, want)
    got = _resize_dev(ctx, img, out_cols, out_rows, f)
    assert np.array_equal(got, want), _differing(got, want)


@pytest.mark.parametrize("f", resize_cases.FILTER_IDS)
def test_same_size_is_a_copy(ctx, f):
    img = resize_cases.all_pairs()
    assert np.array_equal(ctx.resize(img, 256, 256, f), img)
    assert np.array_equal(_resize_dev(ctx, img, 256, 256, f), img)


def test_all_pairs_box_doubling(ctx):
    img = resize_cases.all_pairs()
    want = resize_cases.model("pairs", img, 512, 512, M.BOX)
    assert np.array_equal(want, np.repeat(np.repeat(M.unpremultiply(M.premultiply(img)), 2, axis=0), 2, axis=1))
    for got in (ctx.resize(img, 512, 512, M.BOX), _resize_dev(ctx, img, 512, 512, M.BOX)):
        assert np.array_equal(got, want), _differing(got, want)


@pytest.mark.parametrize("shape", resize_cases.edge_shapes(), ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_tile_and_workgroup_edges(ctx, shape):
    cols, rows, out_cols, out_rows = shape
    img = resize_cases.image(cols, rows)
    for f in resize_cases.FILTER_IDS:
        want = resize_cases.model(shape, img, out_cols, out_rows, f)
        got = ctx.resize(img, out_cols, out_rows, f)
        assert np.array_equal(got, want), "filter %d: %s" % (f, _differing(got, want))


def test_one_axis_at_the_edges(ctx):
    # one pass alone carries both fusions: the same edges with the other axis unchanged
    for cols, rows, out_cols, out_rows in [(141, 9, 64, 9), (180, 6, 257, 6), (9, 141, 9, 65), (7, 179, 7, 256)]:
        img = resize_cases.image(cols, rows)
        for f in (M.LANCZOS, M.BOX):
            got, want = ctx.resize(img, out_cols, out_rows, f), M.resize(img, out_cols, out_rows, f)
            assert np.array_equal(got, want), "%dx%d -> %dx%d filter %d: %s" % (cols, rows, out_cols, out_rows, f, _differing(got, want))


def test_medium_shape_row_stride_and_families(ctx):
    cols, rows, out_cols, out_rows = resize_cases.MEDIUM_SHAPE
    img = resize_cases.image(cols, rows)
    want = resize_cases.model("medium", img, out_cols, out_rows, M.LANCZOS)
    ctx.profile_enable(1); ctx.profile_reset()
    try:
        got = _resize_dev(ctx, img, out_cols, out_rows, M.LANCZOS)
        prof = ctx.profile()
    finally:
        ctx.profile_enable(0)
    assert np.array_equal(got, want), _differing(got, want)
    assert prof["resize_h"][1] == 1 and prof["resize_v"][1] == 1
    # padded rows on both sides of the host form; the destination's padding stays
    padded = np.full((rows, cols + 5, 4), 0xEE, np.uint8); padded[:, :cols] = img
    out = np.full((out_rows, out_cols + 3, 4), 0xA5, np.uint8)
    ctx.resize(padded[:, :cols], out_cols, out_rows, M.LANCZOS, out=out[:, :out_cols])
    assert np.array_equal(out[:, :out_cols], want) and (out[:, out_cols:] == 0xA5).all()


def test_batch_equals_single_calls(ctx):
    cols, rows, out_cols, out_rows = 150, 70, 65, 33
    imgs = [resize_cases.image(cols, rows, seed) for seed in (1, 2, 3)]
    outs = [np.empty((out_rows, out_cols, 4), np.uint8) for _ in imgs]
    srcs = [ctx.dev_alloc(im.nbytes) for im in imgs]; dsts = [ctx.dev_alloc(o.nbytes) for o in outs]
    try:
        for p, im in zip(srcs, imgs):
            ctx.upload(p, im)
        ctx.resize_batch_dev(srcs, cols, rows, dsts, out_cols, out_rows, M.BICUBIC)
        for p, o in zip(dsts, outs):
            ctx.download(o, p)
    finally:
        for p in srcs + dsts:
            ctx.dev_free(p)
    singles = [_resize_dev(ctx, im, out_cols, out_rows, M.BICUBIC) for im in imgs]
    for k in range(3):
        assert np.array_equal(outs[k], singles[k]) and np.array_equal(outs[k], M.resize(imgs[k], out_cols, out_rows, M.BICUBIC))
    assert not np.array_equal(outs[0], outs[1])


def test_refusals(pf, ctx):
    img = resize_cases.image(40, 30)
    d_src, d_dst = ctx.dev_alloc(img.nbytes), ctx.dev_alloc(40 * 30 * 4)
    host_out = np.zeros((30, 40, 4), np.uint8)

    def dev(src=d_src, cols=40, rows=30, dst=d_dst, out_cols=20, out_rows=15, f=M.LANCZOS):
        return ctx.l.pf_resize_dev(ctx.h, C.c_void_p(src), cols, rows, C.c_void_p(dst), out_cols, out_rows, f)

    def host(src=img, cols=40, rows=30, dst=host_out, out_cols=20, out_rows=15, f=M.LANCZOS, src_step=160, dst_step=160):
        sp = src.ctypes.data_as(C.c_void_p) if src is not None else None
        dp = dst.ctypes.data_as(C.c_void_p) if dst is not None else None
        return ctx.l.pf_resize(ctx.h, sp, C.c_size_t(src_step), cols, rows, dp, C.c_size_t(dst_step), out_cols, out_rows, f)

    def refused(rc, word):
        msg = ctx.l.pf_last_error(ctx.h).decode()
        assert rc == PF_ERR_ARG and word in msg, (rc, word, msg)

    try:
        ctx.upload(d_src, img)
        assert dev() == 0 and host() == 0
        refused(dev(src=None), "null"); refused(dev(dst=None), "null"); refused(host(src=None), "null"); refused(host(dst=None), "null")
        for bad in (dict(cols=0), dict(rows=-1)):
            refused(dev(**bad), "bad image size"); refused(host(**bad), "bad image size")
        for bad in (dict(out_cols=0), dict(out_rows=-3)):
            refused(dev(**bad), "bad output size"); refused(host(**bad), "bad output size")
        # more than 2e9 pixels on either side (the pointers are never followed: the shape is refused first)
        refused(dev(cols=50000, rows=50000), "too large"); refused(dev(out_cols=50000, out_rows=50000), "too large")
        refused(host(cols=50000, rows=50000), "too large"); refused(host(out_cols=50000, out_rows=50000), "too large")
        for f in (0, 6, -1):
            refused(dev(f=f), "unknown filter"); refused(host(f=f), "unknown filter")
        # a destination inside the source, and one that ends inside it
        refused(dev(dst=d_src), "overlaps"); refused(dev(dst=d_src + 40 * 29 * 4), "overlaps"); refused(dev(src=d_dst + 400, dst=d_dst), "overlaps")
        both = np.zeros((60, 40, 4), np.uint8)
        refused(host(src=both[:30], dst=both[15:]), "overlaps")
        assert host(src=both[:30], dst=both[30:]) == 0
        # a table beyond the documented bound: 3 000 000 -> 1 with LANCZOS needs 18 000 001 coefficients
        refused(dev(cols=3000000, rows=1, out_cols=1, out_rows=1), "coefficients"); refused(dev(cols=1, rows=3000000, out_cols=1, out_rows=1), "coefficients")
        refused(host(src_step=159), "step"); refused(host(dst_step=79), "step")
        refused(ctx.l.pf_resize_batch_dev(ctx.h, -1, None, 40, 30, None, 20, 15, M.LANCZOS), "bad argument")
        assert dev() == 0
    finally:
        ctx.dev_free(d_src); ctx.dev_free(d_dst)


def _golden_pair():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stitch_240x200.npz"))
    return np.ascontiguousarray(g["L"]), np.ascontiguousarray(g["R"])


def test_resident_composite_of_a_lone_step(pf, ctx):
    L, R = _golden_pair()
    out_cols, out_rows = 100, 50
    small = np.empty((out_rows, out_cols, 4), np.uint8)
    c = pf.Context(0); plain = pf.Context(0)
    d = c.dev_alloc(small.nbytes)
    try:
        assert c.l.pf_stitch_result_resized_dev(c.h, out_cols, out_rows, M.LANCZOS, C.c_void_p(d)) == PF_ERR_ARG
        assert "no stitch step result" in c.l.pf_last_error(c.h).decode()
        out1 = c.stitch_step(L, R, PCT)
        want = M.resize(out1, out_cols, out_rows, M.LANCZOS)
        c.stitch_result_resized_dev(out_cols, out_rows, d)                     # the default filter
        assert np.array_equal(c.download(small, d), want), _differing(small, want)
        # the chain into the encoder is exact
        assert c.jpeg_encode_dev(d, out_cols, out_rows) == jpeg_model.encode(want)
        assert c.jpeg_encode_dev(d, out_cols, out_rows, pf.jpeg_params(gpano=1)) == jpeg_model.encode(want, gpano=1)
        c.stitch_result_resized_dev(out_cols, out_rows, d, M.BOX)
        assert np.array_equal(c.download(small, d), M.resize(out1, out_cols, out_rows, M.BOX))
        # the resize changed nothing: a chained step gives what it gives without it, and the full composite is still the encoder's
        out2 = c.stitch_step(L, None, PCT)
        ref1 = plain.stitch_step(L, R, PCT); ref2 = plain.stitch_step(L, None, PCT)
        assert np.array_equal(ref1, out1) and np.array_equal(ref2, out2)
        c.stitch_result_resized_dev(out_cols, out_rows, d, M.HAMMING)
        assert np.array_equal(c.download(small, d), M.resize(ref2, out_cols, out_rows, M.HAMMING))
    finally:
        c.dev_free(d); c.close(); plain.close()


def test_resident_composites_of_a_batch(pf, ctx):
    L, R = _golden_pair()
    Ls, Rs = [L, np.ascontiguousarray(L[:, ::-1])], [R, np.ascontiguousarray(R[:, ::-1])]
    out_cols, out_rows = 77, 130
    small = np.empty((out_rows, out_cols, 4), np.uint8)
    c = pf.Context(0)
    d = c.dev_alloc(small.nbytes)
    try:
        slot = lambda k: c.l.pf_stitch_batch_result_resized_dev(c.h, k, out_cols, out_rows, M.BILINEAR, C.c_void_p(d))
        assert slot(0) == PF_ERR_ARG and "no batch result" in c.l.pf_last_error(c.h).decode()
        outs = c.stitch_step_batch(Ls, Rs, PCT)
        for k in range(2):
            c.stitch_batch_result_resized_dev(k, out_cols, out_rows, d, M.BILINEAR)
            want = M.resize(outs[k], out_cols, out_rows, M.BILINEAR)
            assert np.array_equal(c.download(small, d), want), _differing(small, want)
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
        c.dev_free(d); c.close()
