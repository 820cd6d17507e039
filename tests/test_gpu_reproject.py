"""The device reprojection (pf_reproject*, pf_stitch_result_reprojected_dev, pf_stitch_batch_result_reprojected_dev,
pf_stage_reproject_coords): the bytes and the quantised coordinates are the function of the image, the sizes and the parameters that
DESIGN.md 8.6 specifies, which tests/reproject_model.py computes (and tests/test_reproject_model.py holds to libm and to the
geometry's properties); everything the device gives is compared with the model's for equality."""
import ctypes as C
import os

import numpy as np
import pytest

import png_decode_ref
import reproject_cases
import reproject_model as M

pytestmark = pytest.mark.gpu

PF_ERR_ARG = -1
PCT = 20


@pytest.fixture(scope="module")
def ctx(pf):
    c = pf.Context(0)
    yield c
    c.close()


def _params(pf, case):
    _, s, proj, w, h, face, hfov, r, f = case
    return pf.reproject_params(projection=proj, face=face, filter=f, hfov_deg=hfov if proj == M.RECTILINEAR else None, rot=reproject_cases.ROTATIONS[r])


def _reproject_dev(ctx, img, out_cols, out_rows, params):
    rows, cols = img.shape[:2]
    out = np.empty((out_rows, out_cols, 4), np.uint8)
    d_src, d_dst = ctx.dev_alloc(img.nbytes), ctx.dev_alloc(out.nbytes)
    try:
        ctx.upload(d_src, np.ascontiguousarray(img))
        ctx.reproject_dev(d_src, cols, rows, d_dst, out_cols, out_rows, params)
        return ctx.download(out, d_dst)
    finally:
        ctx.dev_free(d_src); ctx.dev_free(d_dst)


def _differing(got, want):
    return "%d of %d differ" % (int((got != want).sum()), want.size)


@pytest.mark.parametrize("rot", list(reproject_cases.ROTATIONS))
@pytest.mark.parametrize("src", reproject_cases.SOURCES)
def test_cases_host_form_device_form_and_coordinates(pf, ctx, src, rot):
    img = reproject_cases.source_cached(src)
    rows, cols = img.shape[:2]
    d_src = ctx.dev_alloc(img.nbytes)
    bad = []
    try:
        ctx.upload(d_src, np.ascontiguousarray(img))
        for case in reproject_cases.cases():
            if case[1] != src or case[7] != rot:
                continue
            w, h = case[3], case[4]
            p = _params(pf, case)
            if case[8] == M.BICUBIC:   # the coordinates do not depend on the filter: once per geometry
                fx, fy = ctx.stage_reproject_coords(cols, rows, w, h, p)
                mfx, mfy = reproject_cases.model_coords(case)
                if not (np.array_equal(fx, mfx) and np.array_equal(fy, mfy)):
                    bad.append("%s coordinates: fx %s, fy %s" % (case[0], _differing(fx, mfx), _differing(fy, mfy)))
            want = reproject_cases.model_image(case)
            got = ctx.reproject(img, w, h, p)
            if not np.array_equal(got, want):
                bad.append("%s host form: %s" % (case[0], _differing(got, want)))
            out = np.empty((h, w, 4), np.uint8)
            d_dst = ctx.dev_alloc(out.nbytes)
            try:
                ctx.reproject_dev(d_src, cols, rows, d_dst, w, h, p)
                ctx.download(out, d_dst)
            finally:
                ctx.dev_free(d_dst)
            if not np.array_equal(out, want):
                bad.append("%s device form: %s" % (case[0], _differing(out, want)))
    finally:
        ctx.dev_free(d_src)
    assert not bad, "%d mismatches: %s" % (len(bad), bad[:10])


@pytest.mark.parametrize("case", reproject_cases.ringing_cases(), ids=lambda c: c[0])
def test_ringing_source_clamps_in_every_channel(pf, ctx, case):
    low, high = reproject_cases.clamp_counts(case)   # a condition on the inputs, on the model alone
    assert min(low + high) >= reproject_cases.RINGING_MIN_CLAMPED, (low, high)
    img = reproject_cases.source_cached(case[1])
    want = reproject_cases.model_image(case)
    p = _params(pf, case)
    got = ctx.reproject(img, case[3], case[4], p)
    assert np.array_equal(got, want), "host form: " + _differing(got, want)
    got = _reproject_dev(ctx, img, case[3], case[4], p)
    assert np.array_equal(got, want), "device form: " + _differing(got, want)


def test_row_strides_and_profile_family(pf, ctx):
    img = reproject_cases.source_cached("90x40")
    p = pf.reproject_params(projection=M.EQUIRECT, filter=M.BICUBIC, rot=M.rotation(37.0, -21.0, 11.0))
    want = M.reproject(img, 130, 65, M.EQUIRECT, filter=M.BICUBIC, rot=M.rotation(37.0, -21.0, 11.0))
    padded = np.full((40, 95, 4), 0xEE, np.uint8); padded[:, :90] = img
    out = np.full((65, 133, 4), 0xA5, np.uint8)
    ctx.profile_enable(1); ctx.profile_reset()
    try:
        ctx.reproject(padded[:, :90], 130, 65, p, out=out[:, :130])
        prof = ctx.profile()
    finally:
        ctx.profile_enable(0)
    assert np.array_equal(out[:, :130], want) and (out[:, 130:] == 0xA5).all()
    assert prof["reproject"][1] == 1


def test_batch_equals_single_calls(pf, ctx):
    cols, rows, w, h = 90, 40, 65, 33
    imgs = [np.ascontiguousarray(np.roll(reproject_cases.source_cached("90x40"), 7 * k, axis=1)) for k in range(3)]
    rot = M.rotation(37.0, -21.0, 11.0)
    p = pf.reproject_params(projection=M.RECTILINEAR, filter=M.BICUBIC, hfov_deg=100.0, rot=rot)
    outs = [np.empty((h, w, 4), np.uint8) for _ in imgs]
    srcs = [ctx.dev_alloc(im.nbytes) for im in imgs]; dsts = [ctx.dev_alloc(o.nbytes) for o in outs]
    try:
        for d, im in zip(srcs, imgs):
            ctx.upload(d, im)
        ctx.reproject_batch_dev(srcs, cols, rows, dsts, w, h, p)
        for d, o in zip(dsts, outs):
            ctx.download(o, d)
    finally:
        for d in srcs + dsts:
            ctx.dev_free(d)
    for k in range(3):
        assert np.array_equal(outs[k], _reproject_dev(ctx, imgs[k], w, h, p))
        assert np.array_equal(outs[k], M.reproject(imgs[k], w, h, M.RECTILINEAR, filter=M.BICUBIC, hfov_deg=100.0, rot=rot))
    assert not np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("flt", reproject_cases.FILTERS)
def test_cube_set_equals_six_single_calls(pf, ctx, flt):
    img = reproject_cases.source_cached("67x33")
    rot = M.rotation(37.0, -21.0, 11.0)
    n = 65
    faces = [np.empty((n, n, 4), np.uint8) for _ in range(6)]
    d_src = ctx.dev_alloc(img.nbytes); dsts = [ctx.dev_alloc(f.nbytes) for f in faces]
    try:
        ctx.upload(d_src, np.ascontiguousarray(img))
        # the set's projection and face fields are not read
        ctx.reproject_cube_dev(d_src, 67, 33, dsts, n, pf.reproject_params(projection=M.EQUIRECT, face=77, filter=flt, rot=rot))
        for d, f in zip(dsts, faces):
            ctx.download(f, d)
    finally:
        ctx.dev_free(d_src)
        for d in dsts:
            ctx.dev_free(d)
    for face in range(6):
        single = _reproject_dev(ctx, img, n, n, pf.reproject_params(projection=M.CUBE, face=face, filter=flt, rot=rot))
        assert np.array_equal(faces[face], single), M.FACE_NAMES[face]
        assert np.array_equal(single, M.reproject(img, n, n, M.CUBE, face, flt, rot=rot)), M.FACE_NAMES[face]


def test_refusals(pf, ctx):
    img = np.ascontiguousarray(reproject_cases.source_cached("64x32"))
    d_src, d_dst = ctx.dev_alloc(img.nbytes), ctx.dev_alloc(64 * 32 * 4)
    host_out = np.zeros((32, 64, 4), np.uint8)
    ok = pf.reproject_params(projection=M.EQUIRECT)
    byref = lambda p: C.byref(p) if p is not None else None

    def dev(src=d_src, cols=64, rows=32, dst=d_dst, out_cols=40, out_rows=20, p=ok):
        return ctx.l.pf_reproject_dev(ctx.h, C.c_void_p(src), cols, rows, C.c_void_p(dst), out_cols, out_rows, byref(p))

    def host(src=img, cols=64, rows=32, dst=host_out, out_cols=40, out_rows=20, p=ok, src_step=256, dst_step=256):
        sp = src.ctypes.data_as(C.c_void_p) if src is not None else None
        dp = dst.ctypes.data_as(C.c_void_p) if dst is not None else None
        return ctx.l.pf_reproject(ctx.h, sp, C.c_size_t(src_step), cols, rows, dp, C.c_size_t(dst_step), out_cols, out_rows, byref(p))

    def coords(**kw):
        fx = np.zeros((65, 65), np.int32); fy = np.zeros((65, 65), np.int32)
        a = dict(cols=64, rows=32, out_cols=40, out_rows=20, p=ok); a.update(kw)
        return ctx.l.pf_stage_reproject_coords(ctx.h, a["cols"], a["rows"], a["out_cols"], a["out_rows"], byref(a["p"]), fx.ctypes.data_as(C.c_void_p), fy.ctypes.data_as(C.c_void_p))

    def refused(rc, word):
        msg = ctx.l.pf_last_error(ctx.h).decode()
        assert rc == PF_ERR_ARG and word in msg, (rc, word, msg)

    def every(word, **bad):
        refused(dev(**bad), word); refused(host(**bad), word); refused(coords(**bad), word)

    try:
        ctx.upload(d_src, img)
        assert dev() == 0 and host() == 0 and coords() == 0
        refused(dev(src=None), "null"); refused(dev(dst=None), "null"); refused(host(src=None), "null"); refused(host(dst=None), "null")
        every("null", p=None)
        every("bad image size", cols=0); every("bad image size", rows=-1)
        every("bad output size", out_cols=0); every("bad output size", out_rows=-3)
        # a side above 65535; more than 2e9 pixels on either side (the pointers are never followed: the shape is refused first)
        every("above 65535", cols=65536, rows=2); every("above 65535", rows=65536, cols=2)
        every("above 65535", out_cols=65536, out_rows=2); every("above 65535", out_rows=70000, out_cols=2)
        every("too large", cols=50000, rows=50000); every("too large", out_cols=50000, out_rows=50000)
        every("unknown projection", p=pf.reproject_params(projection=3)); every("unknown projection", p=pf.reproject_params(projection=-1))
        for f in (0, 1, 4, -1):
            every("unknown filter", p=pf.reproject_params(projection=M.EQUIRECT, filter=f))
        for face in (-1, 6):
            every("unknown face", p=pf.reproject_params(projection=M.CUBE, face=face), out_cols=20)
        every("square", p=pf.reproject_params(projection=M.CUBE), out_cols=40, out_rows=20)
        for hfov in (0.0, 180.0, -10.0, 400.0, float("nan")):
            every("hfov", p=pf.reproject_params(projection=M.RECTILINEAR, hfov_deg=hfov))
        for k, v in ((0, float("nan")), (4, float("inf")), (8, float("-inf"))):
            rot = list(M.IDENTITY); rot[k] = v
            every("not finite", p=pf.reproject_params(projection=M.EQUIRECT, rot=rot))
        # a destination inside the source, and one that ends inside it
        refused(dev(dst=d_src), "overlaps"); refused(dev(dst=d_src + 64 * 31 * 4), "overlaps"); refused(dev(src=d_dst + 400, dst=d_dst), "overlaps")
        both = np.zeros((64, 64, 4), np.uint8)
        refused(host(src=both[:32], dst=both[16:]), "overlaps")
        assert host(src=both[:32], dst=both[32:]) == 0
        refused(host(src_step=255), "step"); refused(host(dst_step=159), "step")
        refused(ctx.l.pf_reproject_batch_dev(ctx.h, -1, None, 64, 32, None, 40, 20, C.byref(ok)), "bad argument")
        six = (C.c_void_p * 6)(*[C.c_void_p(d_dst)] * 6)
        refused(ctx.l.pf_reproject_cube_dev(ctx.h, None, 64, 32, six, 16, C.byref(ok)), "null")
        refused(ctx.l.pf_reproject_cube_dev(ctx.h, C.c_void_p(d_src), 64, 32, six, 0, C.byref(ok)), "bad output size")
        six = (C.c_void_p * 6)(*([C.c_void_p(d_dst)] * 5 + [C.c_void_p(d_src)]))
        refused(ctx.l.pf_reproject_cube_dev(ctx.h, C.c_void_p(d_src), 64, 32, six, 16, C.byref(ok)), "overlaps")
        assert dev() == 0
    finally:
        ctx.dev_free(d_src); ctx.dev_free(d_dst)


def _golden_pair():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stitch_240x200.npz"))
    return np.ascontiguousarray(g["L"]), np.ascontiguousarray(g["R"])


def test_resident_composite_of_a_lone_step(pf, ctx):
    L, R = _golden_pair()
    n = 50
    rot = M.rotation(37.0, -21.0, 11.0)
    face = np.empty((n, n, 4), np.uint8)
    c = pf.Context(0); plain = pf.Context(0)
    d = c.dev_alloc(face.nbytes)
    try:
        p = pf.reproject_params(projection=M.CUBE, face=M.LEFT, filter=M.BICUBIC, rot=rot)
        assert c.l.pf_stitch_result_reprojected_dev(c.h, n, n, C.byref(p), C.c_void_p(d)) == PF_ERR_ARG
        assert "no stitch step result" in c.l.pf_last_error(c.h).decode()
        out1 = c.stitch_step(L, R, PCT)
        c.stitch_result_reprojected_dev(n, n, p, d)
        want = M.reproject(out1, n, n, M.CUBE, M.LEFT, M.BICUBIC, rot=rot)
        assert np.array_equal(c.download(face, d), want), _differing(face, want)
        # the chain into the encoder is exact
        assert np.array_equal(png_decode_ref.decode(c.png_encode_dev(d, n, n)), want)
        # a levelled sphere at the composite's size
        rows, cols = out1.shape[:2]
        level = np.empty_like(out1)
        d2 = c.dev_alloc(level.nbytes)
        try:
            pe = pf.reproject_params(projection=M.EQUIRECT, filter=M.BILINEAR, rot=rot)
            c.stitch_result_reprojected_dev(cols, rows, pe, d2)
            assert np.array_equal(c.download(level, d2), M.reproject(out1, cols, rows, M.EQUIRECT, filter=M.BILINEAR, rot=rot))
        finally:
            c.dev_free(d2)
        # the reprojection changed nothing: a chained step gives what it gives without it
        out2 = c.stitch_step(L, None, PCT)
        ref1 = plain.stitch_step(L, R, PCT); ref2 = plain.stitch_step(L, None, PCT)
        assert np.array_equal(ref1, out1) and np.array_equal(ref2, out2)
        c.stitch_result_reprojected_dev(n, n, p, d)
        assert np.array_equal(c.download(face, d), M.reproject(ref2, n, n, M.CUBE, M.LEFT, M.BICUBIC, rot=rot))
    finally:
        c.dev_free(d); c.close(); plain.close()


def test_resident_composites_of_a_batch(pf, ctx):
    L, R = _golden_pair()
    Ls, Rs = [L, np.ascontiguousarray(L[:, ::-1])], [R, np.ascontiguousarray(R[:, ::-1])]
    w, h = 77, 43
    view = np.empty((h, w, 4), np.uint8)
    c = pf.Context(0)
    d = c.dev_alloc(view.nbytes)
    try:
        p = pf.reproject_params(projection=M.RECTILINEAR, filter=M.BILINEAR, hfov_deg=110.0, rot=M.rotation(-30.0, 10.0, 0.0))
        slot = lambda k: c.l.pf_stitch_batch_result_reprojected_dev(c.h, k, w, h, C.byref(p), C.c_void_p(d))
        assert slot(0) == PF_ERR_ARG and "no batch result" in c.l.pf_last_error(c.h).decode()
        outs = c.stitch_step_batch(Ls, Rs, PCT)
        for k in range(2):
            c.stitch_batch_result_reprojected_dev(k, w, h, p, d)
            want = M.reproject(outs[k], w, h, M.RECTILINEAR, filter=M.BILINEAR, hfov_deg=110.0, rot=M.rotation(-30.0, 10.0, 0.0))
            assert np.array_equal(c.download(view, d), want), _differing(view, want)
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
