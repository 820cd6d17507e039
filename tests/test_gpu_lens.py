"""The device lens remap (pf_lens_remap_dev, pf_lens_remap, pf_lens_remap_batch_dev, pf_stage_lens_coords): the bytes and the quantised
coordinates are the function of the photo, the sizes and the lens that DESIGN.md 8.7 specifies, which tests/lens_model.py computes
(and tests/test_lens_model.py holds to libm and to the reprojection's conventions); everything the device gives is compared with the
model's for equality, on the case list the host-run kernel runs (tests/lens_cases.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import lens_cases
import lens_model as M
import reproject_model as R

pytestmark = pytest.mark.gpu

PF_ERR_ARG = -1
PCT = 20


@pytest.fixture(scope="module")
def ctx(pf):
    c = pf.Context(0)
    yield c
    c.close()


def _lens(pf, m):
    """the library's pf_lens of a model Lens"""
    return pf.lens(m.model, filter=m.filter, rot=m.rot, focal_px=m.focal_px, a=m.a, b=m.b, c=m.c, dd=m.dd, shift_x=m.shift_x, shift_y=m.shift_y, min_cos=m.min_cos,
                   crop_cx256=m.crop[0], crop_cy256=m.crop[1], crop_r256=m.crop[2])


def _differing(got, want):
    return "%d of %d differ" % (int((got != want).sum()), want.size)


def test_the_librarys_helpers_are_the_models(pf):
    for model in range(4):
        for cols, hfov in ((64, 120.0), (6000, 95.5), (65535, 60.0)):
            assert pf.lens_focal(model, cols, hfov) == M.focal(model, cols, hfov)
        p = pf.lens(model)
        assert (p.filter, p.focal_px, p.a, p.b, p.c, p.dd, p.shift_x, p.shift_y, p.crop_r256) == (M.BICUBIC, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0)
        assert p.min_cos == (0.0 if model == M.RECTILINEAR else -0.5) and list(p.rot) == R.IDENTITY
    assert pf.lens_focal(7, 64, 90.0) == 0.0
    assert pf.lens_rotation(37.0, -21.0, 11.0) == M.rotation(37.0, -21.0, 11.0)
    rp = pf.reproject_rotation(37.0, -21.0, 11.0)
    assert pf.lens_rotation(37.0, -21.0, 11.0) == [rp[3 * j + i] for i in range(3) for j in range(3)]


@pytest.mark.parametrize("canvas", lens_cases.CANVASES, ids=lambda c: "%dx%d" % c)
@pytest.mark.parametrize("photo", lens_cases.PHOTOS)
def test_cases_host_form_device_form_and_coordinates(pf, ctx, photo, canvas):
    img = lens_cases.photo_cached(photo)
    rows, cols = img.shape[:2]
    w, h = canvas
    padded = np.full((rows, cols + 3, 4), 0xEE, np.uint8); padded[:, :cols] = img   # row steps wider than the rows, on both sides
    host_out = np.empty((h, w + 5, 4), np.uint8)
    out = np.empty((h, w, 4), np.uint8)
    d_src, d_dst = ctx.dev_alloc(img.nbytes), ctx.dev_alloc(out.nbytes)
    bad, ran, done = [], 0, set()
    try:
        ctx.upload(d_src, np.ascontiguousarray(img))
        for case in lens_cases.cases():
            if case.photo != photo or (case.cols, case.rows) != canvas:
                continue
            ran += 1
            p = _lens(pf, case.lens)
            if case.key not in done:   # the coordinates do not depend on the filter: once per geometry
                done.add(case.key)
                fx, fy = ctx.stage_lens_coords(cols, rows, w, h, p)
                mfx, mfy = lens_cases.model_coords(case)
                if not (np.array_equal(fx, mfx) and np.array_equal(fy, mfy)):
                    bad.append("%s coordinates: fx %s, fy %s" % (case.name, _differing(fx, mfx), _differing(fy, mfy)))
            want = lens_cases.model_image(case)
            host_out[:] = 0xA5
            ctx.lens_remap(padded[:, :cols], w, h, p, out=host_out[:, :w])
            if not np.array_equal(host_out[:, :w], want):
                bad.append("%s host form: %s" % (case.name, _differing(host_out[:, :w], want)))
            if not (host_out[:, w:] == 0xA5).all():
                bad.append("%s host form: the bytes behind the canvas's rows were written" % case.name)
            ctx.lens_remap_dev(d_src, cols, rows, d_dst, w, h, p)
            ctx.download(out, d_dst)
            if not np.array_equal(out, want):
                bad.append("%s device form: %s" % (case.name, _differing(out, want)))
    finally:
        ctx.dev_free(d_src); ctx.dev_free(d_dst)
    assert ran > 50
    assert not bad, "%d mismatches: %s" % (len(bad), bad[:10])


@pytest.mark.parametrize("k", range(2), ids=["equidistant", "rectilinear"])
def test_ringing_photo_clamps_in_every_channel(pf, ctx, k):
    case = lens_cases.ringing_cases()[k]
    low, high = lens_cases.clamp_counts(case)   # a condition on the inputs, on the model alone
    assert min(low + high) >= lens_cases.RINGING_MIN_CLAMPED, (low, high)
    img = lens_cases.photo_cached(case.photo)
    want = lens_cases.model_image(case)
    got = ctx.lens_remap(img, case.cols, case.rows, _lens(pf, case.lens))
    assert np.array_equal(got, want), "host form: " + _differing(got, want)
    out = np.empty_like(want)
    d_src, d_dst = ctx.dev_alloc(img.nbytes), ctx.dev_alloc(out.nbytes)
    try:
        ctx.upload(d_src, np.ascontiguousarray(img))
        ctx.lens_remap_dev(d_src, img.shape[1], img.shape[0], d_dst, case.cols, case.rows, _lens(pf, case.lens))
        ctx.download(out, d_dst)
    finally:
        ctx.dev_free(d_src); ctx.dev_free(d_dst)
    assert np.array_equal(out, want), "device form: " + _differing(out, want)


def _batch(ctx, pf, img, w, h, cases):
    outs = [np.empty((h, w, 4), np.uint8) for _ in cases]
    rows, cols = img.shape[:2]
    # every image its own photo too: the case's photo rolled by its index
    imgs = [np.ascontiguousarray(np.roll(img, 3 * k, axis=1)) for k in range(len(cases))]
    srcs = [ctx.dev_alloc(im.nbytes) for im in imgs]; dsts = [ctx.dev_alloc(o.nbytes) for o in outs]
    try:
        for d, im in zip(srcs, imgs):
            ctx.upload(d, im)
        ctx.lens_remap_batch_dev(srcs, cols, rows, dsts, w, h, [_lens(pf, c.lens) for c in cases])
        for d, o in zip(dsts, outs):
            ctx.download(o, d)
    finally:
        for d in srcs + dsts:
            ctx.dev_free(d)
    return imgs, outs


@pytest.mark.parametrize("mixed", [False, True], ids=["one_filter", "both_filters"])
def test_batch_of_17_each_image_under_its_own_lens(pf, ctx, mixed):
    w, h = 130, 65
    mine = [c for c in lens_cases.cases() if c.photo == "33x67" and (c.cols, c.rows) == (w, h) and (mixed or c.lens.filter == M.BICUBIC)]
    picked, keys = [], set()
    for c in mine[::len(mine) // 18]:   # 17 different geometries spread over the list, every lens model among them
        if c.key not in keys and len(picked) < 17:
            keys.add(c.key); picked.append(c)
    assert len(picked) == 17 and {c.lens.model for c in picked} == {0, 1, 2, 3}
    assert {c.lens.filter for c in picked} == ({M.BILINEAR, M.BICUBIC} if mixed else {M.BICUBIC})
    img = lens_cases.photo_cached("33x67")
    ctx.profile_enable(1); ctx.profile_reset()
    try:
        imgs, outs = _batch(ctx, pf, img, w, h, picked)
        prof = ctx.profile()
    finally:
        ctx.profile_enable(0)
    if not mixed:
        assert prof["lens"][1] == 2   # 16 images and 1: two launch groups, one drain
    for k, c in enumerate(picked):
        want = M.remap(imgs[k], w, h, c.lens)
        assert np.array_equal(outs[k], want), (k, c.name, _differing(outs[k], want))
    assert not np.array_equal(outs[0], outs[16])


def test_refusals(pf, ctx):
    img = np.ascontiguousarray(lens_cases.photo_cached("64x48"))
    d_src, d_dst = ctx.dev_alloc(img.nbytes), ctx.dev_alloc(64 * 32 * 4)
    host_out = np.zeros((32, 64, 4), np.uint8)
    ok = pf.lens(M.EQUIDISTANT, focal_px=30.0)
    byref = lambda p: C.byref(p) if p is not None else None

    def dev(src=d_src, pc=64, pr=48, dst=d_dst, cols=40, rows=20, p=ok):
        return ctx.l.pf_lens_remap_dev(ctx.h, C.c_void_p(src), pc, pr, C.c_void_p(dst), cols, rows, byref(p))

    def host(src=img, pc=64, pr=48, dst=host_out, cols=40, rows=20, p=ok, src_step=256, dst_step=256):
        sp = src.ctypes.data_as(C.c_void_p) if src is not None else None
        dp = dst.ctypes.data_as(C.c_void_p) if dst is not None else None
        return ctx.l.pf_lens_remap(ctx.h, sp, C.c_size_t(src_step), pc, pr, dp, C.c_size_t(dst_step), cols, rows, byref(p))

    def batch(src=d_src, pc=64, pr=48, dst=d_dst, cols=40, rows=20, p=ok):
        one = lambda v: (C.c_void_p * 1)(C.c_void_p(v))
        return ctx.l.pf_lens_remap_batch_dev(ctx.h, 1, one(src), pc, pr, one(dst), cols, rows, byref(p))

    def coords(**kw):
        fx = np.zeros((65, 65), np.int32); fy = np.zeros((65, 65), np.int32)
        a = dict(pc=64, pr=48, cols=40, rows=20, p=ok); a.update(kw)
        return ctx.l.pf_stage_lens_coords(ctx.h, a["pc"], a["pr"], a["cols"], a["rows"], byref(a["p"]), fx.ctypes.data_as(C.c_void_p), fy.ctypes.data_as(C.c_void_p))

    def refused(rc, word):
        msg = ctx.l.pf_last_error(ctx.h).decode()
        assert rc == PF_ERR_ARG and word in msg, (rc, word, msg)

    def every(word, **bad):
        refused(dev(**bad), word); refused(host(**bad), word); refused(batch(**bad), word); refused(coords(**bad), word)

    try:
        ctx.upload(d_src, img)
        assert dev() == 0 and host() == 0 and batch() == 0 and coords() == 0
        refused(dev(src=None), "null"); refused(dev(dst=None), "null"); refused(host(src=None), "null"); refused(host(dst=None), "null")
        refused(batch(src=None), "null"); refused(batch(dst=None), "null")
        refused(ctx.l.pf_stage_lens_coords(ctx.h, 64, 48, 40, 20, C.byref(ok), None, None), "null")
        refused(ctx.l.pf_lens_remap_batch_dev(ctx.h, -1, None, 64, 48, None, 40, 20, C.byref(ok)), "bad argument")
        every("null", p=None)
        every("bad image size", pc=0); every("bad image size", pr=-1)
        every("bad canvas size", cols=0); every("bad canvas size", rows=-3)
        # a side above 65535; more than 2e9 pixels on either side (the pointers are never followed: the shape is refused first)
        every("above 65535", pc=65536, pr=2); every("above 65535", pr=65536, pc=2)
        every("above 65535", cols=65536, rows=2); every("above 65535", rows=70000, cols=2)
        every("too large", pc=50000, pr=50000); every("too large", cols=50000, rows=50000)
        every("unknown model", p=pf.lens(4, focal_px=30.0)); every("unknown model", p=pf.lens(-1, focal_px=30.0))
        for f in (0, 1, 4, -1):
            every("unknown filter", p=pf.lens(M.EQUIDISTANT, focal_px=30.0, filter=f))
        for name in ("focal_px", "a", "b", "c", "dd", "shift_x", "shift_y", "min_cos"):
            for v in (float("nan"), float("inf"), float("-inf")):
                fields = {"focal_px": 30.0}; fields[name] = v
                every("%s is not finite" % name, p=pf.lens(M.EQUIDISTANT, **fields))
        for k, v in ((0, float("nan")), (4, float("inf")), (8, float("-inf"))):
            rot = list(R.IDENTITY); rot[k] = v
            every("rot[%d] is not finite" % k, p=pf.lens(M.EQUIDISTANT, focal_px=30.0, rot=rot))
        every("not positive", p=pf.lens(M.EQUIDISTANT)); every("not positive", p=pf.lens(M.EQUIDISTANT, focal_px=-30.0))
        for m in (1.0, 1.5, -1.000001):
            every("min_cos", p=pf.lens(M.EQUISOLID, focal_px=30.0, min_cos=m))
        every("rectilinear", p=pf.lens(M.RECTILINEAR, focal_px=30.0, min_cos=-0.25))
        assert dev(p=pf.lens(M.STEREOGRAPHIC, focal_px=30.0, min_cos=-1.0)) == 0
        every("crop_r256", p=pf.lens(M.EQUIDISTANT, focal_px=30.0, crop_r256=-1))
        # a canvas inside the photo, and one that ends inside it
        for call in (dev, batch):
            refused(call(dst=d_src), "overlaps"); refused(call(dst=d_src + 64 * 47 * 4), "overlaps"); refused(call(src=d_dst + 400, dst=d_dst), "overlaps")
            refused(call(src=d_src + 2), "aligned"); refused(call(dst=d_dst + 1), "aligned")
        both = np.zeros((96, 64, 4), np.uint8)
        refused(host(src=both[:48], dst=both[24:]), "overlaps")
        assert host(src=both[:48], dst=both[48:]) == 0
        refused(host(src_step=255), "step"); refused(host(dst_step=159), "step")
        assert dev() == 0
    finally:
        ctx.dev_free(d_src); ctx.dev_free(d_dst)


def test_the_reprojections_scratch_and_a_resident_composite_survive(pf):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stitch_240x200.npz"))
    L, Rimg = np.ascontiguousarray(g["L"]), np.ascontiguousarray(g["R"])
    n = 50
    rot = R.rotation(37.0, -21.0, 11.0)
    face = np.empty((n, n, 4), np.uint8)
    case = next(c for c in lens_cases.cases() if c.photo == "33x67" and c.lens.filter == M.BICUBIC and c.lens.model == M.EQUISOLID)
    c = pf.Context(0); plain = pf.Context(0)
    d = c.dev_alloc(face.nbytes)
    try:
        p = pf.reproject_params(projection=R.EQUIRECT, filter=R.BICUBIC, rot=rot)   # (both of the reprojection's tables become resident)
        out1 = c.stitch_step(L, Rimg, PCT)
        c.stitch_result_reprojected_dev(n, n, p, d)
        before = c.download(face, d).copy()
        assert np.array_equal(before, R.reproject(out1, n, n, R.EQUIRECT, filter=R.BICUBIC, rot=rot))
        # remaps in between, at the reprojection's output size and at another: host form, device form, coordinates
        photo = lens_cases.photo_cached(case.photo)
        for (w, h) in ((n, n), (case.cols, case.rows)):
            got = c.lens_remap(photo, w, h, _lens(pf, case.lens))
            assert np.array_equal(got, M.remap(photo, w, h, case.lens))
            c.stage_lens_coords(photo.shape[1], photo.shape[0], w, h, _lens(pf, case.lens))
        c.stitch_result_reprojected_dev(n, n, p, d)
        assert np.array_equal(c.download(face, d), before)
        # the chain goes on as if nothing had happened
        out2 = c.stitch_step(L, None, PCT)
        ref1 = plain.stitch_step(L, Rimg, PCT); ref2 = plain.stitch_step(L, None, PCT)
        assert np.array_equal(ref1, out1) and np.array_equal(ref2, out2)
    finally:
        c.dev_free(d); c.close(); plain.close()
