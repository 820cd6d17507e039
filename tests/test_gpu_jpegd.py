"""The device JPEG decoder (pf_jpeg_probe, pf_jpeg_decode*): every case of tests/jpegd_cases.py decodes to Pillow's bytes; the stage
planes and entry states equal the serial model's (tests/jpegd_model.py) on the seam cases, at the product's subsequence size and, in the
lab build, at the smallest; batches, refusals, the round trip through the device encoder, large and extreme sizes, and the scratch of
other families surviving decode calls.  The only damaged scan sent to the GPU is a truncated one, whose walk ends at the segment's end;
the flipped and random scans stay with the host-run kernels (test_jpegd_kernels_host.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import jpeg_model
import jpegd_cases as jc
import jpegd_model as jm

pytestmark = pytest.mark.gpu

PF_ERR_ARG = -1


@pytest.fixture(scope="module")
def ctx(pf):
    c = pf.Context(0)
    yield c
    c.close()


def _dev(ctx, data, cols, rows):
    p = ctx.dev_alloc(cols * rows * 4)
    try:
        ctx.upload(p, np.full((rows, cols, 4), 0xEE, np.uint8))
        ctx.jpeg_decode_dev(data, cols, rows, p)
        return ctx.download(np.empty((rows, cols, 4), np.uint8), p)
    finally:
        ctx.dev_free(p)


def test_every_case_gives_pillows_bytes(pf, ctx):
    wrong = []
    cases = jc.all_valid_cases()
    assert len(cases) > 90
    for name, data in cases:
        info = pf.jpeg_probe(data)
        assert info.device_decodable == 1, (name, info.reason)
        want = jc.pillow_bgra(data)
        assert (info.rows, info.cols) == want.shape[:2]
        got = _dev(ctx, data, info.cols, info.rows)
        if not np.array_equal(got, want):
            wrong.append((name, int((got != want).sum())))
    assert not wrong, "cases whose bytes are not Pillow's (name, bytes that differ): %s" % wrong


def test_host_form_leaves_the_row_padding_alone(ctx):
    data = jc.pil_jpeg(jc.scene(37, 21, 3), 85, "420")
    want = jc.pillow_bgra(data)
    step = 37 * 4 + 12
    out = np.full((21, step), 0xEE, np.uint8)
    got = ctx.jpeg_decode(data, (21, 37), out=out, row_step=step)
    assert np.array_equal(got, want) and (out[:, 37 * 4:] == 0xEE).all()
    assert np.array_equal(ctx.jpeg_decode(data), want)


def _stage_equals_model(ctx, name, data, S):
    m = jm.decode(data)
    info = m["info"]
    nsub = jm.n_subsequences(info, S)
    states, coef, planes, counts = ctx.stage_jpeg_decode(data, nsub, m["coef"].shape[0], sum(p.size for p in m["planes"]))
    assert counts[0] == nsub and counts[3] == S, name
    assert np.array_equal(coef, m["coef"]), name
    assert np.array_equal(planes, np.concatenate([p.reshape(-1) for p in m["planes"]])), name
    want = jm.entry_states(m, S)
    have = states[:-1]
    assert np.array_equal(have[:, 0], want[:, 0]) and np.array_equal(have[:, 1] & 0xff, want[:, 1]) and np.array_equal(have[:, 1] >> 8, want[:, 2]), name
    return counts


def test_stage_planes_and_entry_states_equal_the_models_on_the_seams(ctx):
    counts = {}
    for name, S, data in jc.seam_cases():
        counts[name] = _stage_equals_model(ctx, name, data, jc.S_PRODUCT)
    assert counts["more_than_lanes-S%d" % jc.S_PRODUCT][2] >= 2      # launches: the state crossed a workgroup
    assert counts["word_split-S%d" % jc.S_PRODUCT][1] > 1
    for name, data in jc.model_only_cases():          # (the hand-made long blocks: held to the model, pixels included)
        c = _stage_equals_model(ctx, name, data, jc.S_PRODUCT)
        assert c[1] > 1, name
        m = jm.decode(data)
        assert np.array_equal(_dev(ctx, data, m["info"]["cols"], m["info"]["rows"]), jm.bgra(m["rgb"])), name


def test_the_lab_build_at_the_smallest_subsequence_size(pf):
    old = os.environ.get("PANOFLOW_JPEGD_SUBSEQ")
    os.environ["PANOFLOW_JPEGD_SUBSEQ"] = str(jc.S_MIN)
    lab = pf.Context(0, exp=True)
    try:
        counts = {}
        for name, S, data in jc.seam_cases():
            counts[name] = _stage_equals_model(lab, name, data, jc.S_MIN)
            assert np.array_equal(lab.jpeg_decode(data), jc.pillow_bgra(data)), name
        assert counts["more_than_lanes-S%d" % jc.S_MIN][2] >= 2
        assert counts["no_block_completes-S%d" % jc.S_MIN][1] > 1
    finally:
        lab.close()
        if old is None:
            del os.environ["PANOFLOW_JPEGD_SUBSEQ"]
        else:
            os.environ["PANOFLOW_JPEGD_SUBSEQ"] = old


def _batch_files():
    """17 files of 75 x 43 with mixed subsampling, tables and intervals"""
    out = []
    for k in range(17):
        img = jc.scene(75, 43, 100 + k) if k % 3 else jc.noise(75, 43, 100 + k)
        sub = ("444", "422", "420", "grey")[k % 4]
        out.append(jc.pil_jpeg(img, (30, 75, 95)[k % 3], sub if sub != "grey" else "444", bool(k & 1), (0, 1, 4, 5)[(k // 2) % 4], grey=sub == "grey"))
    return out


def test_a_batch_of_seventeen_mixed_files(ctx):
    files = _batch_files()
    ptrs = [ctx.dev_alloc(75 * 43 * 4) for _ in files]
    try:
        ctx.jpeg_decode_batch_dev(files, 75, 43, ptrs)
        for k, (d, p) in enumerate(zip(files, ptrs)):
            got = ctx.download(np.empty((43, 75, 4), np.uint8), p)
            assert np.array_equal(got, jc.pillow_bgra(d)), k
    finally:
        for p in ptrs:
            ctx.dev_free(p)


def test_a_cut_file_fails_the_batch_names_it_and_zeroes_the_outputs(pf, ctx):
    files = _batch_files()
    info = jm.parse(files[5])
    cut = files[5][:info["begin"] + (info["end"] - info["begin"]) // 2] + b"\xff\xd9"
    m = jm.decode(cut)
    assert not m["accept"]
    files[5] = cut
    ptrs = [ctx.dev_alloc(75 * 43 * 4) for _ in files]
    try:
        for p in ptrs:
            ctx.upload(p, np.full((43, 75, 4), 0xEE, np.uint8))
        with pytest.raises(pf.PanoflowError) as e:
            ctx.jpeg_decode_batch_dev(files, 75, 43, ptrs)
        assert "file 5" in str(e.value) and "MCU %d " % m["event_mcu"] in str(e.value)
        for p in ptrs:
            assert not ctx.download(np.empty((43, 75, 4), np.uint8), p).any()
    finally:
        for p in ptrs:
            ctx.dev_free(p)


def test_host_form_writes_nothing_for_a_damaged_scan(pf, ctx):
    data = jc.pil_jpeg(jc.scene(75, 43, 3), 85, "420", False, 2)
    info = jm.parse(data)
    cut = data[:info["begin"] + (info["end"] - info["begin"]) // 3] + b"\xff\xd9"
    m = jm.decode(cut)
    assert not m["accept"]
    out = np.full((43, 75 * 4 + 8), 0xEE, np.uint8)
    with pytest.raises(pf.PanoflowError) as e:
        ctx.jpeg_decode(cut, (43, 75), out=out, row_step=75 * 4 + 8)
    assert "file 0" in str(e.value) and "MCU %d " % m["event_mcu"] in str(e.value)
    assert (out == 0xEE).all()


@pytest.mark.parametrize("name", sorted(jc.refusals()))
def test_refusals_come_with_their_reason_before_any_work(pf, ctx, name):
    data, word = jc.refusals()[name]
    with pytest.raises(jm.Refused) as e:
        jm.parse(data)
    assert word in str(e.value)
    info = pf.jpeg_probe(data)
    assert info.device_decodable == 0 and word in info.reason.decode()
    p = ctx.dev_alloc(32 * 24 * 4)
    try:
        ctx.upload(p, np.full((24, 32, 4), 0xEE, np.uint8))
        with pytest.raises(pf.PanoflowError) as e:
            ctx.jpeg_decode_dev(data, 32, 24, p)
        assert word in str(e.value)
        assert (ctx.download(np.empty((24, 32, 4), np.uint8), p) == 0xEE).all()       # nothing was written
    finally:
        ctx.dev_free(p)


def test_argument_refusals(pf, ctx):
    data = jc.pil_jpeg(jc.scene(32, 24, 1), 80, "420")
    buf = np.frombuffer(data, np.uint8)
    p = ctx.dev_alloc(2 * 32 * 24 * 4)
    try:
        call = lambda f, n, c, r, d: ctx.l.pf_jpeg_decode_dev(ctx.h, f, C.c_size_t(n), c, r, C.c_void_p(d))
        assert call(buf.ctypes.data_as(C.c_void_p), buf.size, 32, 24, p) == 0
        assert call(None, buf.size, 32, 24, p) == PF_ERR_ARG
        assert call(buf.ctypes.data_as(C.c_void_p), buf.size, 32, 24, None) == PF_ERR_ARG
        assert call(buf.ctypes.data_as(C.c_void_p), buf.size, 32, 24, p + 2) == PF_ERR_ARG and b"aligned" in ctx.l.pf_last_error(ctx.h)
        assert call(buf.ctypes.data_as(C.c_void_p), buf.size, 24, 32, p) == PF_ERR_ARG and b"expects" in ctx.l.pf_last_error(ctx.h)
        with pytest.raises(pf.PanoflowError) as e:
            ctx.jpeg_decode_batch_dev([data, data], 32, 24, [p, p + 32 * 24 * 4 - 4])
        assert "overlaps" in str(e.value)
        with pytest.raises(pf.PanoflowError):
            pf.jpeg_probe(b"II*\0 not a jpeg")
    finally:
        ctx.dev_free(p)


@pytest.mark.parametrize("sub", [0, 1])
def test_round_trip_through_the_device_encoder(pf, ctx, sub):
    img = jm.bgra(jc.scene(203, 131, 7))
    data = ctx.jpeg_encode(img, pf.jpeg_params(quality=90, subsampling=sub))
    assert np.array_equal(_dev(ctx, data, 203, 131), jc.pillow_bgra(data))


@pytest.mark.parametrize("sub", ["444", "422", "420"])
@pytest.mark.parametrize("rows_per_interval", [0, 1])
def test_a_large_image_crosses_workgroups_and_launches(ctx, sub, rows_per_interval):
    img = jc.scene(2048, 1536, 11)
    data = jc.pil_jpeg(img, 90, sub, False, jc._mcu_row(2048, sub) * rows_per_interval)
    info = jm.parse(data)
    assert (info["end"] - info["begin"]) > 4 * jc.LANES * jc.S_PRODUCT
    got = _dev(ctx, data, 2048, 1536)
    want = jc.pillow_bgra(data)
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())


@pytest.mark.parametrize("shape", [(65500, 8), (8, 65500)])
def test_extreme_sides_against_pillow(ctx, shape):
    w, h = shape
    data = jc.pil_jpeg(jc.ramp(w, h, 5), 80, "420")
    assert np.array_equal(_dev(ctx, data, w, h), jc.pillow_bgra(data))


@pytest.mark.parametrize("shape", [(65535, 9), (9, 65535)])
def test_the_largest_sides_against_the_model(ctx, shape):
    w, h = shape
    data = jpeg_model.encode(jm.bgra(jc.ramp(w, h, 9)), 75, 1)
    m = jm.decode(data)
    assert m["accept"]
    assert np.array_equal(_dev(ctx, data, w, h), jm.bgra(m["rgb"]))


def test_the_reprojections_and_the_lens_scratch_and_a_resident_composite_survive(pf):
    import lens_cases
    import lens_model as M
    import reproject_model as R
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stitch_240x200.npz"))
    L, Rimg = np.ascontiguousarray(g["L"]), np.ascontiguousarray(g["R"])
    n = 50
    rot = R.rotation(37.0, -21.0, 11.0)
    face = np.empty((n, n, 4), np.uint8)
    case = next(c for c in lens_cases.cases() if c.photo == "33x67" and c.lens.filter == M.BICUBIC and c.lens.model == M.EQUISOLID)
    m = case.lens
    lens = pf.lens(m.model, filter=m.filter, rot=m.rot, focal_px=m.focal_px, a=m.a, b=m.b, c=m.c, dd=m.dd, shift_x=m.shift_x, shift_y=m.shift_y, min_cos=m.min_cos,
                   crop_cx256=m.crop[0], crop_cy256=m.crop[1], crop_r256=m.crop[2])
    photo = lens_cases.photo_cached(case.photo)
    files = [jc.pil_jpeg(jc.scene(n, n, 21), 90, "420"), jc.pil_jpeg(jc.scene(240, 200, 22), 85, "422", False, 3)]
    c = pf.Context(0); plain = pf.Context(0)
    d = c.dev_alloc(face.nbytes)
    try:
        p = pf.reproject_params(projection=R.EQUIRECT, filter=R.BICUBIC, rot=rot)
        out1 = c.stitch_step(L, Rimg, 20)
        c.stitch_result_reprojected_dev(n, n, p, d)
        before = c.download(face, d).copy()
        remapped = c.lens_remap(photo, case.cols, case.rows, lens)
        # decodes in between, at the reprojection's output size and at the composite's: host form and the stage hook
        for data in files:
            assert np.array_equal(c.jpeg_decode(data), jc.pillow_bgra(data))
            mm = jm.decode(data)
            c.stage_jpeg_decode(data, jm.n_subsequences(mm["info"], jc.S_PRODUCT), mm["coef"].shape[0], sum(q.size for q in mm["planes"]))
        c.stitch_result_reprojected_dev(n, n, p, d)
        assert np.array_equal(c.download(face, d), before)
        assert np.array_equal(c.lens_remap(photo, case.cols, case.rows, lens), remapped)
        # the chain goes on as if nothing had happened
        out2 = c.stitch_step(L, None, 20)
        ref1 = plain.stitch_step(L, Rimg, 20); ref2 = plain.stitch_step(L, None, 20)
        assert np.array_equal(ref1, out1) and np.array_equal(ref2, out2)
    finally:
        c.dev_free(d); c.close(); plain.close()
