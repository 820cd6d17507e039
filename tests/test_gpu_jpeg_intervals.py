"""The device JPEG encoder at the counts the product runs at and the geometry only the lab build reaches:
every kind of restart interval the coder admits (lab build, PANOFLOW_JPEG_RESTART: one MCU, a partial and a full second round of the
coder's threads), the compaction scan with more than one interval per thread (more than 1024 intervals), and the format's largest
side.  Everything is byte equality: with the serial model (tests/jpeg_model.py) where its Python loops are quick enough, with
libjpeg-turbo's own file through Pillow (which tests/test_jpeg_model.py holds the model to) for the large shapes."""
import re

import numpy as np
import pytest

import jpeg_cases
import jpeg_model as M

pytestmark = pytest.mark.gpu

VAR = "PANOFLOW_JPEG_RESTART"
INTERVAL_IMAGES = ("hostile_noise_q100", "marker_index_wraps", "ff_last_byte", "dummy_both")


@pytest.fixture(scope="module")
def ctx(pf):
    c = pf.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lab(pf):
    c = pf.Context(0, exp=True)
    yield c
    c.close()


def _first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return "%d and %d bytes, first difference at byte %d" % (len(got), len(want), k)


def _segments(data):
    """(marker, body) of every segment from SOI to SOS, and the entropy-coded data behind SOS without the EOI"""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    out, at = [], 2
    while True:
        assert data[at] == 0xFF
        marker, n = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        out.append((marker, data[at + 4:at + 2 + n]))
        at += 2 + n
        if marker == 0xDA:
            return out, data[at:-2]


def _dri(data):
    dri = [body for marker, body in _segments(data)[0] if marker == 0xDD]
    assert len(dri) == 1 and len(dri[0]) == 2
    return int.from_bytes(dri[0], "big")


def _restart_markers(data):
    """the RSTn markers of the entropy-coded data, in order (a 0xFF in the data itself has a stuffed 0x00 behind it)"""
    return [m[1] - 0xD0 for m in re.findall(b"\xff[\xd0-\xd7]", _segments(data)[1])]


# ---- A. every admitted restart interval: the lab build ----
@pytest.mark.parametrize("name", INTERVAL_IMAGES)
def test_lab_build_at_every_admitted_interval_equals_the_serial_model(pf, lab, monkeypatch, name):
    img = jpeg_cases.branch_cases()[name].img
    for sub in (0, 1):
        for q in (50, 100):
            for r in jpeg_cases.INTERVALS[sub]:
                monkeypatch.setenv(VAR, str(r))
                want = M.encode(img, q, sub, r)
                got = lab.jpeg_encode(img, pf.jpeg_params(quality=q, subsampling=sub))
                assert got == want, "subsampling %d quality %d interval %d: %s" % (sub, q, r, _first_difference(got, want))
                assert _dri(got) == r
                side = 16 if sub else 8
                n = -(-(-(-img.shape[0] // side) * -(-img.shape[1] // side)) // r)
                assert _restart_markers(got) == [k & 7 for k in range(n - 1)]


def test_an_interval_that_does_not_fit_leaves_the_products(pf, lab, ctx, monkeypatch):
    img = jpeg_cases.branch_cases()["marker_index_wraps"].img
    for sub in (0, 1):
        params = pf.jpeg_params(quality=50, subsampling=sub)
        want = M.encode(img, 50, sub)
        for value in (str(jpeg_cases.REFUSED_INTERVAL[sub]), "0", "-3", "65536", "many"):
            monkeypatch.setenv(VAR, value)
            got = lab.jpeg_encode(img, params)
            assert got == want and _dri(got) == M.RESTART[sub], "subsampling %d, %s=%s" % (sub, VAR, value)
        # the product library does not read the variable at all
        for value in ("1", str(jpeg_cases.INTERVALS[sub][-1])):
            monkeypatch.setenv(VAR, value)
            got = ctx.jpeg_encode(img, params)
            assert got == want and _dri(got) == M.RESTART[sub], "the product library, %s=%s" % (VAR, value)


# ---- C. more than 1024 intervals: k_jpeg_scan's threads sum two sizes each, most of them ----
@pytest.mark.parametrize("cols,rows,sub", [(2056, 2048, 0), (4112, 2048, 1)], ids=["444", "420"])
def test_1028_intervals_equal_libjpegs_file(pf, ctx, cols, rows, sub):
    """257 MCU columns, 1028 intervals of the product's length: they cross MCU rows at every phase"""
    img = jpeg_cases.patched(cols, rows, 41, (300, 900, 500, 1500))
    r = M.RESTART[sub]
    assert -(-len(range(0, cols, 16 if sub else 8)) * len(range(0, rows, 16 if sub else 8)) // r) == 1028
    want = jpeg_cases.pillow_file(img, 90, sub, r)
    got = ctx.jpeg_encode(img, pf.jpeg_params(quality=90, subsampling=sub))
    assert got == want, _first_difference(got, want)
    assert _dri(got) == r
    assert _restart_markers(got) == [k & 7 for k in range(1027)]
    assert len(got) <= pf.jpeg_bound(cols, rows, pf.jpeg_params(subsampling=sub))


def test_1056_intervals_of_one_mcu_equal_the_serial_model(pf, lab, monkeypatch):
    img = jpeg_cases.patched(528, 512, 42, (100, 300, 150, 400))
    monkeypatch.setenv(VAR, "1")
    want, info = M.encode(img, 90, 1, 1, want_info=True)
    assert info["intervals"] == 33 * 32 == 1056 and len(set(info["interval_bytes"])) > 20     # sizes from 31 to 245 bytes: a wrong offset moves bytes
    got = lab.jpeg_encode(img, pf.jpeg_params(quality=90, subsampling=1))
    assert got == want, _first_difference(got, want)
    assert _dri(got) == 1 and _restart_markers(got) == [k & 7 for k in range(1055)]


# ---- D. the largest side the format holds ----
@pytest.mark.parametrize("sub", [0, 1], ids=["444", "420"])
@pytest.mark.parametrize("across", [True, False], ids=["65535x9", "9x65535"])
def test_largest_side_equals_the_model_and_libjpegs_file(pf, ctx, across, sub):
    """65535 across: 256 tiles of k_jpeg_blocks, the last one of 255 pixels, and 8192 (4096) MCU columns, the last one a pixel short;
    down: 8192 (4096) MCU rows.  libjpeg itself writes no side above 65500 (Pillow refuses 65535), so the expected bytes at 65535 are
    the serial model's, and libjpeg's own file is the expected one for the same image cut to 65500, the longest it writes."""
    img = jpeg_cases.long_image(across)
    rows, cols = img.shape[:2]
    assert max(rows, cols) == 65535 and min(rows, cols) == 9
    params = pf.jpeg_params(quality=90, subsampling=sub)
    want = M.encode(img, 90, sub)
    got = ctx.jpeg_encode(img, params)
    assert got == want, _first_difference(got, want)
    assert _dri(got) == M.RESTART[sub]
    assert len(got) <= pf.jpeg_bound(cols, rows, params)
    cut = np.ascontiguousarray(img[:, :jpeg_cases.LIBJPEG_MAX_SIDE] if across else img[:jpeg_cases.LIBJPEG_MAX_SIDE])
    want = jpeg_cases.pillow_file(cut, 90, sub, M.RESTART[sub])
    got = ctx.jpeg_encode(cut, params)
    assert got == want, "cut to 65500: " + _first_difference(got, want)
