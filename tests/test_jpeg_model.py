"""CPU tier: the serial model of the device JPEG encoder (tests/jpeg_model.py) writes libjpeg's own file.  Every whole
file equals Pillow's (libjpeg-turbo) for the same image, quality, subsampling and restart interval, byte for byte; and every branch case
(tests/jpeg_cases.py) reaches, by the model's symbol trace, the branch it is named for."""
import io

import numpy as np
import pytest
from PIL import Image, features

import jpeg_cases
import jpeg_model as M

SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (9, 40), (40, 9), (25, 25), (75, 100)]


def pillow_file(img, quality, subsampling, restart):
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., [2, 1, 0]]), "RGB").save(buf, format="JPEG", quality=quality, subsampling=2 if subsampling else 0,
                                                                          restart_marker_blocks=restart)
    return buf.getvalue()


def test_pillow_is_libjpeg_turbo():
    assert features.check_feature("libjpeg_turbo")


@pytest.mark.parametrize("subsampling", [0, 1])
@pytest.mark.parametrize("kind", ["smooth", "noise"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_model_equals_pillow(size, kind, subsampling):
    assert features.check_feature("libjpeg_turbo")
    cols, rows = size
    img = jpeg_cases.smooth(cols, rows) if kind == "smooth" else jpeg_cases.noise(cols, rows, cols * 100 + rows)
    for quality in (1, 10, 50, 90, 100):
        for restart in (1, 5, M.RESTART[subsampling]):
            got = M.encode(img, quality, subsampling, restart)
            want = pillow_file(img, quality, subsampling, restart)
            assert got == want, "q %d R %d: %d and %d bytes" % (quality, restart, len(got), len(want))


@pytest.mark.parametrize("name", sorted(jpeg_cases.branch_cases()))
def test_branch_case_equals_pillow_and_reaches_its_branch(name):
    case = jpeg_cases.branch_cases()[name]
    data, info = M.encode(case.img, case.quality, case.subsampling, want_info=True)
    assert data == pillow_file(case.img, case.quality, case.subsampling, M.RESTART[case.subsampling])
    assert case.reached(info), {k: v for k, v in info.items() if k != "interval_bytes"}


def test_the_branch_list_is_whole():
    assert set(jpeg_cases.branch_cases()) >= set(jpeg_cases.BRANCHES)
