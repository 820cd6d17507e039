"""CPU tier: the serial model of the device JPEG encoder (tests/jpeg_model.py) writes libjpeg's own file.  Every whole
file equals Pillow's (libjpeg-turbo) for the same image, quality, subsampling and restart interval, byte for byte; and every branch case
(tests/jpeg_cases.py) reaches, by the model's symbol trace, the branch it is named for."""
import numpy as np
import pytest
from PIL import features

import jpeg_cases
import jpeg_model as M

SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (9, 40), (40, 9), (25, 25), (75, 100)]


pillow_file = jpeg_cases.pillow_file


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
        for restart in sorted({1, 5, M.RESTART[subsampling]} | set(jpeg_cases.INTERVALS[subsampling])):
            got = M.encode(img, quality, subsampling, restart)
            want = pillow_file(img, quality, subsampling, restart)
            assert got == want, "q %d R %d: %d and %d bytes" % (quality, restart, len(got), len(want))


@pytest.mark.parametrize("name", sorted(jpeg_cases.branch_cases()))
def test_branch_case_equals_pillow_and_reaches_its_branch(name):
    case = jpeg_cases.branch_cases()[name]
    data, info = M.encode(case.img, case.quality, case.subsampling, want_info=True)
    assert data == pillow_file(case.img, case.quality, case.subsampling, M.RESTART[case.subsampling])
    assert case.reached(info), {k: v for k, v in info.items() if not isinstance(v, list)}


@pytest.mark.parametrize("name", ["hostile_noise_q100", "marker_index_wraps", "ff_last_byte", "dummy_both"])
def test_interval_case_equals_pillow_at_every_admitted_interval(name):
    """the images the device tests run at every admitted interval (tests/test_gpu_jpeg_intervals.py), at those intervals"""
    case = jpeg_cases.branch_cases()[name]
    for subsampling in (0, 1):
        for restart in jpeg_cases.INTERVALS[subsampling]:
            assert M.encode(case.img, case.quality, subsampling, restart) == pillow_file(case.img, case.quality, subsampling, restart), (subsampling, restart)


@pytest.mark.parametrize("subsampling", [0, 1])
@pytest.mark.parametrize("across", [True, False], ids=["65500x9", "9x65500"])
def test_model_equals_pillow_at_the_longest_side_libjpeg_writes(across, subsampling):
    """the device tests take the model's file at 65535 a side, where libjpeg writes none (its limit is 65500): here the model is held to
    libjpeg's file for the same image cut to 65500"""
    img = jpeg_cases.long_image(across)
    cut = np.ascontiguousarray(img[:, :jpeg_cases.LIBJPEG_MAX_SIDE] if across else img[:jpeg_cases.LIBJPEG_MAX_SIDE])
    assert M.encode(cut, 90, subsampling) == pillow_file(cut, 90, subsampling, M.RESTART[subsampling])


def test_the_trace_gives_each_intervals_geometry():
    """the trace's bit counts, 0xFF offsets and code words, against the file itself"""
    case = jpeg_cases.branch_cases()["hostile_noise_q100"]
    data, info = M.encode(case.img, case.quality, case.subsampling, want_info=True)
    assert len(info["interval_bits"]) == len(info["ff_offsets"]) == len(info["word_starts"]) == len(info["word_lens"]) == info["intervals"] == 2
    for k in range(2):
        nbits, starts, lens = info["interval_bits"][k], info["word_starts"][k], info["word_lens"][k]
        assert starts[0] == 0 and (starts[1:] == starts[:-1] + lens[:-1]).all() and starts[-1] + lens[-1] == nbits
        assert lens.min() >= 2 and lens.max() <= 26
        marker = 2 if k == 0 else 0
        assert info["interval_bytes"][k] == (nbits + 7) // 8 + len(info["ff_offsets"][k]) + marker
    # the 0xFF offsets of the first interval, read back from the file: un-stuff the bytes between SOS and the first RST0
    scan = data[data.index(b"\xff\xda") + 14:]
    first = scan[:info["interval_bytes"][0] - 2]
    assert scan[len(first):len(first) + 2] == b"\xff\xd0"
    raw = first.replace(b"\xff\x00", b"\xff")
    assert np.array_equal(np.flatnonzero(np.frombuffer(raw, np.uint8) == 0xFF), info["ff_offsets"][0])


def test_the_branch_list_is_whole():
    assert set(jpeg_cases.branch_cases()) >= set(jpeg_cases.BRANCHES)
