"""CPU tier of the device PNG encoder's tests: the strict reader the GPU tests judge by (tests/png_decode_ref.py) against hand-built
files, and the GPU tests' images against what they are named for -- both from numpy and stdlib zlib alone."""
import os
import zlib

import numpy as np
import pytest

import png_cases
import png_decode_ref as R


def _image(cols, rows, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 4), dtype=np.uint8)


@pytest.mark.parametrize("ftype", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("cols,rows", [(1, 1), (1, 4), (5, 1), (9, 7)])
def test_round_trip_each_filter(ftype, cols, rows):
    img = _image(cols, rows, 10 * ftype + cols)
    data = R.frame(cols, rows, zlib.compress(R.filter_rows(img, [ftype] * rows)))
    got, types = R.decode(data, want_types=True)
    assert np.array_equal(got, img) and list(types) == [ftype] * rows


def test_round_trip_mixed_filters_and_split_idat():
    img = _image(13, 10, 5)
    types = [0, 1, 2, 3, 4, 4, 3, 2, 1, 0]
    z = zlib.compress(R.filter_rows(img, types), 9)
    for idat_max in (None, 7, 1):
        got, t = R.decode(R.frame(13, 10, z, idat_max), want_types=True)
        assert np.array_equal(got, img) and list(t) == types


def _good():
    img = _image(6, 5, 3)
    return bytearray(R.frame(6, 5, zlib.compress(R.filter_rows(img, [4] * 5))))


def test_refuses_flipped_crc_bit_in_every_chunk():
    good = _good()
    R.decode(good)
    pos = 8
    while pos < len(good):
        n = int.from_bytes(good[pos:pos + 4], "big")
        for at in (pos + 8 + n, pos + 4):          # the CRC itself, and a byte the CRC covers
            bad = bytearray(good); bad[at] ^= 0x10
            with pytest.raises(R.PngError):
                R.decode(bad)
        pos += 12 + n


def test_refuses_truncated_stream_and_bad_fields():
    good = _good()
    for cut in (1, 4, 12, 13, 20):
        with pytest.raises(R.PngError):
            R.decode(good[:-cut])
    img = _image(6, 5, 3)
    raw = R.filter_rows(img, [0] * 5)
    z = zlib.compress(raw)
    with pytest.raises(R.PngError):                # deflate data cut short, chunk CRCs right
        R.decode(R.frame(6, 5, z[:-9]))
    with pytest.raises(R.PngError):                # wrong Adler-32
        R.decode(R.frame(6, 5, z[:-1] + bytes([z[-1] ^ 1])))
    with pytest.raises(R.PngError):                # bytes after the zlib stream
        R.decode(R.frame(6, 5, z + b"\0"))
    with pytest.raises(R.PngError):                # a row short
        R.decode(R.frame(6, 6, z))
    with pytest.raises(R.PngError):                # filter type 5
        R.decode(R.frame(6, 5, zlib.compress(bytes([5]) + raw[1:])))
    with pytest.raises(R.PngError):
        R.decode(good + b"\0")                     # bytes after IEND
    bad = bytearray(good); bad[0] = 0x88
    with pytest.raises(R.PngError):
        R.decode(bad)


# ---- the GPU tests' images are what they are named for ----
def test_noise_image_does_not_compress():
    img = png_cases.noise(300, 200, 1)
    for types in ([0] * 200, [2] * 200):
        raw = R.filter_rows(img, types)
        assert len(zlib.compress(raw, 9)) >= 0.99 * len(raw)


def test_constant_images_are_one_run():
    for bgra in ((0, 0, 0, 0), (7, 7, 7, 255)):
        img = png_cases.constant(300, 200, bgra)
        assert (img.reshape(-1, 4) == img[0, 0]).all()


def _filter_sums(img):
    """per row and filter type: the sum of absolute residuals, residual bytes read as signed"""
    rows = img.shape[0]
    out = np.zeros((rows, 5), np.int64)
    for f in range(5):
        res = np.frombuffer(R.filter_rows(img, [f] * rows), np.uint8).reshape(rows, -1)[:, 1:].astype(np.int64)
        out[:, f] = np.where(res < 128, res, 256 - res).sum(1)
    return out


def test_ramp_images_leave_one_filter_the_smallest_sum():
    s = _filter_sums(png_cases.ramp_sub())
    assert (s[:, 1] < s[:, 0]).all() and (s[:, 1] < s[:, 2]).all() and (s[:, 1] < s[:, 3]).all() and (s[:, 1] <= s[:, 4]).all()
    s = _filter_sums(png_cases.ramp_up())[1:]
    assert (s[:, 2] < s[:, 0]).all() and (s[:, 2] < s[:, 1]).all() and (s[:, 2] < s[:, 3]).all() and (s[:, 2] <= s[:, 4]).all()


def test_alpha_noise_is_noise_in_alpha_only():
    img = png_cases.alpha_noise(300, 200, 2)
    assert (img[:, :, :3] == img[0, 0, :3]).all()
    a = img[:, :, 3].tobytes()
    assert len(zlib.compress(a, 9)) >= 0.99 * len(a)


def test_exact_fit_shapes_fill_whole_segments(pf):
    if not os.path.exists(pf.SO_PATH):
        pytest.skip("libpanoflow.so is not built")
    S = pf.png_segment_bytes()
    names = sorted(png_cases.small_cases(S))
    for k in (1, 2):
        full = png_cases.fit_rows(S, k)
        lens = {}
        for rows in (full - 1, full, full + 1):
            name = "fit%d_noise_%dx%d" % (k, png_cases.FIT_COLS, rows)
            assert name in names
            img = png_cases.small_cases(S)[name]
            lens[rows] = len(R.filter_rows(img, [0] * rows))
        assert lens[full] == k * S
        assert lens[full - 1] == k * S - (4 * png_cases.FIT_COLS + 1) and lens[full + 1] == k * S + (4 * png_cases.FIT_COLS + 1)
    assert pf.png_bound(300, 200) >= 300 * 200 * 4 + 200
