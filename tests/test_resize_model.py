"""CPU tier: the serial model of the device resize (tests/resize_model.py) equals Pillow's Image.resize of an RGBA image, byte for byte,
for all five filters: on down- and upscaling shapes with transparent, opaque and random alpha, on the same size (a copy) and on the
image that holds every (colour, alpha) pair, where every premultiply and every reachable un-premultiply operand occurs."""
import numpy as np
import pytest
from PIL import Image

import resize_cases
import resize_model


def pillow(img, out_cols, out_rows, f):
    return np.asarray(Image.fromarray(img, "RGBA").resize((out_cols, out_rows), f))


def test_filter_numbers_are_pillows():
    R = Image.Resampling
    assert (R.LANCZOS, R.BILINEAR, R.BICUBIC, R.BOX, R.HAMMING) == (1, 2, 3, 4, 5) == tuple(resize_cases.FILTER_IDS)


@pytest.mark.parametrize("f", resize_cases.FILTER_IDS)
@pytest.mark.parametrize("shape", resize_cases.MODEL_SHAPES + [resize_cases.PIECE_SHAPE], ids=lambda s: "%dx%d_to_%dx%d" % s)
def test_model_is_pillow(shape, f):
    cols, rows, out_cols, out_rows = shape
    img = resize_cases.image(cols, rows)
    got, want = resize_model.resize(img, out_cols, out_rows, f), pillow(img, out_cols, out_rows, f)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert int((got != want).sum()) == 0


@pytest.mark.parametrize("f", resize_cases.FILTER_IDS)
def test_same_size_is_a_copy(f):
    img = resize_cases.image(37, 23)
    assert np.array_equal(resize_model.resize(img, 37, 23, f), img)
    assert np.array_equal(pillow(img, 37, 23, f), img)
    # ... which a premultiply round trip would not be
    assert not np.array_equal(resize_model.unpremultiply(resize_model.premultiply(resize_cases.all_pairs())), resize_cases.all_pairs())


def test_all_pairs_box_doubling():
    img = resize_cases.all_pairs()
    got = resize_model.resize(img, 512, 512, resize_model.BOX)
    assert int((got != pillow(img, 512, 512, resize_model.BOX)).sum()) == 0
    round_trip = resize_model.unpremultiply(resize_model.premultiply(img))
    assert np.array_equal(got, np.repeat(np.repeat(round_trip, 2, axis=0), 2, axis=1))


def test_medium_shape():
    cols, rows, out_cols, out_rows = resize_cases.MEDIUM_SHAPE
    img = resize_cases.image(cols, rows)
    got = resize_cases.model("medium", img, out_cols, out_rows, resize_model.LANCZOS)
    assert int((got != pillow(img, out_cols, out_rows, resize_model.LANCZOS)).sum()) == 0
