"""CPU tier: the serial TIFF model (tests/tiff_model.py) is held to libtiff both ways through Pillow -- the model decodes Pillow's files to
the image, Pillow decodes every well-formed model-written file to the image -- and the closed form for the bit offset of an LZW code is
held to a serial walk of the same streams."""
import numpy as np
import pytest

import tiff_cases
import tiff_model as tm


@pytest.fixture(scope="module")
def cases(synth):
    return tiff_cases.cases(synth)


# (libtiff applies the predictor to LZW and deflate only)
@pytest.mark.parametrize("compression,rps,predictor", [("raw", None, None), ("raw", 1, None), ("packbits", None, None), ("packbits", 1, None),
                                                       ("tiff_lzw", None, None), ("tiff_lzw", 1, None), ("tiff_lzw", 5, 2), ("tiff_lzw", 1, 2)])
def test_model_reads_pillow(compression, rps, predictor):
    for spp in (3, 4):
        img = tiff_cases.smooth(37, 65, spp, 3)
        data = tiff_cases.pillow_tiff(img, compression, rps, predictor)
        f = tm.parse(data)
        assert f[259][0] == {"raw": 1, "tiff_lzw": 5, "packbits": 32773}[compression]
        assert f.get(317, [1])[0] == (predictor or 1) and (rps is None or f[278][0] == rps)
        got, status = tm.decode(data)
        assert all(a == b and r == 0 for a, b, r in status)
        assert np.array_equal(got, tm.expected_bgra(img))


def test_pillow_reads_model_files(cases):
    checked = 0
    for name, c in sorted(cases.items()):
        got, status = tm.decode(c.file)
        assert all(a == b and r == 0 for a, b, r in status), name
        assert np.array_equal(got, tm.expected_bgra(c.img)), name
        if c.pillow:
            assert np.array_equal(tiff_cases.pillow_read(c.file), c.img), name
            checked += 1
    assert checked == len(cases) - 9   # never_clear, no_eoi, no_leading_clear and the six uncompressed predictor files


def test_bit_offset_closed_form_matches_a_serial_walk():
    # width changes at j = 254, 766, 1790; with and without Clears in between; a full table
    assert [tm.lzw_width(j) for j in (0, 253, 254, 765, 766, 1789, 1790, 3838, 10 ** 6)] == [9, 9, 10, 10, 11, 11, 12, 12, 12]
    data = tiff_cases.noise(1, 4000, 3, 11).tobytes()
    for kw in (dict(), dict(never_clear=True), dict(clear_every=300), dict(clear_at_start=False), dict(clear_every=1)):
        stream = tm.lzw_encode(data, **kw)
        walk = tm.lzw_walk(stream)
        assert walk[-1][2] == tm.EOI
        base = 0   # bit position of code 0 after the last Clear
        for pos, wd, code, j in walk:
            assert pos == base + tm.lzw_offset(j) and wd == tm.lzw_width(j)
            if code == tm.CLEAR:
                base = pos + wd
        assert max(j for _, _, _, j in walk) >= (4000 if kw.get("never_clear") else 0)
        assert tm.lzw_decode(stream, len(data)) == (data, 0)


def test_model_on_malformed_streams():
    bad = tiff_cases.malformed()
    reasons = {}
    for name, data in bad.items():
        _, status = tm.decode(data)
        short = [(s, a, b, r) for s, (a, b, r) in enumerate(status) if a != b]
        assert short, name
        reasons[name] = short[0]
    assert reasons["code_above_next"][1:] == (1, 60, tm.REASON_BAD_CODE)
    assert reasons["first_code_not_literal"] == (1, 2, 60, tm.REASON_BAD_CODE)
    assert reasons["early_eoi"] == (1, 2, 60, tm.REASON_OK)
    assert reasons["packbits_cut_literal"][3] == tm.REASON_CUT_PACKET and reasons["packbits_cut_repeat"][3] == tm.REASON_CUT_PACKET
    assert reasons["cut_code"][3] == tm.REASON_OK and 0 < reasons["cut_code"][1] < 60
