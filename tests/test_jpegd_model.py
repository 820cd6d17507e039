"""CPU tier: the JPEG decoder's model (tests/jpegd_model.py) equals Pillow (libjpeg-turbo) on every valid case of tests/jpegd_cases.py,
and the edge rules DESIGN.md 8.10 states are pinned on hand-made planes."""
import numpy as np
import pytest

import jpegd_cases as jc
import jpegd_model as jm


def test_model_equals_pillow_on_every_valid_case():
    cases = jc.all_valid_cases()
    names = [n for n, _ in cases]
    assert len(cases) > 90 and len(set(names)) == len(names)
    wrong = []
    for name, data in cases:
        r = jm.decode(data)
        if not r["accept"] or not np.array_equal(jm.bgra(r["rgb"]), jc.pillow_bgra(data)):
            wrong.append(name)
    assert not wrong, wrong


def test_the_grid_covers_its_axes():
    names = [n for n, _ in jc.grid_cases()]
    for word in ("1x1-", "7x9-", "35x7-", "-444-", "-422-", "-420-", "-grey-", "-q1-", "-q100-", "-opt-", "-std-", "-r0", "-r1", "-r3", "noise", "ramp"):
        assert any(word in n for n in names), word
    for what in jc.SEAMS:
        assert jc.seam_case(what, jc.S_MIN)


def test_h2v1_edges_and_rounding():
    p = np.array([[10, 20, 40, 41]])
    out = jm.upsample_h2v1(p)
    assert out.tolist() == [[10, (30 + 20 + 2) >> 2, (60 + 10 + 1) >> 2, (60 + 40 + 2) >> 2, (120 + 20 + 1) >> 2, (120 + 41 + 2) >> 2, (123 + 40 + 1) >> 2, 41]]
    assert jm.upsample_h2v1(np.array([[7, 200]])).tolist() == [[7, 7, 200, 200]]        # two samples a row: plain replication
    assert jm.upsample_h2v1(np.array([[9]])).tolist() == [[9, 9]]


def test_h2v2_edges_and_rounding():
    p = np.array([[0, 100, 200], [50, 150, 250]])
    out = jm.upsample_h2v2(p)
    s0 = [3 * a + a for a in p[0]]; s1 = [3 * a + b for a, b in zip(p[0], p[1])]
    assert out[0].tolist() == [(4 * s0[0] + 8) >> 4, (3 * s0[0] + s0[1] + 7) >> 4, (3 * s0[1] + s0[0] + 8) >> 4, (3 * s0[1] + s0[2] + 7) >> 4,
                               (3 * s0[2] + s0[1] + 8) >> 4, (4 * s0[2] + 7) >> 4]
    assert out[1, 1] == (3 * s1[0] + s1[1] + 7) >> 4 and out[1, 2] == (3 * s1[1] + s1[0] + 8) >> 4
    assert out[3].tolist() == jm.upsample_h2v2(p[::-1])[0].tolist()                      # the last row replicates as the first does
    assert jm.upsample_h2v2(np.array([[1, 2], [3, 4]])).tolist() == [[1, 1, 2, 2], [1, 1, 2, 2], [3, 3, 4, 4], [3, 3, 4, 4]]


def test_colour_constants_and_clamp():
    y = np.array([[0, 255, 128, 255]]); cb = np.array([[128, 128, 255, 0]]); cr = np.array([[128, 128, 0, 255]])
    out = jm.colour(y, cb, cr)
    assert out[0, 0].tolist() == [0, 0, 0] and out[0, 1].tolist() == [255, 255, 255]
    assert out[0, 2].tolist() == [0, 128 + ((-22554 * 127 + 46802 * 128 + 32768) >> 16), 255]
    assert out[0, 3].tolist() == [255, 255 + ((22554 * 128 - 46802 * 127 + 32768) >> 16), 255 + ((-116130 * 128 + 32768) >> 16)]     # R clamps


def test_idct_dc_only_and_clamp():
    q = np.ones(64, np.int32)
    c = np.zeros((3, 64), np.int32); c[0, 0] = 8; c[1, 0] = 2000; c[2, 0] = -2000
    out = jm.idct_blocks(c, q)
    assert (out[0] == 129).all() and (out[1] == 255).all() and (out[2] == 0).all()


def test_events_name_the_mcu():
    data = jc.pil_jpeg(jc.scene(48, 32, 4), 80, "420", False, 2)
    info = jm.parse(data)
    b, e = info["begin"], info["end"]
    assert jm.decode(data)["accept"]
    cut = jm.decode(data[:b + (e - b) // 2] + data[e:])
    assert not cut["accept"] and 0 < cut["event_mcu"] < 6
    k = data.index(b"\xff\xd0", b)
    wrong_marker = jm.decode(data[:k + 1] + b"\xd3" + data[k + 2:])
    assert not wrong_marker["accept"] and wrong_marker["event_mcu"] == 2
    longer = jm.decode(data[:e] + b"\x00\x00" + data[e:])
    assert not longer["accept"] and longer["event_mcu"] == 6
