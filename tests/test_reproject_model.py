"""The reprojection model (tests/reproject_model.py) held to things it does not restate: its coordinates to the C library's atan2 and
sqrt, and its images to properties of the geometry (a constant image, the identity, a yaw of whole columns, the faces' shared edges,
the sense of yaw, pitch and roll) and of the weights."""
import math

import numpy as np
import pytest

import reproject_model as M
from resize_model import premultiply, unpremultiply

_atan2 = np.frompyfunc(math.atan2, 2, 1)
_sqrt = np.frompyfunc(math.sqrt, 1, 1)

ROTATIONS = [M.IDENTITY, M.rotation(37.0, -21.0, 11.0), M.rotation(0.0, 90.0, 0.0), M.rotation(-135.0, 60.0, -170.0), M.rotation(180.0, 0.0, 0.0),
             M.rotation(1.0e-7, -1.0e-7, 0.0)]
OUTPUTS = [(M.CUBE, 33, 33, face, 0.0) for face in range(6)] + [(M.RECTILINEAR, 40, 30, 0, 90.0), (M.RECTILINEAR, 31, 8, 0, 150.0), (M.RECTILINEAR, 16, 16, 0, 1.0),
                                                                (M.EQUIRECT, 64, 32, 0, 0.0), (M.EQUIRECT, 45, 23, 0, 0.0)]


def _random_rotation(rng):
    return M.rotation(*(float(x) for x in rng.uniform(-180.0, 180.0, size=3)))


def test_arctangent_against_libm():
    rng = np.random.default_rng(7)
    y = np.concatenate([rng.standard_normal(200000), [0.0, 0.0, 1.0, -1.0, 1e-300, 1.0, -0.0, 3.0], rng.standard_normal(1000) * 1e-9])
    x = np.concatenate([rng.standard_normal(200000), [1.0, -1.0, 0.0, 0.0, 1.0, 1e300, -1.0, -3.0], rng.standard_normal(1000)])
    # on both sides of the reduction's threshold and of the fold at 1
    t = np.concatenate([np.linspace(0.2679, 0.268, 5001), np.linspace(0.9999, 1.0001, 5001)])
    y, x = np.concatenate([y, t]), np.concatenate([x, np.ones_like(t)])
    want = _atan2(y, x).astype(np.float64)
    got = M.atan2_poly(y, x)
    same_angle = np.abs(got - want)
    same_angle = np.minimum(same_angle, np.abs(same_angle - 2 * math.pi))   # atan2(-0.0, -1) is -pi there and +pi here
    print("largest angle error: %.3g rad" % same_angle.max())
    assert same_angle.max() < 1.0e-15
    assert float(M.atan2_poly(np.array([0.0]), np.array([0.0]))[0]) == 0.0 and float(M.atan2_poly(np.array([-0.0]), np.array([-0.0]))[0]) == 0.0


@pytest.mark.parametrize("size", [(64, 32), (9000, 4000), (65535, 32767), (65535, 65535)], ids=lambda s: "%dx%d" % s)
def test_coordinates_against_libm(size):
    cols, rows = size
    worst = 0.0
    for (proj, w, h, face, hfov) in OUTPUTS:
        d = M.rays(proj, w, h, face, hfov)
        for rot in ROTATIONS:
            px, py = M.source_position(d, rot, cols, rows)
            R = np.array(rot).reshape(3, 3)
            s = [R[k, 0] * d[0] + R[k, 1] * d[1] + R[k, 2] * d[2] for k in range(3)]
            lon = _atan2(s[1], s[0]).astype(np.float64)
            lat = _atan2(s[2], _sqrt(s[0] * s[0] + s[1] * s[1]).astype(np.float64)).astype(np.float64)
            wx = (lon / (2 * math.pi) + 0.5) * cols - 0.5
            wy = (rows / 2 - 0.5) - lat * cols / (2 * math.pi)
            ex = np.abs(px - wx)
            ex = np.minimum(ex, np.abs(ex - cols))   # the seam: longitude -pi and +pi are one column
            ex = np.where((s[0] == 0.0) & (s[1] == 0.0), np.abs(px - (cols / 2 - 0.5)), ex)   # exactly at a pole the longitude is 0 by definition
            worst = max(worst, float(ex.max()), float(np.abs(py - wy).max()))
    print("largest coordinate error at %d x %d: %.3g px (bound %.3g)" % (cols, rows, worst, 2.0 ** -20))
    assert worst <= 2.0 ** -20


@pytest.mark.parametrize("size", [(64, 32), (90, 40), (67, 33)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("flt", [M.BILINEAR, M.BICUBIC])
def test_constant_image(size, flt):
    cols, rows = size
    colour = np.array([17, 200, 93, 255], np.uint8)
    img = np.empty((rows, cols, 4), np.uint8); img[:] = colour
    rng = np.random.default_rng(cols)
    some_inside = some_outside = False
    for (proj, w, h, face, hfov) in [(M.CUBE, 19, 19, f, 0.0) for f in range(6)] + [(M.RECTILINEAR, 21, 13, 0, 120.0), (M.EQUIRECT, 50, 25, 0, 0.0)]:
        for rot in [M.IDENTITY, M.rotation(0.0, 90.0, 0.0)] + [_random_rotation(rng) for _ in range(4)]:
            out = M.reproject(img, w, h, proj, face, flt, hfov, rot)
            _, fy = M.coords(cols, rows, w, h, proj, face, hfov, rot)
            ins = M.inside(fy, rows)
            assert (out[ins] == colour).all() and (out[~ins] == 0).all()
            some_inside |= bool(ins.any()); some_outside |= bool((~ins).any())
    assert some_inside and (some_outside or cols == 2 * rows)   # 90 x 40 and 67 x 33 do not cover the poles


def _image(cols, rows, seed=3):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(rows, cols, 4), dtype=np.uint8)
    img[: rows // 2, : cols // 3, 3] = 0
    img[rows // 2:, cols // 2:, 3] = 255
    return img


@pytest.mark.parametrize("size", [(64, 32), (90, 40), (67, 33)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("flt", [M.BILINEAR, M.BICUBIC])
def test_identity_and_whole_columns(size, flt):
    cols, rows = size
    img = _image(cols, rows)
    same = unpremultiply(premultiply(img))
    assert np.array_equal(M.reproject(img, cols, rows, M.EQUIRECT, filter=flt), same)
    for k in (1, 5, cols // 2, cols - 1, -7):
        out = M.reproject(img, cols, rows, M.EQUIRECT, filter=flt, rot=M.rotation(k * 360.0 / cols, 0.0, 0.0))
        # a yaw to the right by k columns: output column u shows source column u + k
        assert np.array_equal(out, np.roll(same, -k, axis=1)), k


def test_front_face_centre_and_shared_edges():
    for cols, rows in ((64, 32), (9000, 4000), (67, 33)):
        for n in (1, 7, 65):
            px, py = M.source_position(M.rays(M.CUBE, n, n, M.FRONT), M.IDENTITY, cols, rows)
            assert px[n // 2, n // 2] == cols / 2 - 0.5 and py[n // 2, n // 2] == rows / 2 - 0.5
    # the rays of the cube's shared edges: half a pixel beyond the last row of one face is half a pixel before the first row of the next.
    # On the edge itself (b = +-1) the up face's bottom, the front face's top ... are the same rays, so they sample the same positions
    n = 16
    a = (2.0 * (np.arange(n) + 0.5)) / n - 1.0
    one = np.ones(n)
    edge = lambda face, b: {M.FRONT: [one, a, b * one], M.UP: [-b * one, a, one], M.DOWN: [b * one, a, -one]}[face]
    for rot in (M.IDENTITY, M.rotation(37.0, -21.0, 11.0)):
        for (f0, b0, f1, b1) in ((M.UP, -1.0, M.FRONT, 1.0), (M.FRONT, -1.0, M.DOWN, 1.0)):
            p0 = M.source_position(edge(f0, b0), rot, 64, 32); p1 = M.source_position(edge(f1, b1), rot, 64, 32)
            assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1])
    # ... and the model's own rays meet that edge from both sides: the last row of `up` mirrors the first row of `front` in the edge's plane
    up, front, down = (M.rays(M.CUBE, n, n, f) for f in (M.UP, M.FRONT, M.DOWN))
    assert np.array_equal(up[0][-1], front[2][0]) and np.array_equal(up[2][-1], front[0][0]) and np.array_equal(up[1][-1], front[1][0])
    assert np.array_equal(front[2][-1], -down[0][0]) and np.array_equal(front[0][-1], -down[2][0]) and np.array_equal(front[1][-1], down[1][0])
    assert (up[0][-1] == 1.0 - 1.0 / n).all() and (down[0][0] == 1.0 - 1.0 / n).all()


def test_sense_of_yaw_pitch_roll():
    cols, rows, n = 720, 360, 9
    c = n // 2
    centre = lambda rot: tuple(float(p[c, c]) for p in M.source_position(M.rays(M.CUBE, n, n, M.FRONT), rot, cols, rows))
    x0, y0 = centre(M.IDENTITY)
    assert centre(M.rotation(30.0, 0.0, 0.0)) == pytest.approx((x0 + 60.0, y0), abs=1e-9)      # to the right: later columns
    assert centre(M.rotation(0.0, 30.0, 0.0)) == pytest.approx((x0, y0 - 60.0), abs=1e-9)      # up: earlier rows
    px, py = M.source_position(M.rays(M.CUBE, n, n, M.FRONT), M.rotation(0.0, 0.0, 20.0), cols, rows)
    assert py[c, -1] < y0 < py[c, 0] and centre(M.rotation(0.0, 0.0, 20.0)) == pytest.approx((x0, y0), abs=1e-9)   # the right side looks higher
    # the side faces are the front face after a quarter turn
    for face, yaw in ((M.RIGHT, 90.0), (M.BACK, 180.0), (M.LEFT, -90.0)):
        a = M.source_position(M.rays(M.CUBE, n, n, face), M.IDENTITY, cols, rows)
        b = M.source_position(M.rays(M.CUBE, n, n, M.FRONT), M.rotation(yaw, 0.0, 0.0), cols, rows)
        dx = np.abs(a[0] - b[0]); dx = np.minimum(dx, np.abs(dx - cols))
        assert dx.max() < 1e-9 and np.abs(a[1] - b[1]).max() < 1e-9
    for face, pitch in ((M.UP, 90.0), (M.DOWN, -90.0)):
        a = M.source_position(M.rays(M.CUBE, n, n, face), M.IDENTITY, cols, rows)
        b = M.source_position(M.rays(M.CUBE, n, n, M.FRONT), M.rotation(0.0, pitch, 0.0), cols, rows)
        dx = np.abs(a[0] - b[0]); dx = np.minimum(dx, np.abs(dx - cols))
        far = np.abs(a[1] - (rows / 2 - 0.5)) < 89.0 * cols / 360   # (away from the pole itself, where the longitude is ill-conditioned)
        assert dx[far].max() < 1e-6 and np.abs(a[1] - b[1]).max() < 1e-9


def test_bicubic_table():
    tab = M.cubic_table()
    assert (tab.sum(axis=1) == 2048).all()
    assert list(tab[0]) == [0, 2048, 0, 0] and list(tab[128]) == [-128, 1152, 1152, -128]
    assert np.abs(tab).sum(axis=1).max() <= 1.25 * 2048
    exact = np.array([[M.cubic_weight(f / 256.0 - (i - 1)) * 2048 for i in range(4)] for f in range(256)])
    # every tap is rounded (within 1/2); the largest also takes the phase's remainder, at most four halves
    err = np.sort(np.abs(tab - exact), axis=1)
    assert err[:, :3].max() <= 0.5 and err[:, 3].max() <= 2.5


def test_library_host_helpers_are_the_models(pf):
    pf.build()
    for ypr in ((0.0, 0.0, 0.0), (37.0, -21.0, 11.0), (0.0, 90.0, 0.0), (16.875, 0.0, 0.0), (-135.0, 60.0, -170.0)):
        assert pf.reproject_rotation(*ypr) == M.rotation(*ypr)
    p = pf.reproject_params()
    assert (p.projection, p.face, p.filter, list(p.rot)) == (M.CUBE, M.FRONT, M.BICUBIC, M.IDENTITY)
