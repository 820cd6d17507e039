"""Vectorised numpy model of the device reprojection (csrc/kernels_reproject.hip, csrc/reproject_math.hpp), restated:
an output pixel's ray, the rotation, longitude and latitude through the same range reduction and the same thirteen-term polynomial in
the same order of operations, the source position quantised to 8 fractional bits, and the integer bilinear / Catmull-Rom sample over
alpha-premultiplied colour.  Every numpy operation used on doubles (+ - * / sqrt) is the correctly rounded one and none is fused, so
the model's coordinates are what IEEE arithmetic gives for the written order; the tables go through this host's sin / cos / tan
(math.*: the C library's, as the library's own host code).  tests/test_reproject_model.py holds the model to libm and to properties
it does not restate; the host-run kernels and the device are held to the model, bit for bit."""
import math

import numpy as np

from resize_model import premultiply, unpremultiply

CUBE, RECTILINEAR, EQUIRECT = 0, 1, 2
FRONT, RIGHT, BACK, LEFT, UP, DOWN = range(6)
FACE_NAMES = ("front", "right", "back", "left", "up", "down")
BILINEAR, BICUBIC = 2, 3

PI = float.fromhex("0x1.921fb54442d18p+1")
TWO_PI = float.fromhex("0x1.921fb54442d18p+2")
HALF_PI = float.fromhex("0x1.921fb54442d18p+0")
PI_6 = float.fromhex("0x1.0c152382d7365p-1")
SQRT3 = float.fromhex("0x1.bb67ae8584caap+0")
TAN_PI_12 = float.fromhex("0x1.126145e9ecd56p-2")
ATAN_COEF = [float.fromhex(h) for h in (
    "0x1.0000000000000p+0", "-0x1.5555555555555p-2", "0x1.999999999999ap-3", "-0x1.2492492492492p-3", "0x1.c71c71c71c71cp-4",
    "-0x1.745d1745d1746p-4", "0x1.3b13b13b13b14p-4", "-0x1.1111111111111p-4", "0x1.e1e1e1e1e1e1ep-5", "-0x1.af286bca1af28p-5",
    "0x1.8618618618618p-5", "-0x1.642c8590b2164p-5", "0x1.47ae147ae147bp-5")]
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def rotation(yaw_deg=0.0, pitch_deg=0.0, roll_deg=0.0):
    """Rz(yaw) Ry(-pitch) Rx(roll), multiplied out in the library's order (reproject::rotation)"""
    yaw, pitch, roll = (yaw_deg * PI) / 180.0, (pitch_deg * PI) / 180.0, (roll_deg * PI) / 180.0
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    return [cy * cp, -(sy * cr) - (cy * sp) * sr, sy * sr - (cy * sp) * cr,
            sy * cp, cy * cr - (sy * sp) * sr, -(cy * sr) - (sy * sp) * cr,
            sp, cp * sr, cp * cr]


def atan_unit(t):
    big = t > TAN_PI_12
    num = np.where(big, t * SQRT3 - 1.0, t)
    den = np.where(big, SQRT3 + t, 1.0)
    r = num / den
    z = r * r
    p = np.full_like(r, ATAN_COEF[-1])
    for c in ATAN_COEF[-2::-1]:
        p = p * z + c
    return np.where(big, PI_6, 0.0) + r * p


def atan2_poly(y, x):
    ax, ay = np.where(x < 0.0, -x, x), np.where(y < 0.0, -y, y)
    swap = ay > ax
    mn, mx = np.where(swap, ax, ay), np.where(swap, ay, ax)
    r = atan_unit(mn / np.where(mx == 0.0, 1.0, mx))
    r = np.where(swap, HALF_PI - r, r)
    r = np.where(x < 0.0, PI - r, r)
    return np.where(y < 0.0, -r, r)


def equirect_tables(out_cols, out_rows):
    lon = [((u + 0.5) / out_cols - 0.5) * TWO_PI for u in range(out_cols)]
    lat = [((out_rows * 0.5 - (v + 0.5)) * TWO_PI) / out_cols for v in range(out_rows)]
    f = lambda fn, xs: np.array([fn(x) for x in xs], dtype=np.float64)
    return f(math.cos, lon), f(math.sin, lon), f(math.cos, lat), f(math.sin, lat)


def rays(projection, out_cols, out_rows, face=FRONT, hfov_deg=90.0):
    """the three components of every output pixel's ray, (out_rows, out_cols) doubles each"""
    u = np.arange(out_cols, dtype=np.float64)[None, :]
    v = np.arange(out_rows, dtype=np.float64)[:, None]
    shape = (out_rows, out_cols)
    if projection == EQUIRECT:
        cl, sl, cb, sb = equirect_tables(out_cols, out_rows)
        return [np.broadcast_to(cb[:, None] * cl[None, :], shape), np.broadcast_to(cb[:, None] * sl[None, :], shape), np.broadcast_to(sb[:, None], shape)]
    a = np.broadcast_to((2.0 * (u + 0.5)) / out_cols - 1.0, shape)
    b = np.broadcast_to(1.0 - (2.0 * (v + 0.5)) / out_rows, shape)
    one = np.ones(shape)
    if projection == RECTILINEAR:
        t = math.tan((hfov_deg * PI) / 360.0)
        return [one, a * t, ((b * t) * out_rows) / out_cols]
    return {FRONT: [one, a, b], RIGHT: [-a, one, b], BACK: [-one, -a, b], LEFT: [a, -one, b], UP: [-b, a, one], DOWN: [b, a, -one]}[face]


def source_position(d, rot, cols, rows):
    """unquantised (px, py) of rays d under the row-major rotation rot"""
    R = [float(x) for x in rot]
    sx = (R[0] * d[0] + R[1] * d[1]) + R[2] * d[2]
    sy = (R[3] * d[0] + R[4] * d[1]) + R[5] * d[2]
    sz = (R[6] * d[0] + R[7] * d[1]) + R[8] * d[2]
    lon = atan2_poly(sy, sx)
    lat = atan2_poly(sz, np.sqrt(sx * sx + sy * sy))
    px = (lon / TWO_PI + 0.5) * cols - 0.5
    py = (rows * 0.5 - 0.5) - (lat * cols) / TWO_PI
    return px, py


def coords(cols, rows, out_cols, out_rows, projection, face=FRONT, hfov_deg=90.0, rot=IDENTITY):
    """(fx, fy): int32 planes of floor(256 * position + 1/2); a position that is no number is outside (fy = INT32_MIN)"""
    with np.errstate(all="ignore"):
        px, py = source_position(rays(projection, out_cols, out_rows, face, hfov_deg), rot, cols, rows)
        qx, qy = 256.0 * px + 0.5, 256.0 * py + 0.5
        number = (qx >= -1.0e9) & (qx <= 1.0e9) & (qy >= -1.0e9) & (qy <= 1.0e9)
        fx = np.where(number, np.floor(np.where(number, qx, 0.0)), 0.0).astype(np.int64)
        fy = np.where(number, np.floor(np.where(number, qy, 0.0)), float(-2 ** 31)).astype(np.int64)
    return fx.astype(np.int32), fy.astype(np.int32)


def inside(fy, rows):
    return (fy >= -128) & (fy <= 256 * (rows - 1) + 128)


def cubic_weight(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def cubic_table():
    """(256, 4) int64: the taps at x0 - 1 .. x0 + 2 of phase f / 256, each phase summing to 2048"""
    tab = np.zeros((256, 4), dtype=np.int64)
    for f in range(256):
        t = f / 256.0
        w = [int(math.floor(cubic_weight(t - (i - 1)) * 2048.0 + 0.5)) for i in range(4)]
        w[w.index(max(w))] += 2048 - sum(w)
        tab[f] = w
    return tab


_CUBIC = cubic_table()


def sample_raw(img, fx, fy, filter):
    """the sample before its clamp to a byte and the un-premultiply: (out_rows, out_cols, 4) int64, the rounded sum shifted down"""
    rows, cols = img.shape[:2]
    pre = premultiply(np.ascontiguousarray(img)).astype(np.int64)
    fx, fy = fx.astype(np.int64), fy.astype(np.int64)
    x0, y0 = fx >> 8, fy >> 8
    if filter == BILINEAR:
        wx = np.stack([256 - (fx & 255), fx & 255], axis=-1); wy = np.stack([256 - (fy & 255), fy & 255], axis=-1)
        first, half, shift = 0, 32768, 16
    elif filter == BICUBIC:
        wx, wy = _CUBIC[fx & 255], _CUBIC[fy & 255]
        first, half, shift = -1, 1 << 21, 22
    else:
        raise ValueError("unknown filter %r" % (filter,))
    acc = np.zeros(fx.shape + (4,), dtype=np.int64)
    for j in range(wy.shape[-1]):
        yy = np.clip(y0 + first + j, 0, rows - 1)
        for i in range(wx.shape[-1]):
            xx = np.mod(x0 + first + i, cols)
            acc += (wx[..., i] * wy[..., j])[..., None] * pre[yy, xx]
    assert np.abs(acc).max(initial=0) + half < 2 ** 31   # the device accumulates in 32 bits
    return (acc + half) >> shift


def sample(img, fx, fy, filter):
    """(rows, cols, 4) uint8 with alpha last, int planes fx, fy -> (out_rows, out_cols, 4)"""
    out = unpremultiply(np.clip(sample_raw(img, fx, fy, filter), 0, 255).astype(np.uint8))
    out[~inside(fy, img.shape[0])] = 0
    return out


def reproject(img, out_cols, out_rows, projection, face=FRONT, filter=BICUBIC, hfov_deg=90.0, rot=IDENTITY):
    rows, cols = img.shape[:2]
    fx, fy = coords(cols, rows, out_cols, out_rows, projection, face, hfov_deg, rot)
    fy_in = np.where(inside(fy, rows), fy, 0)   # (an outside pixel's taps are never read)
    out = sample(img, fx, fy_in, filter)
    out[~inside(fy, rows)] = 0
    return out
