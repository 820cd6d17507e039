"""Vectorised numpy model of the device lens remap (csrc/kernels_lens.hip, csrc/lens_math.hpp), restated: a canvas
pixel's ray from the canvas's tables, the rotation into the camera, the outside exits, the lens model's radius, the radial polynomial,
the position in the photo quantised to 8 fractional bits, and the reprojection's integer bilinear / Catmull-Rom sample over
alpha-premultiplied colour with columns clamped like rows.  What it shares with the reprojection (the arctangent, the tables, the
phase table, the rotation) is imported from reproject_model, not restated.  Every numpy operation used on doubles (+ - * / sqrt) is
the correctly rounded one and none is fused; focal() and the tables go through this host's libm (math.*), as the library's host code.
tests/test_lens_model.py holds the model to libm and to the reprojection's conventions; the host-run kernel and the device are held
to the model, bit for bit."""
import math

import numpy as np

import reproject_model as R
from resize_model import premultiply, unpremultiply

RECTILINEAR, EQUIDISTANT, STEREOGRAPHIC, EQUISOLID = range(4)
MODEL_NAMES = ("rectilinear", "equidistant", "stereographic", "equisolid")
BILINEAR, BICUBIC = R.BILINEAR, R.BICUBIC


class Lens:
    """pf_lens with pf_lens_init's defaults (focal_px has none: it is asked for)"""

    def __init__(self, model, focal_px, filter=BICUBIC, a=0.0, b=0.0, c=0.0, dd=1.0, shift_x=0.0, shift_y=0.0, min_cos=None, crop=(0, 0, 0), rot=R.IDENTITY):
        self.model, self.focal_px, self.filter = model, float(focal_px), filter
        self.a, self.b, self.c, self.dd = float(a), float(b), float(c), float(dd)
        self.shift_x, self.shift_y = float(shift_x), float(shift_y)
        self.min_cos = float((0.0 if model == RECTILINEAR else -0.5) if min_cos is None else min_cos)
        self.crop = tuple(int(v) for v in crop)   # (cx256, cy256, r256)
        self.rot = [float(x) for x in rot]


def focal(model, photo_cols, hfov_deg):
    """lens::focal (pf_lens_focal), in its order of operations"""
    hfov = (hfov_deg * R.PI) / 180.0
    if model == RECTILINEAR:
        return (photo_cols * 0.5) / math.tan(hfov * 0.5)
    if model == EQUIDISTANT:
        return photo_cols / hfov
    if model == STEREOGRAPHIC:
        return (photo_cols * 0.5) / (2.0 * math.tan(hfov * 0.25))
    if model == EQUISOLID:
        return (photo_cols * 0.5) / (2.0 * math.sin(hfov * 0.25))
    raise ValueError("unknown model %r" % (model,))


def rotation(yaw_deg=0.0, pitch_deg=0.0, roll_deg=0.0):
    """lens::rotation (pf_lens_rotation): the transpose of the reprojection's rotation"""
    r = R.rotation(yaw_deg, pitch_deg, roll_deg)
    return [r[3 * j + i] for i in range(3) for j in range(3)]


def canvas_rays(cols, rows):
    return R.rays(R.EQUIRECT, cols, rows)


def photo_position(d, lens, photo_cols, photo_rows):
    """(px, py, seen): the unquantised position of rays d in the photo; seen is False where the camera does not see the ray (the
    position there is arbitrary)"""
    M = lens.rot
    cx = (M[0] * d[0] + M[1] * d[1]) + M[2] * d[2]
    cy = (M[3] * d[0] + M[4] * d[1]) + M[5] * d[2]
    cz = (M[6] * d[0] + M[7] * d[1]) + M[8] * d[2]
    rho = np.sqrt(cy * cy + cz * cz)
    n = np.sqrt((cx * cx + cy * cy) + cz * cz)
    seen = ~((n == 0.0) | (cx <= lens.min_cos * n))
    if lens.model == RECTILINEAR:
        g = rho / cx
    elif lens.model == EQUIDISTANT:
        g = R.atan2_poly(rho, cx)
    else:
        m = n + cx
        seen &= ~(m <= 0.0)
        g = (2.0 * rho) / (m if lens.model == STEREOGRAPHIC else np.sqrt((2.0 * n) * m))
    r = lens.focal_px * g
    rn = r / (min(photo_cols, photo_rows) * 0.5)
    s = ((lens.a * rn + lens.b) * rn + lens.c) * rn + lens.dd
    r_src = r * s
    k = np.where(rho == 0.0, 0.0, r_src / np.where(rho == 0.0, 1.0, rho))
    px = ((photo_cols * 0.5 - 0.5) + lens.shift_x) + k * cy
    py = ((photo_rows * 0.5 - 0.5) + lens.shift_y) - k * cz
    return px, py, seen


def coords(photo_cols, photo_rows, cols, rows, lens):
    """(fx, fy): int32 planes of floor(256 * position + 1/2); a pixel with no position has fx = 0, fy = INT32_MIN"""
    return coords_of_rays(canvas_rays(cols, rows), photo_cols, photo_rows, lens)


def coords_of_rays(d, photo_cols, photo_rows, lens):
    with np.errstate(all="ignore"):
        px, py, seen = photo_position(d, lens, photo_cols, photo_rows)
        qx, qy = 256.0 * px + 0.5, 256.0 * py + 0.5
        number = seen & (qx >= -1.0e9) & (qx <= 1.0e9) & (qy >= -1.0e9) & (qy <= 1.0e9)
        fx = np.where(number, np.floor(np.where(number, qx, 0.0)), 0.0).astype(np.int64)
        fy = np.where(number, np.floor(np.where(number, qy, 0.0)), float(-2 ** 31)).astype(np.int64)
    return fx.astype(np.int32), fy.astype(np.int32)


def inside(fx, fy, photo_cols, photo_rows, lens):
    fx, fy = fx.astype(np.int64), fy.astype(np.int64)
    ok = (fx >= -128) & (fx <= 256 * (photo_cols - 1) + 128) & (fy >= -128) & (fy <= 256 * (photo_rows - 1) + 128)
    cx, cy, cr = lens.crop
    if cr > 0:
        # (64 unsigned bits, as the library: they hold the sum of the squares of two differences of 32-bit numbers)
        dx = np.abs(fx - cx).astype(np.uint64); dy = np.abs(fy - cy).astype(np.uint64)
        ok &= dx * dx + dy * dy <= np.uint64(cr * cr)
    return ok


def sample_raw(img, fx, fy, filter):
    """R.sample_raw with columns clamped: the sample before its clamp to a byte and the un-premultiply, (out_rows, out_cols, 4) int64"""
    rows, cols = img.shape[:2]
    pre = premultiply(np.ascontiguousarray(img)).astype(np.int64)
    fx, fy = fx.astype(np.int64), fy.astype(np.int64)
    x0, y0 = fx >> 8, fy >> 8
    if filter == BILINEAR:
        wx = np.stack([256 - (fx & 255), fx & 255], axis=-1); wy = np.stack([256 - (fy & 255), fy & 255], axis=-1)
        first, half, shift = 0, 32768, 16
    elif filter == BICUBIC:
        wx, wy = R._CUBIC[fx & 255], R._CUBIC[fy & 255]
        first, half, shift = -1, 1 << 21, 22
    else:
        raise ValueError("unknown filter %r" % (filter,))
    acc = np.zeros(fx.shape + (4,), dtype=np.int64)
    for j in range(wy.shape[-1]):
        yy = np.clip(y0 + first + j, 0, rows - 1)
        for i in range(wx.shape[-1]):
            xx = np.clip(x0 + first + i, 0, cols - 1)
            acc += (wx[..., i] * wy[..., j])[..., None] * pre[yy, xx]
    assert np.abs(acc).max(initial=0) + half < 2 ** 31   # the device accumulates in 32 bits
    return (acc + half) >> shift


def sample(img, fx, fy, filter):
    """R.sample with columns clamped: (rows, cols, 4) uint8 with alpha last, int planes fx, fy -> (out_rows, out_cols, 4); every
    position is taken as inside"""
    return unpremultiply(np.clip(sample_raw(img, fx, fy, filter), 0, 255).astype(np.uint8))


def remap_from_coords(photo, fx, fy, lens):
    ok = inside(fx, fy, photo.shape[1], photo.shape[0], lens)
    out = sample(photo, np.where(ok, fx, 0), np.where(ok, fy, 0), lens.filter)   # (an outside pixel's taps are never read)
    out[~ok] = 0
    return out


def remap(photo, cols, rows, lens):
    """the canvas (rows, cols, 4) of a photo (photo_rows, photo_cols, 4) under a Lens"""
    fx, fy = coords(photo.shape[1], photo.shape[0], cols, rows, lens)
    return remap_from_coords(photo, fx, fy, lens)
