"""Photos, canvases, lenses, poses and filters shared by the lens remap's tests (host-run kernel vs model, device vs model).

The options are not multiplied out.  Photo x canvas x (model, hfov) x pose x filter is the frame; the three on/off options
(polynomial, shift, crop circle) ride on it as two rows of the orthogonal array L4(2^3), the rows chosen by the frame's indices, so
that every pair of option values meets every frame value somewhere in the list.  That is 1152 candidates, the reprojection's count.

Of the candidates, those stay whose geometry leaves at least a tenth of the canvas inside the photo and a tenth outside, decided by
the model (a 60 degree rectilinear 4:3 photo covers 4 % of a sphere wherever it looks but up: it stays with the top camera; a kernel
that writes zeros, or never does, fails every case that is left).  tests/test_lens_model.py asserts the condition on every case of the
list, that every option value listed here is still in it, and its size.  One named case per lens model is all outside on purpose."""
import numpy as np

import lens_model as M
import resize_cases

FILTERS = [M.BILINEAR, M.BICUBIC]

# (name): landscape; odd and portrait; one image with every alpha class (a crop of the all-pairs image: alpha = row, colour = column)
PHOTOS = ["64x48", "33x67", "pairs"]

# 2:1; 160 degrees of latitude; one pixel past two 32-wide workgroup tiles and past eight 8-row tiles
CANVASES = [(64, 32), (90, 40), (130, 65)]

# (model, hfov in degrees): each model narrow and wide
LENSES = [(M.RECTILINEAR, 60.0), (M.RECTILINEAR, 120.0)] + [(m, h) for m in (M.EQUIDISTANT, M.STEREOGRAPHIC, M.EQUISOLID) for h in (120.0, 190.0)]

# identity; a generic turn; a top camera (the pole inside the photo); a camera looking back (the canvas's seam through the photo)
ROTATIONS = {
    "identity": M.rotation(),
    "generic": M.rotation(37.0, -21.0, 11.0),
    "pitch90": M.rotation(0.0, 90.0, 0.0),
    "yaw180": M.rotation(180.0, 0.0, 0.0),
}

POLYNOMIAL = (0.01, -0.05, 0.02)   # dd = 1 - (a + b + c), as the .pto reader sets it
SHIFT = (1.5, -2.25)
L4 = [(0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0)]   # (polynomial, shift, crop)

MIN_INSIDE = MIN_OUTSIDE = 0.10


# a fourth photo for a few BICUBIC cases: the opaque ringing image (resize_cases.ringing, 64 x 32, blocks of 2 x 2), whose taps overshoot in
# every channel, so that the sample's clamp to a byte works in both directions in all four byte positions.  Not in PHOTOS: it rides on
# ringing_cases() only
RINGING_MIN_CLAMPED = 10


def photo(name):
    if name == "ringing":
        return resize_cases.ringing(64, 32, 2, 2)
    if name == "pairs":
        rows = list(range(0, 248, 8)) + [255]   # 64 x 32: alphas 0, 8, .. 240 and 255 against colours 0, 4, .. 252
        return np.ascontiguousarray(resize_cases.all_pairs()[rows][:, :256:4])
    cols, rows = (int(x) for x in name.split("x"))
    return resize_cases.image(cols, rows)


def crop_circle(photo_cols, photo_rows):
    """an image circle in 1/256 px that cuts the photo's corners, its centre off the photo's by a fraction of a pixel"""
    return ((photo_cols - 1) * 128 + 320, (photo_rows - 1) * 128 - 192, int(0.6 * 256 * min(photo_cols, photo_rows)))


def make_lens(photo_cols, photo_rows, model, hfov, rot_name, poly, shift, crop, flt):
    a, b, c = POLYNOMIAL if poly else (0.0, 0.0, 0.0)
    sx, sy = SHIFT if shift else (0.0, 0.0)
    return M.Lens(model, M.focal(model, photo_cols, hfov), filter=flt, a=a, b=b, c=c, dd=1.0 - (a + b + c), shift_x=sx, shift_y=sy,
                  crop=crop_circle(photo_cols, photo_rows) if crop else (0, 0, 0), rot=ROTATIONS[rot_name])


class Case:
    def __init__(self, name, photo_name, cols, rows, lens, key):
        self.name, self.photo, self.cols, self.rows, self.lens = name, photo_name, cols, rows, lens
        self.key = key   # what the coordinates depend on (not the pixels, not the filter)


_PHOTOS = {}
_COORDS = {}
_IMAGES = {}
_CASES = []


def photo_cached(name):
    if name not in _PHOTOS:
        _PHOTOS[name] = photo(name)
        _PHOTOS[name].setflags(write=False)
    return _PHOTOS[name]


def model_coords(case):
    """the model's (fx, fy) of a case, computed once (they do not depend on the pixels or the filter)"""
    if case.key not in _COORDS:
        pr, pc = photo_cached(case.photo).shape[:2]
        fx, fy = M.coords(pc, pr, case.cols, case.rows, case.lens)
        fx.setflags(write=False); fy.setflags(write=False)
        _COORDS[case.key] = (fx, fy)
    return _COORDS[case.key]


def inside_fraction(case):
    pr, pc = photo_cached(case.photo).shape[:2]
    fx, fy = model_coords(case)
    return float(M.inside(fx, fy, pc, pr, case.lens).mean())


def model_image(case):
    """the model's canvas of a case, computed once and shared between tests (read-only)"""
    if case.name not in _IMAGES:
        fx, fy = model_coords(case)
        out = M.remap_from_coords(photo_cached(case.photo), fx, fy, case.lens)
        out.setflags(write=False)
        _IMAGES[case.name] = out
    return _IMAGES[case.name]


def candidates():
    out = []
    for pi, p in enumerate(PHOTOS):
        pr, pc = photo_cached(p).shape[:2]
        for ci, (w, h) in enumerate(CANVASES):
            for li, (model, hfov) in enumerate(LENSES):
                for ri, r in enumerate(ROTATIONS):
                    for fi, flt in enumerate(FILTERS):
                        for o in range(2):
                            poly, shift, crop = L4[(pi + ci + li + ri + fi + o) % 4]
                            name = "%s_%dx%d_%s%g_%s_p%ds%dc%d_%s" % (p, w, h, M.MODEL_NAMES[model], hfov, r, poly, shift, crop, "cubic" if flt == M.BICUBIC else "linear")
                            key = (p, w, h, model, hfov, r, poly, shift, crop)
                            out.append(Case(name, p, w, h, make_lens(pc, pr, model, hfov, r, poly, shift, crop, flt), key))
    return out


def ringing_cases():
    """one equidistant and one rectilinear case of the list (canvas, lens model, pose and options), with the ringing photo in place of theirs"""
    out = []
    for name in ("64x48_130x65_equidistant190_generic_p1s1c0_cubic", "64x48_130x65_rectilinear120_pitch90_p1s1c0_cubic"):
        base = [c for c in cases() if c.name == name]
        assert len(base) == 1, name
        _, w, h, model, hfov, r, poly, shift, crop = base[0].key
        pr, pc = photo_cached("ringing").shape[:2]
        out.append(Case("ringing" + name[len("64x48"):], "ringing", w, h, make_lens(pc, pr, model, hfov, r, poly, shift, crop, M.BICUBIC), ("ringing",) + base[0].key[1:]))
    return out


def clamp_counts(case):
    """(low, high): per channel (B, G, R, A) how many inside pixels of the case the model's sample clamps from below 0 and from above 255"""
    img = photo_cached(case.photo)
    fx, fy = model_coords(case)
    ok = M.inside(fx, fy, img.shape[1], img.shape[0], case.lens)
    raw = M.sample_raw(img, np.where(ok, fx, 0), np.where(ok, fy, 0), case.lens.filter)
    return [int(((raw[..., c] < 0) & ok).sum()) for c in range(4)], [int(((raw[..., c] > 255) & ok).sum()) for c in range(4)]


def all_outside_cases():
    """one per lens model: nothing of the canvas is inside.  The first two leave at the angle test (min_cos just below 1: no pixel
    centre lies on the axis), the other two at the image circle (one unit of 1/256 px wide, far from the photo)."""
    out = []
    pr, pc = photo_cached("64x48").shape[:2]
    for model, hfov in ((M.RECTILINEAR, 120.0), (M.EQUIDISTANT, 190.0), (M.STEREOGRAPHIC, 190.0), (M.EQUISOLID, 190.0)):
        lens = make_lens(pc, pr, model, hfov, "generic", 0, 0, 0, M.BICUBIC if model % 2 else M.BILINEAR)
        if model in (M.RECTILINEAR, M.EQUIDISTANT):
            lens.min_cos = 0.99999
        else:
            lens.crop = (-1000000, -1000000, 1)
        name = "all_outside_" + M.MODEL_NAMES[model]
        out.append(Case(name, "64x48", 90, 40, lens, (name,)))
    return out


def cases():
    """the list every test runs: the candidates with enough of the canvas on either side of the photo's edge, then the all-outside four"""
    if not _CASES:
        for c in candidates():
            if MIN_INSIDE <= inside_fraction(c) <= 1.0 - MIN_OUTSIDE:
                _CASES.append(c)
        _CASES.extend(all_outside_cases())
    return _CASES
