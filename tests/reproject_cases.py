"""Sources, outputs, rotations and filters shared by the reprojection tests (host-run kernels vs model, device vs model)."""
import numpy as np

import reproject_model as M
import resize_cases

FILTERS = [M.BILINEAR, M.BICUBIC]

# (name, cols, rows): a 2:1 sphere; 160 degrees of latitude (rays outside the coverage); an odd width with rows close to cols / 2;
# one image with every alpha class (a crop of the all-pairs image: alpha = row, colour = column)
SOURCES = ["64x32", "90x40", "67x33", "pairs"]


# a fifth source for a few BICUBIC cases: the opaque ringing image (resize_cases.ringing, 64 x 32, blocks of 2 x 2), whose taps overshoot in
# every channel, so that the sample's clamp to a byte works in both directions in all four byte positions.  Not in SOURCES: it rides on
# the cases below only.  The up face sees the pole, where the image's four bands meet (the side faces see two of them)
RINGING_MIN_CLAMPED = 10


def source(name):
    if name == "ringing":
        return resize_cases.ringing(64, 32, 2, 2)
    if name == "pairs":
        rows = list(range(0, 248, 8)) + [255]   # 64 x 32: alphas 0, 8, .. 240 and 255 against colours 0, 4, .. 252
        return np.ascontiguousarray(resize_cases.all_pairs()[rows][:, :256:4])
    cols, rows = (int(x) for x in name.split("x"))
    img = resize_cases.image(cols, rows)
    img[0, :, 3] = 255   # an opaque first row next to the transparent quadrant: the pole's clamped taps weigh something
    return img


# (projection, out_cols, out_rows, face, hfov): every face at sizes 1, 2, 7, 16 and 65 (one pixel past two workgroup tiles of 32);
# rectilinear views narrower and flatter than a tile; a sphere at 130 x 65, and at the source's size ("same")
CUBE_SIZES = [1, 2, 7, 16, 65]
OUTPUTS = [(M.CUBE, n, n, face, 0.0) for n in CUBE_SIZES for face in range(6)]
OUTPUTS += [(M.RECTILINEAR, w, h, 0, hfov) for (w, h) in ((65, 5), (33, 17)) for hfov in (90.0, 150.0)]
OUTPUTS += [(M.EQUIRECT, 0, 0, 0, 0.0), (M.EQUIRECT, 130, 65, 0, 0.0)]

# identity; a whole-column yaw (3 columns of a 64-wide source); a generic turn; the poles on the horizon and the seam through the image
ROTATIONS = {
    "identity": list(M.IDENTITY),
    "yaw3cols": M.rotation(3 * 360.0 / 64, 0.0, 0.0),
    "generic": M.rotation(37.0, -21.0, 11.0),
    "pitch90": M.rotation(0.0, 90.0, 0.0),
}


def cases():
    """(id, source name, projection, out_cols, out_rows, face, hfov, rotation name, filter)"""
    out = []
    for s in SOURCES:
        rows, cols = source(s).shape[:2]
        for (proj, w, h, face, hfov) in OUTPUTS:
            if proj == M.EQUIRECT and w == 0:
                w, h = cols, rows
            for r in ROTATIONS:
                for f in FILTERS:
                    name = "%s_p%d_%dx%d_f%d_h%g_%s_%s" % (s, proj, w, h, face, hfov, r, "cubic" if f == M.BICUBIC else "linear")
                    out.append((name, s, proj, w, h, face, hfov, r, f))
    return out


def ringing_cases():
    """the sphere at 130 x 65 and the up face at 65, both under the generic rotation, BICUBIC"""
    return [("ringing_p%d_%dx%d_f%d_h0_generic_cubic" % (proj, w, h, face), "ringing", proj, w, h, face, 0.0, "generic", M.BICUBIC)
            for (proj, w, h, face) in ((M.EQUIRECT, 130, 65, 0), (M.CUBE, 65, 65, M.UP))]


def clamp_counts(case):
    """(low, high): per channel (B, G, R, A) how many inside pixels of the case the model's sample clamps from below 0 and from above 255"""
    fx, fy = model_coords(case)
    img = source_cached(case[1])
    ok = M.inside(fy, img.shape[0])
    raw = M.sample_raw(img, fx, np.where(ok, fy, 0), case[8])
    return [int(((raw[..., c] < 0) & ok).sum()) for c in range(4)], [int(((raw[..., c] > 255) & ok).sum()) for c in range(4)]


_SOURCES = {}
_COORDS = {}
_IMAGES = {}


def source_cached(name):
    if name not in _SOURCES:
        _SOURCES[name] = source(name)
        _SOURCES[name].setflags(write=False)
    return _SOURCES[name]


def model_coords(case):
    """the model's (fx, fy) of a case, computed once (they do not depend on the pixels or the filter)"""
    _, s, proj, w, h, face, hfov, r, _ = case
    rows, cols = source_cached(s).shape[:2]
    k = (cols, rows, proj, w, h, face, hfov, r)
    if k not in _COORDS:
        fx, fy = M.coords(cols, rows, w, h, proj, face, hfov, ROTATIONS[r])
        fx.setflags(write=False); fy.setflags(write=False)
        _COORDS[k] = (fx, fy)
    return _COORDS[k]


def model_image(case):
    """the model's image of a case, computed once and shared between tests (read-only)"""
    if case[0] not in _IMAGES:
        fx, fy = model_coords(case)
        img = source_cached(case[1])
        out = M.sample(img, fx, np.where(M.inside(fy, img.shape[0]), fy, 0), case[8])
        out[~M.inside(fy, img.shape[0])] = 0
        out.setflags(write=False)
        _IMAGES[case[0]] = out
    return _IMAGES[case[0]]
