"""The numpy model of the lens remap (tests/lens_model.py) held to what it does not restate: its positions to a plain
libm evaluation of each lens model at the largest photo sides, its conventions to the reprojection's (a rectilinear view rendered by
tests/reproject_model.py and remapped by a rectilinear lens lands on itself), the optical axis to the shifted centre, and the
degenerate rays to defined results.  The case list every other lens test runs (tests/lens_cases.py) is checked here too: a kernel
that writes zeros, or never does, cannot pass it."""
import math

import numpy as np
import pytest

import lens_cases
import lens_model as M
import reproject_model as R

POSES = [(0.0, 0.0, 0.0), (37.0, -21.0, 11.0), (0.0, 90.0, 0.0), (180.0, 0.0, 0.0)]


def _libm_position(model, focal_px, poly, shift, rot, photo_cols, photo_rows, d):
    """one ray through math.atan2 / sqrt / tan / sin: theta from the axis, the model's r(theta), the polynomial, the position"""
    c = [sum(rot[3 * i + j] * d[j] for j in range(3)) for i in range(3)]
    rho = math.sqrt(c[1] * c[1] + c[2] * c[2])
    theta = math.atan2(rho, c[0])
    r = focal_px * {M.RECTILINEAR: lambda t: math.tan(t), M.EQUIDISTANT: lambda t: t, M.STEREOGRAPHIC: lambda t: 2.0 * math.tan(t / 2.0),
                    M.EQUISOLID: lambda t: 2.0 * math.sin(t / 2.0)}[model](theta)
    rn = r / (min(photo_cols, photo_rows) / 2.0)
    a, b, cc = poly
    r_src = r * (a * rn ** 3 + b * rn ** 2 + cc * rn + (1.0 - (a + b + cc)))
    k = r_src / rho if rho else 0.0
    return (photo_cols / 2.0 - 0.5 + shift[0]) + k * c[1], (photo_rows / 2.0 - 0.5 + shift[1]) - k * c[2]


@pytest.mark.parametrize("model,hfov", lens_cases.LENSES)
def test_positions_equal_a_libm_evaluation_within_2_pow_minus_20(model, hfov):
    """The arctangent is good to 1e-15 rad (tests/test_reproject_model.py) and focal_px is below 65535, so the model's position differs
    from libm's by something of order 1e-10 px; the bound is 2^-20 px.  Compared where the position lies on the photo or within one
    photo side of it: further out nothing is sampled, and a rectilinear radius grows without bound towards 90 degrees."""
    d = M.canvas_rays(90, 40)
    flat = [x.ravel() for x in d]
    worst, compared = 0.0, 0
    for (pc, pr) in ((65535, 65535), (65535, 4001), (4001, 65535)):
        for pose, poly, shift in zip(POSES, ((0.0, 0.0, 0.0), lens_cases.POLYNOMIAL) * 2, ((0.0, 0.0), (0.0, 0.0), lens_cases.SHIFT, lens_cases.SHIFT)):
            f = M.focal(model, pc, hfov)
            lens = M.Lens(model, f, a=poly[0], b=poly[1], c=poly[2], dd=1.0 - sum(poly), shift_x=shift[0], shift_y=shift[1], rot=M.rotation(*pose))
            with np.errstate(all="ignore"):
                px, py, seen = M.photo_position(d, lens, pc, pr)
            px, py, seen = px.ravel(), py.ravel(), seen.ravel()
            for at in np.flatnonzero(seen):
                want = _libm_position(model, f, poly, shift, lens.rot, pc, pr, [x[at] for x in flat])
                if -pc <= want[0] <= 2 * pc and -pr <= want[1] <= 2 * pr:
                    worst = max(worst, abs(px[at] - want[0]), abs(py[at] - want[1]))
                    compared += 1
    print("model %d hfov %g: %d positions, worst difference %.3g px" % (model, hfov, compared, worst))
    assert compared > 1000
    assert worst <= 2.0 ** -20


@pytest.mark.parametrize("hfov", [60.0, 120.0])
@pytest.mark.parametrize("pose", POSES)
def test_a_rectilinear_view_of_the_reprojection_lands_on_itself(pose, hfov):
    """the world direction of view pixel (u, v) of reproject_model, rotation Rm and hfov, is at photo position (u, v) under a
    rectilinear lens with rot = Rm transposed and focal = pf_lens_focal: the frame, the axes, the half-pixel centres and the meaning of
    hfov are the reprojection's"""
    w, h = 67, 33
    Rm = R.rotation(*pose)
    dv = R.rays(R.RECTILINEAR, w, h, hfov_deg=hfov)
    world = [(Rm[3 * i] * dv[0] + Rm[3 * i + 1] * dv[1]) + Rm[3 * i + 2] * dv[2] for i in range(3)]
    lens = M.Lens(M.RECTILINEAR, M.focal(M.RECTILINEAR, w, hfov), rot=M.rotation(*pose))
    px, py, seen = M.photo_position(world, lens, w, h)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    assert seen.all()
    assert np.abs(px - u).max() <= 1e-9 and np.abs(py - v).max() <= 1e-9


@pytest.mark.parametrize("model", [M.EQUIDISTANT, M.STEREOGRAPHIC, M.EQUISOLID])
@pytest.mark.parametrize("pose", POSES)
def test_a_fisheyes_axis_lands_on_the_shifted_centre(model, pose):
    pc, pr = 33, 67
    Rm = R.rotation(*pose)
    axis = [np.array([Rm[0]]), np.array([Rm[3]]), np.array([Rm[6]])]   # the camera's +x in the world: the pose's first column
    lens = M.Lens(model, M.focal(model, pc, 190.0), a=0.01, b=-0.05, c=0.02, dd=1.02, shift_x=1.5, shift_y=-2.25, rot=M.rotation(*pose))
    px, py, seen = M.photo_position(axis, lens, pc, pr)
    assert seen.all()
    assert abs(px[0] - (pc / 2.0 - 0.5 + 1.5)) <= 1e-9 and abs(py[0] - (pr / 2.0 - 0.5 - 2.25)) <= 1e-9


@pytest.mark.parametrize("model", range(4))
def test_degenerate_rays_have_defined_results(model):
    pc, pr = 64, 48
    # exactly on the axis (rho == 0); the null ray (n == 0); exactly backwards (n + c.x == 0)
    d = [np.array([1.0, 0.0, -1.0]), np.array([0.0, 0.0, 0.0]), np.array([0.0, 0.0, 0.0])]
    for min_cos in (None, -1.0) if model != M.RECTILINEAR else (None,):
        lens = M.Lens(model, M.focal(model, pc, 120.0), a=0.01, b=-0.05, c=0.02, dd=1.02, min_cos=min_cos)
        fx, fy = M.coords_of_rays(d, pc, pr, lens)
        assert (fx[0], fy[0]) == (256 * 32 - 128 + 0, 256 * 24 - 128 + 0)   # floor(256 (cols / 2 - 1/2) + 1/2): the centre, no NaN from 0 / 0
        for k in (1, 2):
            assert (fx[k], fy[k]) == (0, -2 ** 31), (model, min_cos, k)
        assert not M.inside(fx[1:], fy[1:], pc, pr, lens).any() and M.inside(fx[:1], fy[:1], pc, pr, lens).all()


def test_the_image_circle_is_compared_without_overflow():
    lens = M.Lens(M.EQUIDISTANT, 10.0, crop=(2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1))
    fx = np.array([0, 256 * 65534 + 128], np.int32); fy = np.array([256 * 65534 + 128, 0], np.int32)
    # both differences are near 2^31: the squares' sum is near 2^63 and above the radius's square
    assert not M.inside(fx, fy, 65535, 65535, lens).any()
    lens.crop = (0, 0, 2 ** 31 - 1)
    assert M.inside(fx, fy, 65535, 65535, lens).all()


def test_focal_and_rotation_conventions():
    for model in range(4):   # half the width at half the field of view, by the model's own r(theta)
        f = M.focal(model, 1000, 100.0)
        t = math.radians(50.0)
        r = f * (math.tan(t), t, 2.0 * math.tan(t / 2.0), 2.0 * math.sin(t / 2.0))[model]
        assert abs(r - 500.0) < 1e-9
    Rm, Rt = R.rotation(37.0, -21.0, 11.0), M.rotation(37.0, -21.0, 11.0)
    assert all(Rt[3 * i + j] == Rm[3 * j + i] for i in range(3) for j in range(3))


def test_the_case_list_cannot_be_passed_by_zeros_and_keeps_every_option():
    cases = lens_cases.cases()
    named = [c for c in cases if c.name.startswith("all_outside_")]
    assert sorted(c.lens.model for c in named) == [0, 1, 2, 3]
    for c in named:
        assert lens_cases.inside_fraction(c) == 0.0 and not lens_cases.model_image(c).any(), c.name
    rest = [c for c in cases if c not in named]
    assert 800 <= len(rest) <= 1152 and len({c.name for c in cases}) == len(cases)
    for c in rest:
        f = lens_cases.inside_fraction(c)
        assert 0.10 <= f <= 0.90, (c.name, f)
        assert lens_cases.model_image(c).any(), c.name
    seen = lambda fn: {fn(c) for c in rest}
    assert seen(lambda c: c.photo) == set(lens_cases.PHOTOS)
    assert seen(lambda c: (c.cols, c.rows)) == set(lens_cases.CANVASES)
    assert seen(lambda c: (c.key[3], c.key[4])) == set(lens_cases.LENSES)
    assert seen(lambda c: c.key[5]) == set(lens_cases.ROTATIONS)
    for lens_key in lens_cases.LENSES:   # every lens with both filters and both values of each option
        mine = [c for c in rest if (c.key[3], c.key[4]) == lens_key]
        assert {c.lens.filter for c in mine} == set(lens_cases.FILTERS)
        for opt in (6, 7, 8):
            assert {c.key[opt] for c in mine} == {0, 1}, (lens_key, opt)
