"""The cases of tests/solver_param_cases.py do what they claim -- with the oracle alone, so that a pass of tests/test_gpu_solver_param_range.py
means something: the oracle's level count is the one listed, the result is finite (the overflow case: nowhere) and not the presets'
result, and the two guard sets put gated pixels on both sides of the boundary they are about while the oracle's sweep stays finite.

What the oracle gives (seed 7 pairs; w0 x h0 is level 0, the half-resolution plane with the novel-view pad):

  case                      image, max_pct   levels   max |flow|
  step 2^-16 / 2^16         200x160, 0       12       0.014 / 2.1e3
  step 2^-17 / 2^17         200x160, 0       12       0.0060 / 7.3e3
  step 49152                200x160, 0       12       1.5e3
  step 0                    200x160, 0       12       0 (all-zero flow)
  step 2^-140               200x160, 0       12       2.7e-42 (the flows themselves are denormal)
  (0.85, .., step 49152)    300x260, 0       11       4.3e3
  step 2^16 / 2^-16, search 300x260, 20      16       3.9e3 / 8.8
  (0.9, 10, 100, 100)       300x260, 0       16       11
  (0.9, 1e3, 1e6, 1e6)      300x260, 0       16       9.9e3
  (0.9, 1e-3, 1e-28, 3e-27) 300x260, 0       16       8.9
  (0.9, 1e-30, 1e-36, 1e-30) 200x160, 0      12       8.7
  pyr 0.25                  200x160, 0       1  (110x80)
  pyr 0.25                  420x400, 0       2  (231x200, 58x50)
  pyr 0.3                   640x560, 20      3  (352x280, 106x84, 32x25)
  presets                   148x128 / 162x142  10 / 11
  pyr nextafter(0.98f, 0)   300x260, 0       77
  pyr 0.975                 592x552 / 606x566  96 / 97
  pyr 0.98f                 200x160          1000 (a height of 25 from level 52 on, 25x25 from level 67 on)
  (0.9, 1e20, 1e25, 1e28)   200x160, 0       12       nothing finite

Guard sets, one sweep on 96x40 / 40x96 planes, 3805 gated pixels each (35 of the 3840 are not updated), forward and backward:
  straddle (0.9, 1e-3, 1e-28, 3e-27, 0.5): a regulariser operand below 2^-95 at 491 / 516 gated pixels, both at or above it at 3314 / 3289;
           no energy above 2^99; the oracle's output is finite (max |flow| 5.6)
  large    (0.9, 2e29, 0.01, 0.01, 0.5):   the energy above 2^99 at 404 / 411 gated pixels, at or below it at 3401 / 3394; no regulariser
           operand below 2^-95; the oracle's output is finite (max |flow| 1.0e29)"""
import numpy as np
import pytest

import solver_param_cases as sp


@pytest.fixture()
def orc_params(orc):
    yield orc
    orc.reset_params()


_preset = {}


def preset_flows(orc, synth, cols, rows, max_pct):
    key = (cols, rows, max_pct)
    if key not in _preset:
        orc.reset_params()
        L, R, _ = synth.make_pair_np(cols, rows, sp.SEED)
        _preset[key] = orc.flow_bidir(L, R, max_pct)
    return _preset[key]


SOLVES = dict(sp.STEP_CASES); SOLVES.update(sp.COEF_CASES); SOLVES.update(sp.LEVEL_CASES)


@pytest.mark.parametrize("name", list(SOLVES))
def test_solve_case_has_its_level_count_and_a_finite_result_of_its_own(orc_params, synth, name):
    orc = orc_params
    cols, rows, max_pct, pset, levels = SOLVES[name]
    preset = preset_flows(orc, synth, cols, rows, max_pct)
    L, R, _ = synth.make_pair_np(cols, rows, sp.SEED)
    orc.set_params(*pset)
    n, sizes = sp.oracle_levels(orc, cols, rows)
    assert n == levels, sizes
    f0, f1 = orc.flow_bidir(L, R, max_pct)
    assert np.isfinite(f0).all() and np.isfinite(f1).all()
    if pset != sp.PRESETS:
        assert not np.array_equal(f0, preset[0]) and not np.array_equal(f1, preset[1])
    if name == "step_0":
        assert not f0.any() and not f1.any()
    else:
        assert f0.any() and f1.any()


def test_level_geometry_of_the_named_cases(orc_params):
    orc = orc_params
    orc.set_params(*sp.pyr(0.25))
    assert sp.oracle_levels(orc, 200, 160) == (1, [(110, 80)])
    assert sp.oracle_levels(orc, 420, 400) == (2, [(231, 200), (58, 50)])
    assert sp.oracle_levels(orc, 420, 360)[0] == 2                      # the batch test's size
    orc.set_params(*sp.pyr(0.97))
    assert sp.oracle_levels(orc, 420, 360)[0] == 67
    for name, (cols, rows, _, pset, levels) in sp.REFUSED_CASES.items():
        orc.set_params(*pset)
        n, sizes = sp.oracle_levels(orc, cols, rows)
        assert n == levels, name
    # 0.98f: a side of 25 does not shrink any more (int(25 * 0.98f + 0.5f) is 25); the reference's list runs to its limit of 1000
    assert sizes[0] == (110, 80) and sizes[-1] == (25, 25) and sizes.count((25, 25)) > 900
    orc.set_params(*sp.pyr(sp.PYR_BELOW_098))
    assert sp.oracle_levels(orc, 200, 160)[0] == 53                     # the next float below ends the pyramid


def test_098_is_neither_the_presets_nor_the_next_float_below(orc_params, synth):
    """What a solve at 0.98f would have to match: the reference's 1000 levels give bits of their own."""
    orc = orc_params
    cols, rows, max_pct, pset, _ = sp.REFUSED_CASES["levels_1000"]
    preset = preset_flows(orc, synth, cols, rows, max_pct)
    L, R, _ = synth.make_pair_np(cols, rows, sp.SEED)
    orc.set_params(*pset)
    at = orc.flow_bidir(L, R, max_pct)
    orc.set_params(*sp.pyr(sp.PYR_BELOW_098))
    below = orc.flow_bidir(L, R, max_pct)
    assert np.isfinite(at[0]).all()
    assert not np.array_equal(at[0], preset[0]) and not np.array_equal(at[0], below[0]) and not np.array_equal(below[0], preset[0])


def test_overflow_case_is_nowhere_finite(orc_params, synth):
    orc = orc_params
    cols, rows, max_pct, pset, levels = sp.OVERFLOW_CASE
    L, R, _ = synth.make_pair_np(cols, rows, sp.SEED)
    orc.set_params(*pset)
    assert sp.oracle_levels(orc, cols, rows)[0] == levels
    f0, f1 = orc.flow_bidir(L, R, max_pct)
    assert not np.isfinite(f0).any() and not np.isfinite(f1).any()


@pytest.mark.parametrize("name", list(sp.LEVEL_STEP_SETS))
def test_level_case_is_finite_and_its_own(orc_params, synth, name):
    orc = orc_params
    planes = sp.level_planes(orc, synth)
    base = orc.level(*planes, 0, 0)
    orc.set_params(*sp.LEVEL_STEP_SETS[name])
    out = orc.level(*planes, 0, 0)
    assert np.isfinite(out).all() and not np.array_equal(out, base)


@pytest.mark.parametrize("w,h", sp.GUARD_SIZES)
@pytest.mark.parametrize("name", list(sp.GUARD_SETS))
def test_guard_set_puts_gated_pixels_on_both_sides_of_its_boundary(orc_params, name, w, h):
    orc = orc_params
    pset = sp.GUARD_SETS[name]
    assert pset[4] == 0.5       # a power-of-two step size: the fast form is live and the guard decides
    planes = sp.sweep_planes(orc, w, h)
    g0, g1, blurred, a0, a1, flow = planes
    assert np.abs(flow).max() < 10 and np.abs(flow)[np.abs(flow) > 0].min() > 1e-6     # nothing planted: ordinary flows
    preset = [orc.sweep(g0[..., 0], g0[..., 1], g1[..., 0], g1[..., 1], blurred, a0, a1, flow, fwd) for fwd in (1, 0)]
    orc.set_params(*pset)
    n = sp.guard_counts(orc, pset, planes)
    print(name, w, h, n)
    if name == "straddle":
        assert n["operand_below"] >= 50 and n["operand_at_or_above"] >= 50 and n["energy_above"] == 0
    else:
        assert n["energy_at_or_below"] >= 50 and n["energy_above"] >= 50 and n["operand_below"] == 0
    for i, fwd in enumerate((1, 0)):
        out = orc.sweep(g0[..., 0], g0[..., 1], g1[..., 0], g1[..., 1], blurred, a0, a1, flow, fwd)
        assert np.isfinite(out).all()
        assert not np.array_equal(out, preset[i])
