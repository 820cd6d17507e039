"""Run-time solver parameters (pf_set_solver_params) across their accepted range: the cases shared by tests/test_solver_param_cases.py
(the oracle alone: every case does what it claims) and tests/test_gpu_solver_param_range.py (the HIP path against the oracle, bit for bit).

A parameter set is (pyr_scale_factor, smoothness_coef, vertical_regularization_coef, horizontal_regularization_coef, gradient_step_size), the
order of oracle/orc.py's set_params; every whole-solve case runs on synth.make_pair_np(cols, rows, SEED)."""
import ctypes as C

import numpy as np

KEYS = ("pyr_scale_factor", "smoothness_coef", "vertical_regularization_coef", "horizontal_regularization_coef", "gradient_step_size")
PRESETS = (0.9, 0.001, 0.01, 0.01, 0.5)
SEED = 7
PYR_098 = float(np.float32(0.98))                                       # accepted by pf_set_solver_params, refused by every solve
PYR_BELOW_098 = float(np.nextafter(np.float32(0.98), np.float32(0)))   # the largest usable pyramid scale
TWO_M95 = np.float32(2.0 ** -95)    # operands below it (and not zero) leave the fast exact forms' range
TWO_99 = np.float32(2.0 ** 99)      # energies above it do


def kw(pset):
    return dict(zip(KEYS, pset))


def step(s, base=PRESETS):
    return base[:4] + (float(s),)


def pyr(p, base=PRESETS):
    return (float(p),) + base[1:]


def half_res(cols, rows):
    """Level 0 of a bidirectional solve (the novel-view pad of cols / 20 on either side)."""
    return int((cols + 2 * (cols // 20)) * 0.5), int(rows * 0.5)


def oracle_levels(orc, cols, rows):
    """Level count of the oracle's pyramid under the parameters it holds right now."""
    w0, h0 = half_res(cols, rows)
    ws = (C.c_int * 1024)(); hs = (C.c_int * 1024)()
    n = orc.lib().orc_pyramid_sizes(w0, h0, ws, hs, 1024)
    return n, [(ws[i], hs[i]) for i in range(min(n, 1024))]


# ---- whole solves: name -> (cols, rows, max_pct, parameter set, the oracle's level count) ----
# 1. the fast gradient step (one fused multiply-add, power-of-two step sizes 2^-16 .. 2^16) at the ends of its window, and just outside it
STEP_CASES = {
    "step_2^-16": (200, 160, 0, step(2.0 ** -16), 12),
    "step_2^16": (200, 160, 0, step(2.0 ** 16), 12),
    "step_2^-17": (200, 160, 0, step(2.0 ** -17), 12),            # outside: every step through the IEEE sequence
    "step_2^17": (200, 160, 0, step(2.0 ** 17), 12),
    "step_49152": (200, 160, 0, step(49152.0), 12),               # 1.5 * 2^15: large and no power of two
    "step_0": (200, 160, 0, step(0.0), 12),                       # no gradient step at all: the flow stays zero
    "step_2^-140": (200, 160, 0, step(2.0 ** -140), 12),          # a denormal step size
    "step_49152_odd_set": (300, 260, 0, (0.85, 0.0005, 0.0, 0.03, 49152.0), 11),
    "step_2^16_search": (300, 260, 20, step(2.0 ** 16), 16),
    "step_2^-16_search": (300, 260, 20, step(2.0 ** -16), 16),
}
# 2. coefficients that move the sweep's operands across the range guard, power-of-two step size (the fast form is live, the guard decides)
COEF_CASES = {
    "coef_10_100_100": (300, 260, 0, (0.9, 10.0, 100.0, 100.0, 0.5), 16),
    "coef_1e3_1e6_1e6": (300, 260, 0, (0.9, 1e3, 1e6, 1e6, 0.5), 16),
    "coef_1e-3_1e-28_3e-27": (300, 260, 0, (0.9, 1e-3, 1e-28, 3e-27, 0.5), 16),
    "coef_1e-30_1e-36_1e-30": (200, 160, 0, (0.9, 1e-30, 1e-36, 1e-30, 0.5), 12),
}
# 3. level counts the 0.9 pyramid never produces (and the two on either side of the solve's fine / coarse split, under the presets)
LEVEL_CASES = {
    "levels_1": (200, 160, 0, pyr(0.25), 1),                      # no upsample at all
    "levels_2": (420, 400, 0, pyr(0.25), 2),                      # 231x200 and 58x50: 4x upsample
    "levels_3": (640, 560, 20, pyr(0.3), 3),
    "levels_10": (148, 128, 0, PRESETS, 10),                      # split == 0
    "levels_11": (162, 142, 0, PRESETS, 11),                      # split == 8
    "levels_77": (300, 260, 0, pyr(PYR_BELOW_098), 77),
    "levels_96": (592, 552, 0, pyr(0.975), 96),                   # the level table is full
}
REFUSED_CASES = {
    "levels_97": (606, 566, 0, pyr(0.975), 97),
    "levels_1000": (200, 160, 0, pyr(PYR_098), 1000),             # a side of 25 no longer shrinks: the reference solves 1000 levels
}
# 5. every energy overflows: the oracle's flow is non-finite everywhere
OVERFLOW_CASE = (200, 160, 0, (0.9, 1e20, 1e25, 1e28, 0.5), 12)
# the stitch step's set
STITCH_SET = (0.8, 0.002, 0.02, 0.005, 2.0 ** -3)


# ---- one level on explicit planes (stage_level), as tests/test_gpu_solver_params.py builds them ----
def level_planes(orc, synth):
    rng = np.random.default_rng(5)
    w, h = 233, 141
    L, R, _ = synth.make_pair_np(2 * w, 2 * h, 31)
    I0, a0 = orc.preprocess(L); I1, a1 = orc.preprocess(R)
    I0, a0, I1, a1 = I0[:h, :w].copy(), a0[:h, :w].copy(), I1[:h, :w].copy(), a1[:h, :w].copy()
    fin = (rng.standard_normal((h, w, 2)) * 1.5).astype(np.float32)
    return I0, I1, a0, a1, fin


LEVEL_STEP_SETS = {"2^-16": step(2.0 ** -16), "2^16": step(2.0 ** 16), "49152": step(49152.0)}
SWEEP_FORMS = {"latency": dict(), "throughput": dict(sweep_wide=2), "lab_v1": dict(exp=True, sweep_impl=1)}


# ---- one sweep on explicit planes (stage_sweep): the range guard under coefficients ----
# The planes of tests/test_gpu_stages.py's test_sweep_operands_outside_fast_math_range WITHOUT its planted values: ordinary flows of a
# pixel or two, so that whatever leaves the fast forms' range does so because of the coefficients.
#   straddle: vreg * |flow.y| lies below 2^-95 where |flow.y| < 0.2524 and above elsewhere; fast and IEEE steps alternate inside one sweep
#   large:    the energy is the smoothness term, 2e29 * |blurred - flow|, above 2^99 where |blurred - flow| > 3.17; every operand of the
#             energy itself stays in range there, so it is the guard on the ENERGIES that decides
GUARD_SETS = {"straddle": (0.9, 1e-3, 1e-28, 3e-27, 0.5), "large": (0.9, 2e29, 0.01, 0.01, 0.5)}
GUARD_SIZES = ((96, 40), (40, 96))


def sweep_planes(orc, w, h):
    r = np.random.default_rng(11 + w)
    img0 = r.random((h, w)).astype(np.float32); img1 = r.random((h, w)).astype(np.float32)
    g0 = np.stack(orc.gradients(img0), -1); g1 = np.stack(orc.gradients(img1), -1)
    flow = (r.standard_normal((h, w, 2)) * 1.5).astype(np.float32)
    blurred = orc.gaussian_blur(flow, 15, 8.0)
    a0 = np.ones((h, w), np.float32); a1 = np.ones((h, w), np.float32)
    a0[h // 4:h // 4 + 5, w // 3:w // 3 + 7] = 0.5          # a few pixels that are not updated
    return g0, g1, blurred, a0, a1, flow


def guard_counts(orc, pset, planes):
    """Gated pixels of the incoming flow on either side of the two boundaries, under the parameters `pset` (which the oracle must hold):
    a regulariser operand (coefficient * |flow component|, float32 as the kernel and the reference form it) below / at or above 2^-95, and the
    oracle's energy of the pixel's own flow at or below / above 2^99."""
    g0, g1, blurred, a0, a1, flow = planes
    gated = (a0 > np.float32(0.9)) & (a1 > np.float32(0.9))
    av = np.float32(pset[2]) * np.abs(flow[..., 1]); ah = np.float32(pset[3]) * np.abs(flow[..., 0])
    below = ((av != 0) & (av < TWO_M95)) | ((ah != 0) & (ah < TWO_M95))
    e = orc.error_function(g0[..., 0], g0[..., 1], g1[..., 0], g1[..., 1], blurred, flow)
    return dict(gated=int(gated.sum()), operand_below=int((gated & below).sum()), operand_at_or_above=int((gated & ~below).sum()),
                energy_at_or_below=int((gated & (e <= TWO_99)).sum()), energy_above=int((gated & (e > TWO_99)).sum()))


def float_class(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN, per element."""
    a = np.asarray(a, np.float32)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0))).astype(np.uint8)
