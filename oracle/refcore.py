"""Runs oracle/_ref/pano_ref_core: the reference's own translation units, compiled unmodified against the OpenCV stand-in
(oracle/cvstub) behind the driver oracle/ref_core_main.cpp.  Same call shapes as orc.py, so a test can put the two side by side.

TEST INFRASTRUCTURE ONLY.  The binary is built by `make -C oracle refcore` on a machine that has the reference's sources; it is
never committed.  Every call starts one process and exchanges flat binary files in a temporary directory.
"""
import os
import subprocess
import tempfile

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(_HERE, "_ref", "pano_ref_core")
REF_SRC = os.environ.get("PANO_REF_SRC", "/root/reference/CPU")
BUILD_CMD = "make -C oracle refcore"
PRESET = (0.9, 0.001, 0.01, 0.01, 0.5)   # pyrScaleFactor, smoothnessCoef, vertical / horizontal regularisation, gradientStepSize

_exe = EXE
_params = PRESET


def available():
    return os.path.exists(EXE)


def sources_present():
    return os.path.exists(os.path.join(REF_SRC, "PixFlow.hpp"))


def use_exe(path=None):
    """Run another build of the driver (the sanitized one); None = the default binary."""
    global _exe
    _exe = path or EXE


def set_params(pyr_scale=0.9, smoothness=0.001, vreg=0.01, hreg=0.01, step=0.5):
    global _params
    _params = (pyr_scale, smoothness, vreg, hreg, step)


def reset_params():
    set_params()


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _run(cmd, pct, ints, ins, outs):
    """ins: arrays; outs: list of (shape, dtype).  Returns the output arrays."""
    with tempfile.TemporaryDirectory(prefix="refcore_") as d:
        ipaths = []
        for i, a in enumerate(ins):
            p = os.path.join(d, "in%d.bin" % i); a.tofile(p); ipaths.append(p)
        opaths = [os.path.join(d, "out%d.bin" % i) for i in range(len(outs))]
        argv = [_exe, cmd, str(pct)] + ["%.9g" % np.float32(v) for v in _params] + [str(int(v)) for v in ints] + ipaths + opaths
        r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if r.returncode != 0:
            raise RuntimeError("%s %s failed with %d:\n%s" % (os.path.basename(_exe), cmd, r.returncode, r.stderr.decode(errors="replace")[-4000:]))
        res = []
        for p, (shape, dt) in zip(opaths, outs):
            a = np.fromfile(p, dtype=dt)
            res.append(a if shape is None else a.reshape(shape))
        return res


def pyramid_sizes_range(h, wlo, whi, pct=0):
    """[(w, h), ...] per width wlo..whi of PixFlow::buildPyramid on an h x w plane (sizes only: the resize arithmetic is skipped)."""
    flat, = _run("pyramid", pct, [h, wlo, whi], [], [(None, np.int32)])
    out = []; i = 0
    for _ in range(wlo, whi + 1):
        n = int(flat[i]); i += 1
        out.append([(int(flat[i + 2 * k]), int(flat[i + 2 * k + 1])) for k in range(n)]); i += 2 * n
    assert i == len(flat)
    return out


def error_function(I0x, I0y, I1x, I1y, blurred, cands, pct=0):
    """cands: (K, h, w, 2) candidate flows; returns (K, h, w) errors."""
    c = _f32(cands); K, h, w, _ = c.shape
    out, = _run("errfn", pct, [w, h, K], [_f32(I0x), _f32(I0y), _f32(I1x), _f32(I1y), _f32(blurred), c], [((K, h, w), np.float32)])
    return out


def patch_error(I0, a0, I1, a1, pts, pct=20):
    """pts: (N, 4) int32 rows of (i0x, i0y, i1x, i1y)."""
    I0 = _f32(I0); h, w = I0.shape
    p = np.ascontiguousarray(pts, dtype=np.int32)
    out, = _run("patcherr", pct, [w, h, len(p)], [I0, _f32(a0), _f32(I1), _f32(a1), p], [((len(p),), np.float32)])
    return out


def adjust_initial_flow(I0, I1, a0, a1, hint, max_pct):
    I0 = _f32(I0); h, w = I0.shape
    out, = _run("adjust", max_pct, [w, h, hint], [I0, _f32(I1), _f32(a0), _f32(a1)], [((h, w, 2), np.float32)])
    return out


def level(I0, I1, a0, a1, flow_in, hint, max_pct):
    I0 = _f32(I0); h, w = I0.shape
    ins = [I0, _f32(I1), _f32(a0), _f32(a1)] + ([] if flow_in is None else [_f32(flow_in)])
    out, = _run("level", max_pct, [w, h, hint, int(flow_in is not None)], ins, [((h, w, 2), np.float32)])
    return out


def diffusion(a0, a1, flow):
    f = _f32(flow); h, w, _ = f.shape
    out, = _run("diffusion", 0, [w, h], [_f32(a0), _f32(a1), f], [((h, w, 2), np.float32)])
    return out


def compute_optical_flow(bgra0, bgra1, max_pct, hint):
    a = _u8(bgra0); rows, cols, _ = a.shape
    out, = _run("cof", max_pct, [cols, rows, hint], [a, _u8(bgra1)], [((rows, cols, 2), np.float32)])
    return out


def flow_bidir(L, R, max_pct):
    """NovelViewGeneratorAsymmetricFlow::prepare through the reference's factory: presets only."""
    a = _u8(L); rows, cols, _ = a.shape
    f0, f1 = _run("prepare", max_pct, [cols, rows], [a, _u8(R)], [((rows, cols, 2), np.float32)] * 2)
    return f0, f1


def combine_novel_views(L, R, flowLtoR, flowRtoL, blend):
    a = _u8(L); rows, cols, _ = a.shape
    out, = _run("combine", 0, [cols, rows], [a, _u8(R), _f32(flowLtoR), _f32(flowRtoL), _f32(blend)], [((rows, cols, 4), np.uint8)])
    return out


def stitch_prepare(L, R):
    a = _u8(L); rows, cols, _ = a.shape
    return tuple(_run("stitch_prepare", 0, [cols, rows], [a, _u8(R)],
                      [((rows, cols), np.uint8), ((rows, cols, 4), np.uint8), ((rows, cols, 4), np.uint8), ((rows, cols), np.float32), ((rows, cols), np.float32)]))


def stitch_gather(L, R, merged, mp):
    a = _u8(L); rows, cols, _ = a.shape
    out, = _run("gather", 0, [cols, rows], [a, _u8(R), _u8(merged), _u8(mp)], [((rows, cols, 4), np.uint8)])
    return out
