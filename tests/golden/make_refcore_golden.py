"""Regenerates tests/golden/refcore_*.npz: small inputs and what THE REFERENCE'S OWN TEXT computes for them.

Unlike make_golden.py these fixtures are not the oracle's: every output here comes from oracle/_ref/pano_ref_core, the reference's
translation units compiled unmodified against the OpenCV stand-in (make -C oracle refcore; oracle/refcore.py).  tests/test_gpu_refcore.py
holds the HIP path to them without any oracle call; tests/test_ref_core.py demands that the driver keep reproducing them.

Inputs are stored as small integer arrays (tests/refcore_cases.py decodes them) or as a synth seed plus the SHA-256 of the bytes it must
give.  Outputs are stored whole where the file stays under 1 MB, else as SHA-256 plus a 64 x 64 crop.  Run:
    python tests/golden/make_refcore_golden.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))
import refcore  # noqa: E402
import refcore_cases as rc  # noqa: E402

PAIRS = [(160, 128, 1234), (203, 131, 77)]           # cols, rows, synth seed
ALGS = [("low", 0), ("s20", 20)]
STITCH = "tall_even"                                  # the 400 x 800 canvas of refcore_cases.CANVASES
CROP = (300, 168)                                     # y0, x0 of the composite's 64 x 64 crop: across the overlap's left edge


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def make(synth):
    """{file name: {array name: array}} -- everything computed by the driver."""
    refcore.use_exe(None); refcore.reset_params()
    out = {}
    # adjustInitialFlow, 29 x 26, hints 1..4
    q = rc.adjust_case_q(29, 26, 7 * 29 + 26)
    I0, I1, a0, a1 = rc.img_f32(q["I0"]), rc.img_f32(q["I1"]), rc.img_f32(q["a0"]), rc.img_f32(q["a1"])
    d = dict(q)
    for hint in (1, 2, 3, 4):
        d["flow_h%d" % hint] = refcore.adjust_initial_flow(I0, I1, a0, a1, hint, 20)
    out["refcore_adjust_29x26.npz"] = d
    # one level with an incoming flow (presets, no search), and the coarsest-level form with hint LEFT (3) and the 20 % search
    for (w, h) in ((61, 45), (45, 61)):
        q = rc.level_case_q(w, h, 23 + h)
        I0, I1, a0, a1, fin = rc.decode_level(q)
        d = dict(q); d["flow"] = refcore.level(I0, I1, a0, a1, fin, 0, 0)
        out["refcore_level_%dx%d.npz" % (w, h)] = d
    # ... and the level with exactly tied proposals (smoothnessCoef 0): proposal order and the strict '<'
    q = rc.tie_case_q(61, 45, 61 + 61)
    I0, I1, a0, a1, fin = rc.decode_level(q)
    refcore.set_params(*rc.SET_TIES)
    d = dict(q); d["flow"] = refcore.level(I0, I1, a0, a1, fin, 0, 0); d["params"] = np.array(rc.SET_TIES, np.float32)
    refcore.reset_params()
    out["refcore_level_ties_61x45.npz"] = d
    q = rc.level_case_q(150, 131, 23 + 131)
    I0, I1, a0, a1, _ = rc.decode_level(q)
    d = {k: v for k, v in q.items() if k != "fin"}; d["flow"] = refcore.level(I0, I1, a0, a1, None, 3, 20)
    out["refcore_level_150x131_coarsest.npz"] = d
    # prepare (both flows) + combineNovelViews
    for cols, rows, seed in PAIRS:
        L, R, blend = synth.make_pair_np(cols, rows, seed)
        for name, pct in ALGS:
            f0, f1 = refcore.flow_bidir(L, R, pct)
            out["refcore_pair_%dx%d_%s.npz" % (cols, rows, name)] = dict(
                seed=np.int64(seed), in_sha=sha(L, R, blend), flowLR=f0, flowRL=f1, merged=refcore.combine_novel_views(L, R, f0, f1, blend))
    # one stitch step (CPU/main.cpp:70-95) on the 400 x 800 canvas
    L, R, _ = rc.canvas(synth, STITCH)
    mp, ovl, ovr, bl, md = refcore.stitch_prepare(L, R)
    f0, f1 = refcore.flow_bidir(ovl, ovr, 20)
    merged = refcore.combine_novel_views(ovl, ovr, f0, f1, bl)
    final = refcore.stitch_gather(L, R, merged, mp)
    assert rc.n150_near_border(rc.gather_map(mp, merged)) == 0
    y0, x0 = CROP
    out["refcore_stitch_400x800.npz"] = dict(in_sha=sha(L, R), map=mp, blend=bl, final_sha=sha(final), final_crop=final[y0:y0 + 64, x0:x0 + 64].copy(),
                                             merged_sha=sha(merged))
    return out


def main():
    from conftest import load_pkg_module
    for fname, arrays in make(load_pkg_module("synth")).items():
        p = os.path.join(HERE, fname)
        np.savez_compressed(p, **arrays)
        print(fname, os.path.getsize(p) // 1024, "KiB")
        assert os.path.getsize(p) < (1 << 20), fname


if __name__ == "__main__":
    main()
