"""What a rig plan rests on, pinned against the CPU oracle: the R mask of step i of a chain is top | L_1 | .. | L_{i-1}, so the map and
the smoothed ramp of every step follow from the n + 1 input masks -- a step prepared against a stand-in R with that alpha has the map and
the ramp of the real 5-step oracle chain -- and the region codes k_rig_maps computes (restated in numpy) are those maps.  Plus: the
library loads and resolves the rig entry points without a device."""
import ctypes

import numpy as np
import pytest

from rig_cases import COLS, PCT, ROWS, SEED_A, rig, rig_codes, stand_ins

OVERLAPS = (3536, 8976, 8806, 8806, 14246)   # code-150 pixels per step of this set


@pytest.fixture(scope="module")
def chain(orc, synth):
    """the real oracle chain of seed 1234: (map, ramp) per step"""
    top, imgs = rig(synth, COLS, ROWS, SEED_A)
    R = top
    steps = []
    for L in imgs:
        mp, ovl, ovr, blend, _ = orc.stitch_prepare(L, R, True)
        f0, f1 = orc.flow_bidir(ovl, ovr, PCT)
        R = orc.stitch_gather(L, R, orc.combine_novel_views(ovl, ovr, f0, f1, blend), mp)
        steps.append((mp, blend))
    return top, imgs, steps


def test_stand_in_masks_give_the_chain_s_maps_and_ramps(orc, chain):
    top, imgs, steps = chain
    for i, (L, R) in enumerate(zip(imgs, stand_ins(top, imgs))):
        mp, _, _, blend, _ = orc.stitch_prepare(L, R, True)
        assert np.array_equal(mp, steps[i][0]), "step %d: %d map codes differ from the chain's" % (i + 1, int((mp != steps[i][0]).sum()))
        assert np.array_equal(blend.view(np.uint32), steps[i][1].view(np.uint32)), "step %d: the ramp differs from the chain's" % (i + 1)


def test_numpy_region_codes_are_the_chain_s_maps(chain):
    top, imgs, steps = chain
    codes = rig_codes(top, imgs)
    for i in range(5):
        assert np.array_equal(codes[i], steps[i][0]), "step %d: %d codes differ" % (i + 1, int((codes[i] != steps[i][0]).sum()))
    # every step has overlap: the case checks something
    assert tuple(int((m == 150).sum()) for m, _ in steps) == OVERLAPS


def test_rig_symbols_resolve_without_a_device(pf):
    pf.build()
    lib = ctypes.CDLL(pf.SO_PATH)
    names = ["pf_rig_plan_create", "pf_rig_plan_create_dev", "pf_rig_plan_destroy", "pf_rig_plan_info", "pf_rig_plan_step",
             "pf_rig_stitch_batch", "pf_rig_stitch_batch_dev", "pf_rig_stitch", "pf_rig_stitch_dev", "pf_rig_set_upload_overlap"]
    for n in names:
        assert hasattr(lib, n), n
        assert n in pf.EXPORTS
    for n in ("RigPlan",):
        assert hasattr(pf, n)
    for n in ("rig_plan", "rig_plan_dev", "rig_stitch_batch", "rig_stitch_batch_dev"):
        assert hasattr(pf.Context, n)
    # argument errors that need no device
    assert lib.pf_rig_plan_info(None, None, None, None) == -1
    lib.pf_rig_plan_step.restype = ctypes.c_void_p
    assert lib.pf_rig_plan_step(None, None, 0) is None
