"""Where a planned batch's time goes: kernel-family times (pf_profile_enable(1): events per family, summed over the group's streams)
of the device form at 8 in flight against its planned form, 8 config-4 rigs at 9000x4000, 5 steps, one group of 8 per step; each
form twice, alternated, an unprofiled pass (wall time) before each profiled one.  Companion of stitch_plan_rate.py, which measures
the rate; the planned form's countblend / tile_blur / box_blur / match_images are the plan creation of each step.
  python tests/micro/stitch_plan_families.py > profiles/stitch_plan_9000x4000_families.txt"""
import os, sys, time
import numpy as np
os.environ["GPU_MAX_HW_QUEUES"] = "8"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_pkg_module
import torch
torch.cuda.init()
pf = load_pkg_module("pyabi"); synth = load_pkg_module("synth")
cols, rows, NR, STEPS, PCT = 9000, 4000, 8, 5, 20
nb = cols * rows * 4
c = pf.Context(0)
d_tops, d_imgs = [], []
for k in range(NR):
    t, ims = synth.make_stitch_set(cols, rows, 1234 + k, STEPS, "cuda")
    d_tops.append(c.dev_alloc(nb)); c.upload(d_tops[-1], t.cpu().numpy())
    d_imgs.append([c.dev_alloc(nb) for _ in range(STEPS)])
    for i in range(STEPS):
        c.upload(d_imgs[-1][i], ims[i].cpu().numpy())
    del t, ims
torch.cuda.empty_cache()
d_outs = [[c.dev_alloc(nb) for _ in range(STEPS)] for _ in range(NR)]
def run(planned):
    t0 = time.perf_counter()
    for i in range(STEPS):
        d_r = d_tops if i == 0 else [d_outs[k][i - 1] for k in range(NR)]
        plan = c.stitch_plan_dev(d_imgs[0][i], d_r[0], cols, rows) if planned else None
        c.stitch_step_batch_dev([d_imgs[k][i] for k in range(NR)], d_r, cols, rows, PCT, [d_outs[k][i] for k in range(NR)], in_flight=8, plan=plan)
        if planned: plan.close()
    return time.perf_counter() - t0
run(False); run(True)
for planned in (False, True, False, True):
    w = run(planned)     # unprofiled wall time
    c.profile_enable(1); c.profile_reset()
    wp = run(planned)
    prof = c.profile(); c.profile_enable(0)
    print("planned" if planned else "unplanned", "wall %.3f s (profiled run %.3f s)" % (w, wp), flush=True)
    for name, (ms, n) in sorted(prof.items(), key=lambda kv: -kv[1][0]):
        if n: print("   %-22s %9.1f ms %6d launches" % (name, ms, n))
c.close()
