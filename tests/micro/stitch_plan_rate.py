"""Panoramas/s of the planned batched stitch step against the unplanned one (on a machine with the GPU).

16 config-4 rigs (synth.make_stitch_set, seeds 1234+k, generated on the GPU) at 9000x4000, 5 steps each: the workload of
stitch_batch_rate.py.  All rigs share their masks, so one plan per step serves every frame.  Legs, alternated in one process after
a warm-up round, >= 3 timed repeats each (host clock, ending in a device synchronise):
  dev<K>    pf_stitch_step_batch_dev at in_flight K (inputs resident, the 5 steps chained through per-step output buffers)
  dev<K>p   the same through pf_stitch_step_batch_planned_dev; the plan of each step is made INSIDE the leg, once per step, from
            rig 0's resident images (pf_stitch_plan_create_dev), and destroyed after the step
  host8     pf_stitch_step_batch at in_flight 8 (host images in, every composite out)
  host8p    pf_stitch_step_batch_planned; the plan of each step is made inside the leg from rig 0's host images (its left image and
            the top image, then its previous composite: two uploads per step)
The warm-up round checks every planned composite against the unplanned leg's (SHA-256).
  python tests/micro/stitch_plan_rate.py [--reps 3] [--out profiles/stitch_plan_9000x4000.txt]
  python tests/micro/stitch_plan_rate.py --only dev8p --reps 1 --no-check     (the leg alone, e.g. under rocprofv3)"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

# a lane drives 3 streams, a context 2 more (blend ramp, copies): 8 hardware queues cover every leg here (read at HIP's initialisation)
os.environ["GPU_MAX_HW_QUEUES"] = "8"
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_pkg_module  # noqa: E402

import torch  # noqa: E402  (torch's HIP runtime first: conftest._torch_hip_first)
torch.cuda.init()
pf = load_pkg_module("pyabi")
synth = load_pkg_module("synth")

ap = argparse.ArgumentParser()
ap.add_argument("--cols", type=int, default=9000)
ap.add_argument("--rows", type=int, default=4000)
ap.add_argument("--rigs", type=int, default=16)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--only", default="")
ap.add_argument("--no-check", action="store_true")
ap.add_argument("--out", default="")
a = ap.parse_args()
cols, rows, NR, STEPS, PCT = a.cols, a.rows, a.rigs, 5, 20
nb = cols * rows * 4
legs = ["dev8", "dev8p", "dev16", "dev16p", "host8", "host8p"]
if a.only:
    legs = a.only.split(",")
sha = lambda x: hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()

c = pf.Context(0)
t0 = time.perf_counter()
tops, imgs = [], []          # host copies (host legs)
d_tops, d_imgs = [], []      # resident copies (dev legs)
for k in range(NR):
    t, ims = synth.make_stitch_set(cols, rows, 1234 + k, STEPS, "cuda")
    tops.append(t.cpu().numpy()); imgs.append([im.cpu().numpy() for im in ims])
    del t, ims
    d_tops.append(c.dev_alloc(nb)); c.upload(d_tops[-1], tops[-1])
    d_imgs.append([c.dev_alloc(nb) for _ in range(STEPS)])
    for i in range(STEPS):
        c.upload(d_imgs[-1][i], imgs[-1][i])
torch.cuda.empty_cache()
d_outs = [[c.dev_alloc(nb) for _ in range(STEPS)] for _ in range(NR)]
print("inputs: %d rigs of %dx%d x %d steps in %.1f s" % (NR, cols, rows, STEPS, time.perf_counter() - t0), flush=True)
sync = lambda: c._chk(c.l.pf_sync(c.h))
host_out = [np.empty((rows, cols, 4), np.uint8) for _ in range(NR)]
prev0 = np.empty((rows, cols, 4), np.uint8)   # host8p: rig 0's previous composite, the R of its next plan (host_out is rewritten by the step)


def run(leg, check=None, fill=None):
    """one pass of a leg over all rigs; check = {(rig, step): sha} to verify against, fill = the dict to record them in"""
    planned = leg.endswith("p")
    base = leg[:-1] if planned else leg
    shas = {}
    if base.startswith("dev"):
        K = int(base[3:])
        for i in range(STEPS):
            d_r = d_tops if i == 0 else [d_outs[k][i - 1] for k in range(NR)]
            plan = c.stitch_plan_dev(d_imgs[0][i], d_r[0], cols, rows) if planned else None
            c.stitch_step_batch_dev([d_imgs[k][i] for k in range(NR)], d_r, cols, rows, PCT, [d_outs[k][i] for k in range(NR)], in_flight=K, plan=plan)
            if planned:
                plan.close()
        if check is not None or fill is not None:
            buf = np.empty((rows, cols, 4), np.uint8)
            for k in range(NR):
                for i in range(STEPS):
                    shas[(k, i)] = sha(c.download(buf, d_outs[k][i]))
    else:   # host form
        K = int(base[4:])
        for i in range(STEPS):
            plan = c.stitch_plan(imgs[0][i], tops[0] if i == 0 else prev0) if planned else None
            outs = c.stitch_step_batch([imgs[k][i] for k in range(NR)], tops if i == 0 else None, PCT, in_flight=K, out=host_out, plan=plan)
            if planned:
                plan.close()
                if i + 1 < STEPS:
                    np.copyto(prev0, outs[0])
            if check is not None or fill is not None:
                for k in range(NR):
                    shas[(k, i)] = sha(outs[k])
    sync()
    if fill is not None:
        fill.update(shas)
    if check is not None:
        for key, h in shas.items():
            assert h == check[key], "%s: rig %d step %d differs from the unplanned leg's composite" % (leg, key[0], key[1] + 1)


refs = {}   # unplanned leg -> its composites' hashes
order = sorted(legs, key=lambda l: l.endswith("p"))   # warm-up: the unplanned legs first, they are the planned legs' reference
for leg in order:
    t0 = time.perf_counter()
    if a.no_check:
        run(leg)
    elif leg.endswith("p"):
        if leg[:-1] not in refs:
            refs[leg[:-1]] = {}
            run(leg[:-1], fill=refs[leg[:-1]])
        run(leg, check=refs[leg[:-1]])
    else:
        refs[leg] = {}
        run(leg, fill=refs[leg])
    print("warm-up %-7s %.2f s%s" % (leg, time.perf_counter() - t0, "" if a.no_check else " (hashed)"), flush=True)
times = {leg: [] for leg in legs}
for r in range(a.reps):
    for leg in legs:
        t0 = time.perf_counter()
        run(leg)
        times[leg].append(time.perf_counter() - t0)
    print("rep %d: %s" % (r + 1, "  ".join("%s %.3f s" % (leg, times[leg][-1]) for leg in legs)), flush=True)

lines = ["# stitch_plan_rate.py: %d config-4 rigs (seeds 1234..%d) at %dx%d, %d steps each, pixflow_search_20; %d timed repeats per leg, "
         "legs alternated in one process after a warm-up round" % (NR, 1234 + NR - 1, cols, rows, STEPS, a.reps),
         "# <leg>p = the planned form of <leg>; each of its steps makes its plan from rig 0 inside the timed region and destroys it",
         "# GPU_MAX_HW_QUEUES = 8 for every leg, planned or not (as stitch_batch_rate.py): the dev16 legs' two lanes drive more streams than "
         "that, so the absolute figures depend on the setting; each planned leg is compared with its unplanned leg under the same one",
         "# panoramas/s = rigs / wall time of the leg (host clock, ending in a device synchronise); spread = min..max over the repeats",
         "# every planned composite of the warm-up round %s" % ("was checked against the unplanned leg's (SHA-256): all equal" if not a.no_check else "was NOT checked (--no-check)"),
         "%-7s %10s %12s %12s %12s" % ("leg", "median_s", "spread_s", "panoramas/s", "x unplanned")]
med = {leg: float(np.median(times[leg])) for leg in legs}
for leg in legs:
    x = med[leg[:-1]] / med[leg] if leg.endswith("p") and leg[:-1] in med else float("nan")
    lines.append("%-7s %10.3f %5.3f..%5.3f %12.2f %12s" % (leg, med[leg], min(times[leg]), max(times[leg]), NR / med[leg], "" if x != x else "%.3f" % x))
print("\n".join(lines))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
for k in range(NR):
    for p in [d_tops[k]] + d_imgs[k] + d_outs[k]:
        c.dev_free(p)
c.close()
