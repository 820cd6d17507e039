"""Panoramas/s of the whole-chain call (pf_rig_stitch_batch*) against five planned batched steps (on a machine with the GPU).

16 config-4 rigs (synth.make_stitch_set, seeds 1234+k, generated on the GPU) at 9000x4000, 5 steps each: the workload of
stitch_plan_rate.py.  All rigs share their masks.  The plans of every leg are made BEFORE the timed region (their cost is reported on
its own, below), so the legs time the chains alone.  Legs, alternated in one process after a warm-up round, >= 3 timed repeats each
(host clock, ending in a device synchronise), K = in_flight:
  a_all<K>    five pf_stitch_step_batch_planned calls, every step's composite downloaded
  a_last<K>   the same, only the last step's composite downloaded
  b_all<K>    one pf_rig_stitch_batch call, every composite downloaded; plain uploads (pf_rig_set_upload_overlap 0): a wave that goes up a
              second time (the third and later waves of a call) does so between the waves
  b_last<K>   the same, only the last composite downloaded
  c_all<K>, c_last<K>   the same two with overlapped uploads (pf_rig_set_upload_overlap 1): that second upload runs on the copy stream
              while the wave before computes.  The two forms differ only where a call has more than two waves: 16 rigs at in_flight 4
  da<K>       five pf_stitch_step_batch_planned_dev calls (inputs resident, chained through per-step output buffers)
  db_all<K>   one pf_rig_stitch_batch_dev call, every d_out given
  db_last<K>  one pf_rig_stitch_batch_dev call, only the last d_out given (the others stay in the internal ping-pong planes)
The warm-up round compares every final composite with a_all's (SHA-256).  Plan cost: pf_rig_plan_create against five
pf_stitch_plan_create calls on the same masks, host images in.
  python tests/micro/rig_rate.py [--reps 3] [--out profiles/rig_9000x4000.txt]"""
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
ap.add_argument("--in-flight", default="4,8,16")
ap.add_argument("--out", default="")
a = ap.parse_args()
cols, rows, NR, STEPS, PCT = a.cols, a.rows, a.rigs, 5, 20
nb = cols * rows * 4
Ks = [int(k) for k in a.in_flight.split(",")]
legs = ["%s%d" % (name, K) for K in Ks for name in ("a_all", "a_last", "b_all", "b_last", "c_all", "c_last", "da", "db_all", "db_last")]
sha = lambda x: hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()

c = pf.Context(0)
t0 = time.perf_counter()
tops, imgs = [], []          # host copies (host legs)
d_tops, d_imgs = [], []      # resident copies (device legs)
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
host_out = [np.empty((rows, cols, 4), np.uint8) for _ in range(NR)]                 # a_*: one composite per rig, rewritten by every step
final_only = [[None] * (STEPS - 1) + [host_out[k]] for k in range(NR)]              # b_last
all_out = None                                                                       # b_all: allocated on first use (NR x STEPS composites)

# the plans, outside every timed region: rig 0's chain gives the R of each step's plan
comp0 = [c.stitch_step(imgs[0][i], tops[0] if i == 0 else None, PCT) for i in range(STEPS - 1)]
plan_R = [tops[0]] + comp0
plans = [c.stitch_plan(imgs[0][i], plan_R[i]) for i in range(STEPS)]
rig = c.rig_plan(tops[0], imgs[0])
for i in range(STEPS):
    m0, r0 = plans[i].download(); m1, r1 = rig.steps[i].download()
    assert np.array_equal(m0, m1) and np.array_equal(r0.view(np.uint32), r1.view(np.uint32)) and plans[i].overlap_px == rig.steps[i].overlap_px, "step %d: the rig's plan differs" % (i + 1)
plan_cost = {"5 x pf_stitch_plan_create": [], "pf_rig_plan_create": []}
for r in range(a.reps):
    t0 = time.perf_counter()
    tmp = [c.stitch_plan(imgs[0][i], plan_R[i]) for i in range(STEPS)]
    plan_cost["5 x pf_stitch_plan_create"].append(time.perf_counter() - t0)
    for p in tmp:
        p.close()
    t0 = time.perf_counter()
    tmp = c.rig_plan(tops[0], imgs[0])
    plan_cost["pf_rig_plan_create"].append(time.perf_counter() - t0)
    tmp.close()
del comp0


def run(leg, hashes=None):
    """one pass of a leg over all rigs; hashes = a dict that receives {rig: sha of its final composite}"""
    global all_out
    name = leg.rstrip("0123456789")
    K = int(leg[len(name):])
    if name in ("a_all", "a_last"):
        for i in range(STEPS):
            want = name == "a_all" or i == STEPS - 1
            c.stitch_step_batch([imgs[k][i] for k in range(NR)], tops if i == 0 else None, PCT, in_flight=K, plan=plans[i],
                                out=host_out if want else None, want_out=want)
        final = lambda k: host_out[k]
    elif name in ("b_last", "c_last"):
        c.rig_set_upload_overlap(name[0] == "c")
        c.rig_stitch_batch(rig, tops, imgs, PCT, in_flight=K, out=final_only)
        final = lambda k: host_out[k]
    elif name in ("b_all", "c_all"):
        c.rig_set_upload_overlap(name[0] == "c")
        if all_out is None:
            all_out = [[np.empty((rows, cols, 4), np.uint8) for _ in range(STEPS)] for _ in range(NR)]
        c.rig_stitch_batch(rig, tops, imgs, PCT, in_flight=K, out=all_out)
        final = lambda k: all_out[k][STEPS - 1]
    else:
        if name == "da":
            for i in range(STEPS):
                d_r = d_tops if i == 0 else [d_outs[k][i - 1] for k in range(NR)]
                c.stitch_step_batch_dev([d_imgs[k][i] for k in range(NR)], d_r, cols, rows, PCT, [d_outs[k][i] for k in range(NR)], in_flight=K, plan=plans[i])
        else:
            outs = d_outs if name == "db_all" else [[None] * (STEPS - 1) + [d_outs[k][STEPS - 1]] for k in range(NR)]
            c.rig_stitch_batch_dev(rig, d_tops, d_imgs, PCT, outs, in_flight=K)
        buf = np.empty((rows, cols, 4), np.uint8)
        final = lambda k: c.download(buf, d_outs[k][STEPS - 1])
    sync()
    if hashes is not None:
        for k in range(NR):
            hashes[k] = sha(final(k))


ref = {}
for n, leg in enumerate(legs):
    t0 = time.perf_counter()
    got = {}
    run(leg, got)
    if n == 0:
        ref = got
    for k in range(NR):
        assert got[k] == ref[k], "%s: rig %d's final composite differs from %s's" % (leg, k, legs[0])
    print("warm-up %-10s %.2f s (hashed)" % (leg, time.perf_counter() - t0), flush=True)
times = {leg: [] for leg in legs}
for r in range(a.reps):
    for leg in legs:
        t0 = time.perf_counter()
        run(leg)
        times[leg].append(time.perf_counter() - t0)
    print("rep %d: %s" % (r + 1, "  ".join("%s %.3f" % (leg, times[leg][-1]) for leg in legs)), flush=True)

lines = ["# rig_rate.py: %d config-4 rigs (seeds 1234..%d) at %dx%d, %d steps each, pixflow_search_20; %d timed repeats per leg, legs "
         "alternated in one process after a warm-up round; GPU_MAX_HW_QUEUES = 8" % (NR, 1234 + NR - 1, cols, rows, STEPS, a.reps),
         "# a_* = five pf_stitch_step_batch_planned calls, b_* / c_* = one pf_rig_stitch_batch call with plain / overlapped uploads (they differ "
         "only beyond two waves, i.e. at in_flight 4), da / db_* = the device forms;",
         "# _all = every step's composite delivered, _last = only the last one; the number = in_flight.  Plans are made outside the timed regions.",
         "# panoramas/s = rigs / wall time of the leg (host clock, ending in a device synchronise); spread = min..max over the repeats",
         "# every final composite of the warm-up round was checked against %s's (SHA-256): all equal" % legs[0],
         "%-10s %10s %14s %12s" % ("leg", "median_s", "spread_s", "panoramas/s")]
med = {leg: float(np.median(times[leg])) for leg in legs}
for leg in legs:
    lines.append("%-10s %10.3f %6.3f..%6.3f %12.2f" % (leg, med[leg], min(times[leg]), max(times[leg]), NR / med[leg]))
for K in Ks:
    for x, y in (("b_last", "a_last"), ("b_all", "a_all"), ("c_last", "b_last"), ("c_all", "b_all"), ("c_last", "a_last"), ("c_all", "a_all"), ("db_all", "da"), ("db_last", "da")):
        x, y = "%s%d" % (x, K), "%s%d" % (y, K)
        spread = max(max(times[x]) - min(times[x]), max(times[y]) - min(times[y]))
        lines.append("# %s - %s = %+.3f s (median), the run's spread %.3f s: %s" % (x, y, med[x] - med[y], spread,
                                                                                 "no slower" if med[x] - med[y] <= spread else "SLOWER"))
lines.append("%-28s %10s %14s" % ("plan cost (host images in)", "median_s", "spread_s"))
for name, ts in plan_cost.items():
    lines.append("%-28s %10.3f %6.3f..%6.3f" % (name, float(np.median(ts)), min(ts), max(ts)))
print("\n".join(lines))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
for k in range(NR):
    for p in [d_tops[k]] + d_imgs[k] + d_outs[k]:
        c.dev_free(p)
c.close()
