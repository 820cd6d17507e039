"""Panoramas/s of the batched stitch step against sequential pf_stitch_step chains (on a machine with the GPU).

16 config-4 rigs (synth.make_stitch_set, seeds 1234+k, generated on the GPU) at 9000x4000, 5 steps each.  Legs, alternated in
one process after a warm-up round, >= 3 timed repeats each (host clock, ending in a device synchronise):
  seq       16 chains of pf_stitch_step one after the other (host images in, every composite out)
  dev<K>    pf_stitch_step_batch_dev at in_flight K (inputs resident, the 5 steps chained through per-step output buffers)
  host8     pf_stitch_step_batch at in_flight 8 (host images in, every composite out)
The warm-up round also checks every batched composite against the sequential chain's (SHA-256).
  python tests/micro/stitch_batch_rate.py [--reps 3] [--out profiles/stitch_batch_9000x4000.txt]
  python tests/micro/stitch_batch_rate.py --only dev8 --reps 1 --no-check     (the leg alone, e.g. under rocprofv3)"""
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
legs = ["seq", "dev1", "dev2", "dev4", "dev8", "dev16", "host8"]
if a.only:
    legs = a.only.split(",")
sha = lambda x: hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()

c = pf.Context(0)
t0 = time.perf_counter()
tops, imgs = [], []          # host copies (seq / host legs)
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


def run(leg, check=None):
    """one pass of a leg over all rigs; check = {(rig, step): sha} to verify against (or to fill, for seq)"""
    if leg == "seq":
        for k in range(NR):
            for i in range(STEPS):
                out = c.stitch_step(imgs[k][i], tops[k] if i == 0 else None, PCT, out=host_out[k])
                if check is not None:
                    check[(k, i)] = sha(out)
    elif leg.startswith("dev"):
        K = int(leg[3:])
        for i in range(STEPS):
            d_r = d_tops if i == 0 else [d_outs[k][i - 1] for k in range(NR)]
            c.stitch_step_batch_dev([d_imgs[k][i] for k in range(NR)], d_r, cols, rows, PCT, [d_outs[k][i] for k in range(NR)], in_flight=K)
        if check is not None:
            buf = np.empty((rows, cols, 4), np.uint8)
            for k in range(NR):
                for i in range(STEPS):
                    assert sha(c.download(buf, d_outs[k][i])) == check[(k, i)], "%s: rig %d step %d differs from its sequential chain" % (leg, k, i + 1)
    else:   # host form
        K = int(leg[4:])
        for i in range(STEPS):
            outs = c.stitch_step_batch([imgs[k][i] for k in range(NR)], tops if i == 0 else None, PCT, in_flight=K, out=host_out)
            if check is not None:
                for k in range(NR):
                    assert sha(outs[k]) == check[(k, i)], "%s: rig %d step %d differs from its sequential chain" % (leg, k, i + 1)
    sync()


ref = None if a.no_check else {}
for leg in (["seq"] if ref is not None and "seq" not in legs else []) + legs:   # warm-up round (+ the reference chain)
    t0 = time.perf_counter()
    run(leg, ref)
    print("warm-up %-6s %.2f s%s" % (leg, time.perf_counter() - t0, "" if ref is None else " (checked)"), flush=True)
times = {leg: [] for leg in legs}
for r in range(a.reps):
    for leg in legs:
        t0 = time.perf_counter()
        run(leg)
        times[leg].append(time.perf_counter() - t0)
    print("rep %d: %s" % (r + 1, "  ".join("%s %.3f s" % (leg, times[leg][-1]) for leg in legs)), flush=True)

lines = ["# stitch_batch_rate.py: %d config-4 rigs (seeds 1234..%d) at %dx%d, %d steps each, pixflow_search_20; %d timed repeats per leg, "
         "legs alternated in one process after a warm-up round" % (NR, 1234 + NR - 1, cols, rows, STEPS, a.reps),
         "# panoramas/s = rigs / wall time of the leg (host clock, ending in a device synchronise); spread = min..max over the repeats",
         "# every batched composite of the warm-up round %s" % ("was checked against its sequential chain (SHA-256): all equal" if ref is not None else "was NOT checked (--no-check)"),
         "%-7s %10s %10s %14s %9s" % ("leg", "median_s", "spread_s", "panoramas/s", "x seq")]
med = {leg: float(np.median(times[leg])) for leg in legs}
for leg in legs:
    x = med["seq"] / med[leg] if "seq" in med else float("nan")
    lines.append("%-7s %10.3f %4.3f..%4.3f %10.2f %9.2f" % (leg, med[leg], min(times[leg]), max(times[leg]), NR / med[leg], x))
print("\n".join(lines))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
for k in range(NR):
    for p in [d_tops[k]] + d_imgs[k] + d_outs[k]:
        c.dev_free(p)
c.close()
