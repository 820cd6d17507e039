"""Host cost of the stitch calls, one leg of an A/B (profiles/stitch_host_ab.txt): the calls whose time is mostly the host part's
(csrc/pf_api_stitch.inl, pf_api_plan.inl), by host clock after a warm-up, and the kernel families each kind of call launches.

Timed (the median of --runs calls, --big-runs for the large canvas):
  step 240x200     pf_stitch_step with the next left image announced (pf_stitch_prefetch), so every call takes the prefetched copy and
                   uploads the next one beside its kernels; at this size the host's share of the call is largest
  step 2000x4000   the same on a strip of the flagship's size
  prepare 240x200  pf_stitch_prepare: two uploads, the match and the ramp, five downloads
  rig 3 waves      host-form pf_rig_stitch_batch, two steps, three frames one in flight: three waves, the third uploaded beside the second
Listed (pf_profile_enable): the kernel families and their launch counts of one pf_stitch_step, one pf_stitch_step_planned, one host-form
batch of three frames and one pf_rig_stitch of two steps.

  python tests/micro/stitch_host_ab.py --json leg.json          one leg: this tree's library through this tree's pyabi.py
  python tests/micro/stitch_host_ab.py --report --parent p1.json p2.json p3.json --branch b1.json b2.json b3.json [--out FILE]
The report: per case the parent's spread (max - min of its invocations' medians) and whether the branch's median of medians is at most
the parent's median plus that spread; then the two legs' family lists side by side."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=15)
ap.add_argument("--big-runs", type=int, default=5)
ap.add_argument("--json", default="")
ap.add_argument("--report", action="store_true")
ap.add_argument("--parent", nargs="*", default=[])
ap.add_argument("--branch", nargs="*", default=[])
ap.add_argument("--out", default="")
a = ap.parse_args()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return sorted(v)[len(v) // 2]


def report():
    legs = {"parent": [json.load(open(f)) for f in a.parent], "branch": [json.load(open(f)) for f in a.branch]}
    say("Host cost of the stitch calls before and after the host parts moved onto up_plane / down_plane, stitch_planes, plan_new / plan_free")
    say("and one clamp (tests/micro/stitch_host_ab.py).  Parent = a library built from the parent commit, driven through the parent's pyabi.py;")
    say("the kernels' objects are the same in both.  One MI355X, %d invocations per leg, alternated (parent, branch, parent, ...), each a" % len(legs["parent"]))
    say("fresh process that reports the median of its runs after a warm-up (host clock around the binding's call, ms).")
    say()
    say("%-18s %-7s %s   median of medians" % ("case", "leg", "invocation medians"))
    verdicts = []
    for case in legs["parent"][0]["ms"]:
        m = {leg: [r["ms"][case] for r in legs[leg]] for leg in legs}
        for leg in ("parent", "branch"):
            say("%-18s %-7s %s   %.4f" % (case, leg, "  ".join("%9.4f" % v for v in m[leg]), med(m[leg])))
        spread = max(m["parent"]) - min(m["parent"])
        ok = med(m["branch"]) <= med(m["parent"]) + spread
        verdicts.append(ok)
        say("%-18s parent's spread %.4f; branch - parent %+.4f ms: %s" % (case, spread, med(m["branch"]) - med(m["parent"]), "within the parent's spread or below it" if ok else "ABOVE the parent's spread"))
        say()
    say("all cases within the parent's spread or below it" if all(verdicts) else "at least one case above the parent's spread")
    say()
    say("Kernel families and launch counts (pf_profile_enable), first invocation of each leg")
    same = True
    for call in legs["parent"][0]["families"]:
        p, b = legs["parent"][0]["families"][call], legs["branch"][0]["families"][call]
        same = same and p == b
        say("%-22s parent  %s" % (call, "  ".join("%s %d" % (k, n) for k, n in sorted(p.items()))))
        say("%-22s branch  %s   %s" % ("", "  ".join("%s %d" % (k, n) for k, n in sorted(b.items())), "same" if p == b else "DIFFERENT"))
    say("same families and counts in every call" if same else "the legs launch different kernels")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if all(verdicts) and same else 1


if a.report:
    sys.exit(report())

import numpy as np  # noqa: E402

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_pkg_module  # noqa: E402
from rig_cases import PCT, window_set  # noqa: E402

pf = load_pkg_module("pyabi")


def timed(call, runs, warm=2):
    for _ in range(warm):
        call()
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return med(t)


def families(c, call):
    c.profile_enable(1); c.profile_reset()
    call()
    got = {k: n for k, (ms, n) in c.profile().items() if n}
    c.profile_enable(0)
    return got


def step_case(c, cols, rows, runs):
    """alternate two buffers of one image: each call finds its left image prefetched and uploads the other for the next"""
    top, Ls = window_set(cols, rows, 1, 5)
    left = [Ls[0], Ls[0].copy()]
    out = np.empty((rows, cols, 4), np.uint8)
    turn = [0]

    def call():
        k = turn[0]; turn[0] ^= 1
        c.stitch_prefetch(left[k ^ 1])
        c.stitch_step(left[k], top, PCT, out=out)
    return timed(call, runs)


res = {"ms": {}, "families": {}}
c = pf.Context(0)
cols, rows = 240, 200
top, Ls = window_set(cols, rows, 2, 41)
res["ms"]["step 240x200"] = step_case(c, cols, rows, a.runs)
res["ms"]["step 2000x4000"] = step_case(c, 2000, 4000, a.big_runs)
res["ms"]["prepare 240x200"] = timed(lambda: c.stitch_prepare(Ls[0], top), a.runs)
rg = c.rig_plan(top, Ls)
outs = [[np.empty((rows, cols, 4), np.uint8) for _ in range(2)] for _ in range(3)]
res["ms"]["rig 3 waves"] = timed(lambda: c.rig_stitch_batch(rg, [top] * 3, [Ls] * 3, PCT, in_flight=1, out=outs), a.runs)

plan = c.stitch_plan(Ls[0], top)
res["families"]["stitch_step"] = families(c, lambda: c.stitch_step(Ls[0], top, PCT))
res["families"]["stitch_step_planned"] = families(c, lambda: c.stitch_step(Ls[0], top, PCT, plan=plan))
res["families"]["batch of 3 (host)"] = families(c, lambda: c.stitch_step_batch([Ls[0]] * 3, [top] * 3, PCT, in_flight=3))
res["families"]["rig_stitch, 2 steps"] = families(c, lambda: c.rig_stitch_batch(rg, [top], [Ls], PCT, in_flight=1))
c.close()

for case, ms in res["ms"].items():
    say("%-18s median %.4f ms" % (case, ms))
for call, fam in res["families"].items():
    say("%-22s %s" % (call, "  ".join("%s %d" % (k, n) for k, n in sorted(fam.items()))))
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f)
