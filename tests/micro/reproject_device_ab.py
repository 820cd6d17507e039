"""The reprojection kernel at a user's sizes against the copy rate of the same box (profiles/reproject_device.txt).

Part 1: one 9000x4000 composite in HBM (the result of a stitch step on a config-4 rig, synth.make_stitch_set seed 1234), bicubic:
  cube     six faces of 2250 x 2250 in one launch (pf_reproject_cube_dev)
  level    the sphere turned at the canvas's size (yaw 37, pitch -21, roll 11; equirect to equirect)
  view     one 1920 x 1080 rectilinear view, hfov 90, the same turn
and the level case once more with the bilinear filter (4 taps instead of 16 on the same coordinates).
Three runs, the cases alternated; per case the kernel's time from the library's own events (family `reproject`), the host clock around the
call, and next to it a device-to-device copy that moves the same number of bytes as the kernel must (the source read once plus the
output written: a copy of half that many bytes reads and writes them), timed with events in the same run.  The view reads only the
part of the source it looks at, so its floor is an upper bound of the traffic.
Part 2 (--cli-runs N, default 0): wall time of the whole process `pano_stitch -test_dirs` over four config-4 rigs, -steps 2 -jpeg_device 1,
with and without -cube 2250, alternated.
  python tests/micro/reproject_device_ab.py [--cols 9000 --rows 4000] [--cli-runs 2] [--out profiles/reproject_device.txt]"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import PKG, load_pkg_module  # noqa: E402

import torch  # noqa: E402  (torch's HIP runtime first: conftest._torch_hip_first)
torch.cuda.init()
from PIL import Image  # noqa: E402
pf = load_pkg_module("pyabi")
synth = load_pkg_module("synth")

ap = argparse.ArgumentParser()
ap.add_argument("--cols", type=int, default=9000)
ap.add_argument("--rows", type=int, default=4000)
ap.add_argument("--face", type=int, default=2250)
ap.add_argument("--rigs", type=int, default=4)
ap.add_argument("--steps", type=int, default=2)
ap.add_argument("--cli-runs", type=int, default=0)
ap.add_argument("--out", default="")
a = ap.parse_args()
cols, rows, face = a.cols, a.rows, a.face
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return sorted(v)[len(v) // 2]


say("Reprojection of a %dx%d composite resident in HBM, bicubic, one MI355X: kernel time against a device-to-device copy of the same traffic" % (cols, rows))
c = pf.Context(0)
top, imgs = synth.make_stitch_set(cols, rows, 1234, 5, "cuda")
top = top.cpu().numpy(); imgs = [im.cpu().numpy() for im in imgs]
comp = c.stitch_step(imgs[0], top, 20)
del top, imgs
d_comp = c.dev_alloc(comp.nbytes)
c.upload(d_comp, comp)
turn = pf.reproject_rotation(37.0, -21.0, 11.0)
src_bytes = comp.nbytes

d_faces = [c.dev_alloc(face * face * 4) for _ in range(6)]
d_level = c.dev_alloc(comp.nbytes)
d_view = c.dev_alloc(1920 * 1080 * 4)
cases = [
    ("cube 6 x %d^2" % face, 6 * face * face * 4, lambda: c.reproject_cube_dev(d_comp, cols, rows, d_faces, face, pf.reproject_params(filter=pf.REPROJECT_BICUBIC))),
    ("level %dx%d" % (cols, rows), comp.nbytes,
     lambda: c.reproject_dev(d_comp, cols, rows, d_level, cols, rows, pf.reproject_params(projection=pf.PROJ_EQUIRECT, filter=pf.REPROJECT_BICUBIC, rot=turn))),
    ("level, bilinear", comp.nbytes,   # 4 taps instead of 16 on the same geometry: how the time splits between the coordinates and the taps
     lambda: c.reproject_dev(d_comp, cols, rows, d_level, cols, rows, pf.reproject_params(projection=pf.PROJ_EQUIRECT, filter=pf.REPROJECT_BILINEAR, rot=turn))),
    ("view 1920x1080", 1920 * 1080 * 4,
     lambda: c.reproject_dev(d_comp, cols, rows, d_view, 1920, 1080, pf.reproject_params(projection=pf.PROJ_RECTILINEAR, filter=pf.REPROJECT_BICUBIC, hfov_deg=90.0, rot=turn))),
]
pool = torch.empty(2 * src_bytes, dtype=torch.uint8, device="cuda")   # the copies' source and destination (the largest case moves 2 * src_bytes)


def copy_ms(nbytes):
    """a device-to-device copy that reads nbytes / 2 and writes nbytes / 2, by events; the best of five after a warm-up"""
    half = (nbytes // 2) & ~15
    src, dst = pool[:half], pool[half:2 * half]
    dst.copy_(src); torch.cuda.synchronize()
    best = None
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); dst.copy_(src); e1.record(); torch.cuda.synchronize()
        t = e0.elapsed_time(e1)
        best = t if best is None else min(best, t)
    return best


for name, out_bytes, call in cases:
    call()   # warm-up: tables, code objects
c.profile_enable(1)
say()
say("case                 run   kernel ms   call ms (host clock)   bytes moved (MB)   kernel GB/s   copy ms   kernel / copy")
res = {name: {"k": [], "h": [], "c": []} for name, _, _ in cases}
for run in range(3):
    for name, out_bytes, call in cases:
        moved = src_bytes + out_bytes
        c.profile_reset()
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        k_ms = c.profile()["reproject"][0]
        cp = copy_ms(moved)
        res[name]["k"].append(k_ms); res[name]["h"].append((t1 - t0) * 1e3); res[name]["c"].append(cp)
        say("%-20s %d   %9.3f   %9.3f              %9.1f          %9.0f   %7.3f   %6.2f" % (name, run + 1, k_ms, (t1 - t0) * 1e3, moved / 1e6, moved / 1e6 / k_ms, cp, k_ms / cp))
c.profile_enable(0)
say()
for name, out_bytes, _ in cases:
    r = res[name]
    say("%-20s median kernel %.3f ms (max - min %.3f), call %.3f ms, copy of the same traffic %.3f ms: kernel = %.2f x the copy; %.1f Mpx/s out" %
        (name, med(r["k"]), max(r["k"]) - min(r["k"]), med(r["h"]), med(r["c"]), med(r["k"]) / med(r["c"]), out_bytes / 4 / 1e6 / (med(r["k"]) * 1e-3)))
for d in d_faces + [d_level, d_view, d_comp]:
    c.dev_free(d)
c.close()
del comp, pool
torch.cuda.empty_cache()

if a.cli_runs > 0:
    say()
    say("2. pano_stitch -test_dirs over %d config-4 rigs, -steps %d -jpeg_device 1, pixflow_search_20, with and without -cube %d (wall seconds of the whole process, TIFF reads included)" %
        (a.rigs, a.steps, face))
    work = tempfile.mkdtemp(prefix="reproject_ab_")
    try:
        dirs = []
        for k in range(a.rigs):
            d = os.path.join(work, "rig%d" % k); os.makedirs(d); dirs.append(d)
            t, ims = synth.make_stitch_set(cols, rows, 1234 + k, 5, "cuda")
            Image.fromarray(t.cpu().numpy()[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(d, "top.tif"))
            for i in range(a.steps):
                Image.fromarray(ims[i].cpu().numpy()[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(d, "%d.tif" % (i + 1)))
            del t, ims
        torch.cuda.empty_cache()
        exe = os.path.join(PKG, "tools", "pano_stitch")
        wall = {"plain": [], "cube": []}
        for run in range(a.cli_runs):
            for leg, extra in (("plain", []), ("cube", ["-cube", str(face)])):
                for d in dirs:   # a leg counts its own files
                    for f in os.listdir(d):
                        if f.endswith(".jpg"):
                            os.remove(os.path.join(d, f))
                t0 = time.perf_counter()
                r = subprocess.run([exe, "-test_dirs", ",".join(dirs), "-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", str(a.steps), "-jpeg_device", "1"] + extra,
                                   capture_output=True, text=True)
                t1 = time.perf_counter()
                if r.returncode != 0:
                    say("%s run failed: %s" % (leg, r.stderr[-400:]))
                    raise SystemExit(1)
                wall[leg].append(t1 - t0)
                files = sum(len([f for f in os.listdir(d) if f.endswith(".jpg")]) for d in dirs)
                say("run %d %-6s %7.2f s   %d .jpg files in all rigs" % (run + 1, leg, t1 - t0, files))
        for leg in ("plain", "cube"):
            say("%-6s best %.2f s, worst %.2f s" % (leg, min(wall[leg]), max(wall[leg])))
        say("the six faces of every result (%d files of %dx%d) cost %.2f s of the run (difference of the best)" %
            (6 * a.steps * a.rigs, face, face, min(wall["cube"]) - min(wall["plain"])))
    finally:
        shutil.rmtree(work, ignore_errors=True)

if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
