"""The device PNG encoder against the default path, on a machine with the GPU (profiles/png_device_ab.txt).

Part 1: one 9000x4000 composite resident in HBM (the result of a stitch step on a config-4 rig, synth.make_stitch_set seed 1234), three
runs of each path, alternated, host clock:
  default   pf_download of the raw composite, then the default writer's work on it (tools/image_io.hpp write_png: BGRA -> filter byte 0 +
            RGBA on one thread, one zlib level-1 stream; redone here with numpy and the same zlib call, the parts timed apart)
  device    pf_stitch_result_png (filter, deflate and compaction in kernels, the file's payload down, framing on the host); the kernels'
            share comes from the library's own event timing in a fourth run
Part 2: wall time of `pano_stitch -test_dirs` over four config-4 rigs, with and without -png_device 1, alternated, `--cli-runs` runs each.
  python tests/micro/png_device_ab.py [--cols 9000 --rows 4000] [--steps 2] [--cli-runs 2] [--out profiles/png_device_ab.txt]"""
import argparse
import io
import os
import shutil
import subprocess
import sys
import tempfile
import time
import zlib

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
ap.add_argument("--steps", type=int, default=2)
ap.add_argument("--rigs", type=int, default=4)
ap.add_argument("--cli-runs", type=int, default=2)
ap.add_argument("--out", default="")
a = ap.parse_args()
cols, rows = a.cols, a.rows
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


say("Device PNG encoder against the default path: %dx%d, one MI355X" % (cols, rows))
c = pf.Context(0)
top, imgs = synth.make_stitch_set(cols, rows, 1234, 5, "cuda")
top = top.cpu().numpy(); imgs = [im.cpu().numpy() for im in imgs]
comp = c.stitch_step(imgs[0], top, 20)
d_comp = c.dev_alloc(comp.nbytes)
c.upload(d_comp, comp)
c.stitch_result_png()   # warm-up: the encoder's scratch is allocated here
host = np.empty_like(comp)

say()
say("1. One composite resident in HBM (seconds; %d bytes raw)" % comp.nbytes)
say("run  default: download  swizzle  zlib-1    total   file bytes | device: pf_stitch_result_png   file bytes")
tot = {"default": [], "device": []}
for run in range(3):
    t0 = time.perf_counter()
    c.download(host, d_comp)
    t1 = time.perf_counter()
    raw = np.zeros((rows, cols * 4 + 1), np.uint8)
    raw[:, 1:].reshape(rows, cols, 4)[...] = host[..., [2, 1, 0, 3]]
    t2 = time.perf_counter()
    z = zlib.compress(raw, 1)
    t3 = time.perf_counter()
    nfile = len(z) + 8 + 25 + 12 + 12
    t4 = time.perf_counter()
    data = c.stitch_result_png()
    t5 = time.perf_counter()
    tot["default"].append(t3 - t0); tot["device"].append(t5 - t4)
    say("%d    %17.3f %8.3f %7.3f %8.3f %12d | %28.3f %12d" % (run + 1, t1 - t0, t2 - t1, t3 - t2, t3 - t0, nfile, t5 - t4, len(data)))
assert np.array_equal(np.array(Image.open(io.BytesIO(data)))[..., [2, 1, 0, 3]], comp), "the device file does not decode to the composite"
for k in ("default", "device"):
    v = sorted(tot[k])
    say("%-8s median %.3f s, max - min %.3f s" % (k, v[1], v[2] - v[0]))
say("ratio of the medians: %.1f;  file sizes: default %.4f of raw, device %.4f of raw" % (sorted(tot["default"])[1] / sorted(tot["device"])[1], nfile / comp.nbytes, len(data) / comp.nbytes))
c.profile_enable(1); c.profile_reset()
t0 = time.perf_counter(); c.stitch_result_png(); t1 = time.perf_counter()
prof = c.profile()
say("where the device path's time goes (one more run, %.3f s with event timing on): %s; the rest is the payload's copy to pageable host memory, "
    "the CRC-32 and the buffer" % (t1 - t0, ", ".join("%s %.2f ms" % (k, prof[k][0]) for k in ("png_filter", "png_deflate", "png_pack") if k in prof)))
c.profile_enable(0)
c.dev_free(d_comp)
c.close()
del comp, host, raw, z, data

say()
say("2. pano_stitch -test_dirs over %d config-4 rigs, -steps %d, pixflow_search_20 (wall seconds of the whole process, TIFF reads included)" % (a.rigs, a.steps))
work = tempfile.mkdtemp(prefix="png_ab_")
try:
    dirs = []
    for k in range(a.rigs):
        d = os.path.join(work, "rig%d" % k); os.makedirs(d); dirs.append(d)
        t, ims = synth.make_stitch_set(cols, rows, 1234 + k, 5, "cuda")
        Image.fromarray(t.cpu().numpy()[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(d, "top.tif"))
        for i in range(a.steps):
            Image.fromarray(ims[i].cpu().numpy()[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(d, "%d.tif" % (i + 1)))
        del t, ims
    exe = os.path.join(PKG, "tools", "pano_stitch")
    wall = {"default": [], "device": []}
    sizes = {}
    for run in range(a.cli_runs):
        for leg, extra in (("default", []), ("device", ["-png_device", "1"])):
            t0 = time.perf_counter()
            r = subprocess.run([exe, "-test_dirs", ",".join(dirs), "-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", str(a.steps)] + extra,
                               capture_output=True, text=True)
            t1 = time.perf_counter()
            if r.returncode != 0:
                say("%s run failed: %s" % (leg, r.stderr[-400:]))
                raise SystemExit(1)
            wall[leg].append(t1 - t0)
            parts = [ln.split("= ")[-1] for ln in r.stdout.splitlines() if "Finished!" in ln]
            sizes[leg] = sum(os.path.getsize(os.path.join(d, "FinalResult.png")) for d in dirs)
            say("run %d %-8s %7.2f s   (steps: %s)   FinalResult.png of all rigs: %d bytes" % (run + 1, leg, t1 - t0, ", ".join(parts), sizes[leg]))
            if leg == "default":
                keep = [np.array(Image.open(os.path.join(d, "FinalResult.png"))) for d in dirs[:1]]
            else:
                assert np.array_equal(np.array(Image.open(os.path.join(dirs[0], "FinalResult.png"))), keep[0]), "the two writers' files decode differently"
    for leg in ("default", "device"):
        say("%-8s best %.2f s, worst %.2f s" % (leg, min(wall[leg]), max(wall[leg])))
finally:
    shutil.rmtree(work, ignore_errors=True)

if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
