"""The lens remap kernel at a user's sizes against two yardsticks of the same box (profiles/lens_device.txt).

Part 1: five 6000x4000 photos in HBM, full-frame equidistant fisheyes of 120 degrees across, five poses 72 degrees apart with a generic
pitch and roll, with a radial polynomial, remapped onto five 9000x4000 canvases in ONE pf_lens_remap_batch_dev call, bicubic and
bilinear.  Three runs, the cases alternated; per case the kernel's time from the library's own events (family `lens`) and the host
clock around the call, the median with the spread.  In the same run:
  copy       a device-to-device copy that moves the bytes the kernel must (the photos read once plus the canvases written: a copy of
             half that many bytes reads and writes them), by events
  reproject  pf_reproject_dev levelling one 9000x4000 sphere (equirect to equirect, bicubic, yaw 37, pitch -21, roll 11; family
             `reproject`): the sibling kernel, which samples every pixel of its output
The remap is reported per canvas as a ratio to each.
Part 2 (--cli-runs N, default 0): wall time of the whole process pano_stitch over a rig of five cameras and a top camera at the same
canvas size (upright photos of 3/4 x 1 of --photo-rows, a square top photo), in the two modes tests/test_cli_lens.py runs (the lone
chain that holds its images on the host; -test_dirs -static_rig 1 -rig_chain 1 -tiff_device 1 -png_device 1), from the raw photos with
-lens_rig and from canvases remapped beforehand without it.
  python tests/micro/lens_device_ab.py [--cols 9000 --rows 4000 --photo-cols 6000 --photo-rows 4000] [--cli-runs 2] [--out profiles/lens_device.txt]"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--cols", type=int, default=9000)
ap.add_argument("--rows", type=int, default=4000)
ap.add_argument("--photo-cols", type=int, default=6000)
ap.add_argument("--photo-rows", type=int, default=4000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--cli-runs", type=int, default=0)
ap.add_argument("--out", default="")
a = ap.parse_args()
cols, rows, pc, pr = a.cols, a.rows, a.photo_cols, a.photo_rows
N = 5
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return sorted(v)[len(v) // 2]


def texture(w, h, seed):
    """an opaque BGRA image of smooth blobs with grain, made on the device"""
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    coarse = torch.rand((1, 3, max(h // 64, 2), max(w // 64, 2)), device="cuda", generator=g) * 176.0 + 40.0
    img = torch.nn.functional.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=False)[0]
    img = img + (torch.rand((3, h, w), device="cuda", generator=g) * 24.0 - 12.0)
    out = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
    out[..., :3] = img.clamp(0, 255).round().to(torch.uint8).permute(1, 2, 0)
    out[..., 3] = 255
    return out.cpu().numpy()


say("Lens remap of %d photos of %dx%d onto %dx%d canvases, one batch call, one MI355X: kernel time against a copy of the same traffic and against pf_reproject_dev" % (N, pc, pr, cols, rows))
c = pf.Context(0)
photo_bytes, canvas_bytes = pc * pr * 4, cols * rows * 4
d_photos = [c.dev_alloc(photo_bytes) for _ in range(N)]
d_canvases = [c.dev_alloc(canvas_bytes) for _ in range(N)]
for k in range(N):
    c.upload(d_photos[k], texture(pc, pr, 100 + k))
sphere = texture(cols, rows, 7)
d_sphere, d_level = c.dev_alloc(canvas_bytes), c.dev_alloc(canvas_bytes)
c.upload(d_sphere, sphere)
del sphere
focal = pf.lens_focal(pf.LENS_FISHEYE_EQUIDISTANT, pc, 120.0)
poly = (0.01, -0.05, 0.02)


def lenses(flt):
    return [pf.lens(pf.LENS_FISHEYE_EQUIDISTANT, filter=flt, rot=pf.lens_rotation((k - 2) * 72.0 + 37.0, -21.0, 11.0), focal_px=focal,
                    a=poly[0], b=poly[1], c=poly[2], dd=1.0 - sum(poly)) for k in range(N)]


turn = pf.reproject_rotation(37.0, -21.0, 11.0)
moved = N * (photo_bytes + canvas_bytes)
cases = [
    ("remap 5, bicubic", "lens", moved, N, lambda: c.lens_remap_batch_dev(d_photos, pc, pr, d_canvases, cols, rows, lenses(pf.REPROJECT_BICUBIC))),
    ("remap 5, bilinear", "lens", moved, N, lambda: c.lens_remap_batch_dev(d_photos, pc, pr, d_canvases, cols, rows, lenses(pf.REPROJECT_BILINEAR))),
    ("level %dx%d" % (cols, rows), "reproject", 2 * canvas_bytes, 1,
     lambda: c.reproject_dev(d_sphere, cols, rows, d_level, cols, rows, pf.reproject_params(projection=pf.PROJ_EQUIRECT, filter=pf.REPROJECT_BICUBIC, rot=turn))),
]
pool = torch.empty(moved, dtype=torch.uint8, device="cuda")   # the copies' source and destination


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


for name, fam, nbytes, n, call in cases:
    call()   # warm-up: tables, code objects
inside = []
one = np.empty((rows, cols, 4), np.uint8)
for k in range(N):
    inside.append(float((c.download(one, d_canvases[k])[..., 3] > 0).mean()))
del one
say("share of each canvas inside its photo: " + ", ".join("%.3f" % f for f in inside))
c.profile_enable(1)
say()
say("case                 run   kernel ms   call ms (host clock)   bytes moved (MB)   kernel GB/s   copy ms   kernel / copy")
res = {name: {"k": [], "h": [], "c": []} for name, _, _, _, _ in cases}
for run in range(3):
    for name, fam, nbytes, n, call in cases:
        c.profile_reset()
        t0 = time.perf_counter()
        call()
        t1 = time.perf_counter()
        k_ms = c.profile()[fam][0]
        cp = copy_ms(nbytes)
        res[name]["k"].append(k_ms); res[name]["h"].append((t1 - t0) * 1e3); res[name]["c"].append(cp)
        say("%-20s %d   %9.3f   %9.3f              %9.1f          %9.0f   %7.3f   %6.2f" % (name, run + 1, k_ms, (t1 - t0) * 1e3, nbytes / 1e6, nbytes / 1e6 / k_ms, cp, k_ms / cp))
c.profile_enable(0)
say()
level = med(res[cases[2][0]]["k"])
for name, fam, nbytes, n, _ in cases:
    r = res[name]
    say("%-20s median kernel %.3f ms (max - min %.3f), call %.3f ms (max - min %.3f), copy of the same traffic %.3f ms: kernel = %.2f x the copy; %.1f Mpx/s out" %
        (name, med(r["k"]), max(r["k"]) - min(r["k"]), med(r["h"]), max(r["h"]) - min(r["h"]), med(r["c"]), med(r["k"]) / med(r["c"]), n * cols * rows / 1e6 / (med(r["k"]) * 1e-3)))
for name, fam, nbytes, n, _ in cases[:2]:
    r = res[name]
    say("%-20s per canvas %.3f ms = %.2f x its share of the copy, %.2f x the levelled sphere (%.3f ms)" % (name, med(r["k"]) / n, med(r["k"]) / med(r["c"]), med(r["k"]) / n / level, level))
for d in d_photos + d_canvases + [d_sphere, d_level]:
    c.dev_free(d)
del pool
torch.cuda.empty_cache()

if a.cli_runs > 0:
    say()
    say("2. pano_stitch over a rig of five cameras and a top camera (rectilinear; photos of %dx%d, the top one %dx%d), -steps %d, pixflow_search_20, canvas %dx%d: from the raw photos with -lens_rig, "
        "and from canvases remapped beforehand without it (wall seconds of the whole process, TIFF reads included)" % (pr * 3 // 4, pr, pr, pr, a.steps, cols, rows))
    work = tempfile.mkdtemp(prefix="lens_ab_")
    try:
        rig = [("top.tif", pr, pr, 130.0, 0.0, 90.0, 0.0)] + [("%d.tif" % i, pr * 3 // 4, pr, 90.0, (i - 0.5) * 72.0 - 180.0, 0.0, 0.0) for i in range(1, 6)]
        with open(os.path.join(work, "rig.pto"), "w") as f:
            for name, w, h, v, y, p, r in rig:
                f.write('i w%d h%d f0 v%r y%r p%r r%r a0 b0 c0 d0 e0 n"%s"\n' % (w, h, v, y, p, r, name))
        raws, refs = [], []
        for k in range(2):   # two frames of the rig: the device mode takes several directories
            sphere = texture(cols, rows, 40 + k)
            d_s = c.dev_alloc(canvas_bytes); c.upload(d_s, sphere); del sphere
            raw = os.path.join(work, "raw%d" % k); ref = os.path.join(work, "ref%d" % k); os.makedirs(raw); os.makedirs(ref)
            raws.append(raw); refs.append(ref)
            for name, w, h, v, y, p, r in rig:
                photo = np.empty((h, w, 4), np.uint8); canvas = np.empty((rows, cols, 4), np.uint8)
                d_p, d_c = c.dev_alloc(photo.nbytes), c.dev_alloc(canvas.nbytes)
                c.reproject_dev(d_s, cols, rows, d_p, w, h, pf.reproject_params(projection=pf.PROJ_RECTILINEAR, filter=pf.REPROJECT_BICUBIC, hfov_deg=v, rot=pf.reproject_rotation(y, p, r)))
                c.lens_remap_dev(d_p, w, h, d_c, cols, rows, pf.lens(pf.LENS_RECTILINEAR, rot=pf.lens_rotation(y, p, r), focal_px=pf.lens_focal(pf.LENS_RECTILINEAR, w, v)))
                Image.fromarray(c.download(photo, d_p)[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(raw, name))
                Image.fromarray(c.download(canvas, d_c)[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(ref, name))
                c.dev_free(d_p); c.dev_free(d_c)
            c.dev_free(d_s)
        c.close(); c = None
        torch.cuda.empty_cache()
        exe = os.path.join(PKG, "tools", "pano_stitch")
        common = ["-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", str(a.steps)]
        lens_flags = ["-lens_rig", os.path.join(work, "rig.pto"), "-canvas", "%dx%d" % (cols, rows)]
        modes = [("lone chain, host images", lambda dirs: ["-test_dir", dirs[0]], []),
                 ("rig chain on the device", lambda dirs: ["-test_dirs", ",".join(dirs)], ["-static_rig", "1", "-rig_chain", "1", "-tiff_device", "1", "-png_device", "1"])]
        for mode, where, extra in modes:
            wall = {"canvases": [], "lens_rig": []}
            for run in range(a.cli_runs):
                for leg, dirs, flags in (("canvases", refs, []), ("lens_rig", raws, lens_flags)):
                    t0 = time.perf_counter()
                    r = subprocess.run([exe] + where(dirs) + common + extra + flags, capture_output=True, text=True)
                    t1 = time.perf_counter()
                    if r.returncode != 0:
                        say("%s %s run failed: %s" % (mode, leg, r.stderr[-400:]))
                        raise SystemExit(1)
                    wall[leg].append(t1 - t0)
                    say("%-26s run %d %-9s %7.2f s" % (mode, run + 1, leg, t1 - t0))
            say("%-26s canvases best %.2f s, worst %.2f s; -lens_rig best %.2f s, worst %.2f s: the remap of %d photos costs %.2f s of the run (difference of the best)" %
                (mode, min(wall["canvases"]), max(wall["canvases"]), min(wall["lens_rig"]), max(wall["lens_rig"]),
                 (a.steps + 1) * (1 if "lone" in mode else 2), min(wall["lens_rig"]) - min(wall["canvases"])))
    finally:
        shutil.rmtree(work, ignore_errors=True)
if c is not None:
    c.close()

if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
