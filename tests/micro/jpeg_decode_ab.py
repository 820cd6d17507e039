"""The device JPEG decoder at a camera's size against the host route a user has today (profiles/jpeg_decode_ab.txt).

Images: one photo-like 6000x4000 scene (tests/jpegd_cases.py scene) at quality 90, as 4:2:0 and 4:2:2, both without restart markers and
with an MCU row per interval.
Part 1, per file: three alternated runs of
  host     Pillow's decode on one thread, the BGRA repack, and the upload (pf_upload) -- what a user does today
  device   pf_jpeg_decode_dev from the file's bytes (the file read is timed apart: it is the same for both routes)
medians and spread (max - min), the decoder's kernel times by the library's events (families jpegd_sync, jpegd_write -- place and write --,
jpegd_pixels -- DC sums, IDCT and pixels), and from the stage hook the rounds, the launches to the fixed point and the share of
subsequences whose first guessed walk already gave their final exit state.
Part 2: the same device figures across the lab build's subsequence sizes (PANOFLOW_JPEGD_SUBSEQ = 32 .. 1024): the table the product's
S is chosen from -- the fastest on the marker-less 4:2:0 file unless another is within the spread.
Part 3 (--cli-runs N, default 0): wall time of the whole process pano_stitch -rig_chain 1 -tiff_device 1 -png_device 1 over two frames
of a 5 + top rig from JPEG photos (-input_ext jpg) against the same run from TIFFs that hold Pillow's decode of them.
  python tests/micro/jpeg_decode_ab.py [--cols 6000 --rows 4000] [--cli-runs 2] [--out profiles/jpeg_decode_ab.txt]"""
import argparse
import io
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import PKG, load_pkg_module  # noqa: E402

import torch  # noqa: E402  (torch's HIP runtime first)
torch.cuda.init()
torch.set_num_threads(1)
from PIL import Image  # noqa: E402
import jpegd_cases as jc  # noqa: E402
import jpegd_model as jm  # noqa: E402
pf = load_pkg_module("pyabi")

ap = argparse.ArgumentParser()
ap.add_argument("--cols", type=int, default=6000)
ap.add_argument("--rows", type=int, default=4000)
ap.add_argument("--cli-runs", type=int, default=0)
ap.add_argument("--out", default="")
a = ap.parse_args()
W, H = a.cols, a.rows
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return sorted(v)[len(v) // 2]


def spread(v):
    return max(v) - min(v)


say("JPEG decode of one %dx%d photo-like image, quality 90, one MI355X: the host route (Pillow on one thread + BGRA repack + upload) against pf_jpeg_decode_dev" % (W, H))
img = jc.scene(W, H, 2026)
files = {}
for sub in ("420", "422"):
    for rows_per_interval in (0, 1):
        name = "%s %s" % (sub, "an MCU row per interval" if rows_per_interval else "no restart markers")
        files[name] = jc.pil_jpeg(img, 90, sub, False, jc._mcu_row(W, sub) * rows_per_interval)
del img
work = tempfile.mkdtemp(prefix="jpegd_ab_")
paths = {}
for k, (name, data) in enumerate(files.items()):
    paths[name] = os.path.join(work, "%d.jpg" % k)
    with open(paths[name], "wb") as f:
        f.write(data)


def geometry(data):
    info = jm.parse(data)
    mc, mr, bpm = jm.geometry(info)
    planes = mc * mr * 64 * bpm
    return info, mc * mr * bpm, planes


def host_route(ctx, path, d_out):
    t0 = time.perf_counter()
    rgb = np.asarray(Image.open(path).convert("RGB"))
    t1 = time.perf_counter()
    bgra = np.empty(rgb.shape[:2] + (4,), np.uint8)
    bgra[..., 0] = rgb[..., 2]; bgra[..., 1] = rgb[..., 1]; bgra[..., 2] = rgb[..., 0]; bgra[..., 3] = 255
    t2 = time.perf_counter()
    ctx.upload(d_out, bgra)
    t3 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3


def device_route(ctx, path, d_out):
    t0 = time.perf_counter()
    with open(path, "rb") as f:
        data = f.read()
    t1 = time.perf_counter()
    ctx.profile_reset()
    ctx.jpeg_decode_dev(data, W, H, d_out)
    t2 = time.perf_counter()
    prof = ctx.profile()
    fam = [prof.get(n, (0.0, 0))[0] for n in ("jpegd_sync", "jpegd_write", "jpegd_pixels")]
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, fam


def measure(ctx, S, with_host):
    """three alternated runs over the files; -> per file a dict of lists"""
    d_out = ctx.dev_alloc(W * H * 4)
    res = {name: dict(host=[], dec=[], rep=[], up=[], read=[], dev=[], fam=[]) for name in files}
    stage = {}
    try:
        for name, data in files.items():   # warm-up: code objects, the arena; and the stage hook's counts
            ctx.jpeg_decode_dev(data, W, H, d_out)
            info, nblocks, planes = geometry(data)
            _, _, _, counts = ctx.stage_jpeg_decode(data, jm.n_subsequences(info, S), nblocks, planes)
            stage[name] = [int(v) for v in counts]
        ctx.profile_enable(1)
        for run in range(3):
            for name in files:
                if with_host:
                    dec, rep, up = host_route(ctx, paths[name], d_out)
                    r = res[name]; r["dec"].append(dec); r["rep"].append(rep); r["up"].append(up); r["host"].append(dec + rep + up)
                read, dev, fam = device_route(ctx, paths[name], d_out)
                r = res[name]; r["read"].append(read); r["dev"].append(dev); r["fam"].append(fam)
        ctx.profile_enable(0)
    finally:
        ctx.dev_free(d_out)
    return res, stage


c = pf.Context(0)
S0 = jc.S_PRODUCT
res, stage = measure(c, S0, True)
# the device's bytes are Pillow's, at this size too
d = c.dev_alloc(W * H * 4)
for name, data in files.items():
    c.jpeg_decode_dev(data, W, H, d)
    same = np.array_equal(c.download(np.empty((H, W, 4), np.uint8), d), jc.pillow_bgra(data))
    say("%-32s file %8d bytes, entropy segment %8d: the device's bytes %s Pillow's" % (name, len(data), jm.parse(data)["end"] - jm.parse(data)["begin"], "ARE" if same else "ARE NOT"))
c.dev_free(d)
say()
say("1. the product (S = %d): medians of three alternated runs in ms, (max - min)" % S0)
say("file                              host route = decode + repack + upload                    device call      file read   sync / write / pixels kernels   host / device")
for name in files:
    r = res[name]
    fam = [med([f[k] for f in r["fam"]]) for k in range(3)]
    say("%-32s %7.1f (%5.1f) = %6.1f + %5.1f + %5.1f      %7.2f (%5.2f)   %6.2f      %6.2f / %5.2f / %5.2f            %5.1f x" %
        (name, med(r["host"]), spread(r["host"]), med(r["dec"]), med(r["rep"]), med(r["up"]), med(r["dev"]), spread(r["dev"]), med(r["read"]), fam[0], fam[1], fam[2],
         med(r["host"]) / med(r["dev"])))
say()
say("file                              subsequences   rounds   launches   already final after the first walk")
for name in files:
    n, rounds, launches, S, moved = stage[name]
    say("%-32s %9d   %6d   %6d      %6.2f %%" % (name, n, rounds, launches, 100.0 * max(0, n - moved) / n))
c.close()

say()
say("2. the lab build across subsequence sizes: device call ms, median (max - min); kernels sync / write / pixels; rounds, launches, share final after the first walk")
lab = pf.Context(0, exp=True)
table = {}
for S in (32, 64, 128, 256, 512, 1024):
    os.environ["PANOFLOW_JPEGD_SUBSEQ"] = str(S)
    r_s, st_s = measure(lab, S, False)
    table[S] = r_s
    for name in files:
        r = r_s[name]
        fam = [med([f[k] for f in r["fam"]]) for k in range(3)]
        n, rounds, launches, s_used, moved = st_s[name]
        assert s_used == S
        say("S = %4d  %-32s %7.2f (%5.2f)   %6.2f / %5.2f / %5.2f   %4d rounds, %3d launches, %6.2f %%" %
            (S, name, med(r["dev"]), spread(r["dev"]), fam[0], fam[1], fam[2], rounds, launches, 100.0 * max(0, n - moved) / n))
del os.environ["PANOFLOW_JPEGD_SUBSEQ"]
lab.close()
key = "420 no restart markers"
best = min(table, key=lambda S: med(table[S][key]["dev"]))
say("fastest on the marker-less 4:2:0 file: S = %d (%.2f ms); the product's S = %d takes %.2f ms (spread %.2f)" %
    (best, med(table[best][key]["dev"]), S0, med(table[S0][key]["dev"]), spread(table[S0][key]["dev"])))

if a.cli_runs > 0:
    import test_cli_jpeg_input as T
    import test_cli_lens as L
    say()
    say("3. pano_stitch -static_rig 1 -rig_chain 1 -tiff_device 1 -png_device 1 over two frames of the 5 + top rig of tests/test_cli_lens.py "
        "(its photo sizes), canvas %dx%d: wall seconds of the whole process" % L.CANVAS)
    jpgs, tifs = [], []
    for k in range(2):
        j, t = os.path.join(work, "jpg%d" % k), os.path.join(work, "tif%d" % k)
        T._write_rig(j, t, 900 + k)
        jpgs.append(j); tifs.append(t)
    exe = os.path.join(PKG, "tools", "pano_stitch")
    mode = ["-static_rig", "1", "-rig_chain", "1", "-tiff_device", "1", "-png_device", "1", "-canvas", "%dx%d" % L.CANVAS]
    wall = {"tif": [], "jpg": []}
    for run in range(a.cli_runs):
        for leg, dirs, common in (("tif", tifs, L.COMMON), ("jpg", jpgs, T.COMMON_JPG)):
            t0 = time.perf_counter()
            r = subprocess.run([exe, "-test_dirs", ",".join(dirs)] + common + mode + ["-lens_rig", os.path.join(dirs[0], "rig.pto")], capture_output=True, text=True)
            t1 = time.perf_counter()
            if r.returncode != 0:
                say("%s run failed: %s" % (leg, r.stderr[-400:]))
                raise SystemExit(1)
            wall[leg].append(t1 - t0)
            say("run %d from %s photos %7.2f s" % (run + 1, leg, t1 - t0))
    say("from TIFF photos best %.2f s, from JPEG photos best %.2f s (the rig's photos are 96x128 and 128x128: process start-up dominates)" % (min(wall["tif"]), min(wall["jpg"])))
shutil.rmtree(work, ignore_errors=True)

if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
