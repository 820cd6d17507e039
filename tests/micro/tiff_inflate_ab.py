"""The device inflate (pf_tiff_set_inflate) against the host reader, on a machine with the GPU (profiles/tiff_inflate_ab.txt).

Part 1: one 9000x4000 RGBA image (synth.make_stitch_set seed 1234, image 1) as Pillow tiff_adobe_deflate at one row per strip, and the
same with predictor 2; the file is in the page cache.  Three alternated runs of each path, host clock:
  host      tools/image_io.hpp read_tiff (one thread, zlib's uncompress strip after strip) in a stand-alone program
            (tests/micro/read_tiff_time.cpp, built here with g++ -O2 unless --host-exe names a built one)
  device    the file's bytes read from the page cache, then pf_tiff_decode_dev; the kernels' share comes from the library's own event
            timing in a fourth run
Part 2 (--cli-runs N, default 0): wall time of the whole process `pano_stitch -test_dirs` over deflate rigs with -steps 2 -static_rig 1
-rig_chain 1 -png_device 1 -tiff_device 1, with and without -tiff_inflate 1, alternated.
  python tests/micro/tiff_inflate_ab.py [--cols 9000 --rows 4000] [--cli-runs 0] [--out profiles/tiff_inflate_ab.txt]"""
import argparse
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
ap.add_argument("--cli-runs", type=int, default=0)
ap.add_argument("--host-exe", default="")
ap.add_argument("--out", default="")
a = ap.parse_args()
cols, rows = a.cols, a.rows
lines = []
KINDS = (("deflate", dict(compression="tiff_adobe_deflate", tiffinfo={278: 1})), ("deflate+pred2", dict(compression="tiff_adobe_deflate", tiffinfo={278: 1, 317: 2})))


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med_spread(v):
    v = sorted(v)
    return v[len(v) // 2], v[-1] - v[0]


work = tempfile.mkdtemp(prefix="tiff_inflate_ab_")
try:
    exe_host = a.host_exe
    if not exe_host:
        exe_host = os.path.join(work, "read_tiff_time")
        subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe_host, os.path.join(ROOT, "tests", "micro", "read_tiff_time.cpp"), "-lz"], check=True)
    say("Device inflate against the host reader: %dx%d RGBA, one MI355X" % (cols, rows))
    c = pf.Context(0)
    c.tiff_set_inflate(1)
    top, imgs = synth.make_stitch_set(cols, rows, 1234, 5, "cuda")
    img = imgs[0].cpu().numpy()
    del top, imgs
    d_img = c.dev_alloc(img.nbytes)
    say()
    say("1. One image, file in the page cache (seconds; %d bytes raw)" % img.nbytes)
    for kind, kw in KINDS:
        path = os.path.join(work, kind + ".tif")
        Image.fromarray(img[..., [2, 1, 0, 3]], "RGBA").save(path, **kw)
        data = open(path, "rb").read()
        info = pf.tiff_probe(data)
        c.tiff_decode_dev(data, cols, rows, d_img)   # warm-up: the decoder's scratch is allocated here
        assert np.array_equal(c.download(np.empty_like(img), d_img), img), "the device decode of %s is not the image" % kind
        host, dev = [], []
        for run in range(3):
            r = subprocess.run([exe_host, path, "1"], capture_output=True, text=True, check=True)
            host.append(float(r.stdout.split()[0]))
            t0 = time.perf_counter()
            data = open(path, "rb").read()
            c.tiff_decode_dev(data, cols, rows, d_img)
            dev.append(time.perf_counter() - t0)
        c.profile_enable(1); c.profile_reset()
        c.tiff_decode_dev(data, cols, rows, d_img)
        prof = c.profile(); c.profile_enable(0)
        say("%-13s file %11d bytes, %5d strips | host read_tiff: median %.3f s, max - min %.3f s (runs %s) | device: median %.3f s, max - min %.3f s (runs %s) | kernels: %s"
            % (kind, len(data), info.n_strips, *med_spread(host), " ".join("%.3f" % v for v in host), *med_spread(dev), " ".join("%.3f" % v for v in dev),
               ", ".join("%s %.2f ms" % (k, prof[k][0]) for k in ("tiff_inflate", "tiff_finish") if k in prof)))
    c.dev_free(d_img)
    c.close()
    del img, data

    if a.cli_runs:
        say()
        say("2. pano_stitch -test_dirs over %d config-4 deflate rigs, -steps %d -static_rig 1 -rig_chain 1 -png_device 1 -tiff_device 1, pixflow_search_20 (wall seconds of the whole process)" % (a.rigs, a.steps))
        exe = os.path.join(PKG, "tools", "pano_stitch")
        kind, kw = KINDS[0]
        dirs = []
        for k in range(a.rigs):
            d = os.path.join(work, "rig%d" % k); os.makedirs(d); dirs.append(d)
            t, ims = synth.make_stitch_set(cols, rows, 1234 + k, 5, "cuda")
            Image.fromarray(t.cpu().numpy()[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(d, "top.tif"), **kw)
            for i in range(a.steps):
                Image.fromarray(ims[i].cpu().numpy()[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(d, "%d.tif" % (i + 1)), **kw)
            del t, ims
        wall = {"host": [], "device": []}
        keep = None
        for run in range(a.cli_runs):
            for leg, extra in (("host", []), ("device", ["-tiff_inflate", "1"])):
                t0 = time.perf_counter()
                r = subprocess.run([exe, "-test_dirs", ",".join(dirs), "-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", str(a.steps),
                                    "-static_rig", "1", "-rig_chain", "1", "-png_device", "1", "-tiff_device", "1"] + extra, capture_output=True, text=True)
                t1 = time.perf_counter()
                if r.returncode != 0:
                    say("%s run failed: %s" % (leg, r.stderr[-400:]))
                    raise SystemExit(1)
                wall[leg].append(t1 - t0)
                plan = [ln.split("= ")[-1] for ln in r.stdout.splitlines() if "Rig plan" in ln]
                say("run %d %-7s %7.2f s   (inputs read and rig plan made after %s s)" % (run + 1, leg, t1 - t0, ", ".join(plan)))
                got = open(os.path.join(dirs[0], "FinalResult.png"), "rb").read()
                if keep is None:
                    keep = got
                assert got == keep, "the two readers' runs wrote different files"
        for leg in ("host", "device"):
            say("%-7s median %.2f s, max - min %.2f s" % (leg, *med_spread(wall[leg])))
finally:
    shutil.rmtree(work, ignore_errors=True)

if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
