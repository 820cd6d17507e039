"""A result at the delivery size: resized and encoded on the device against what a user did before (profiles/resize_device_ab.txt).

One 9000x4000 composite resident in HBM (the result of a stitch step on a config-4 rig, synth.make_stitch_set seed 1234), delivered as a
quality-90 4:2:0 JPEG at 4096x2048 (LANCZOS) and at 1024x512 (BOX); three runs of each path, alternated, host clock:
  host      pf_download of the raw composite, Pillow's Image.resize of the RGBA image (ONE host thread), the RGB repack and Pillow's
            libjpeg-turbo encode
  device    pf_stitch_result_resized_dev + pf_jpeg_encode_dev: only the JPEG crosses the link
Then the kernels' share from the library's own event timing in a fourth run, and the bytes each pass moves against the measured HBM
copy rate (6.29 TB/s).  The resized images of the two paths are compared byte for byte at these sizes as well.
  python tests/micro/resize_device_ab.py [--cols 9000 --rows 4000] [--out profiles/resize_device_ab.txt]"""
import argparse
import io
import os
import sys
import time

import numpy as np

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import load_pkg_module  # noqa: E402

import torch  # noqa: E402  (torch's HIP runtime first: conftest._torch_hip_first)
torch.cuda.init()
from PIL import Image  # noqa: E402
pf = load_pkg_module("pyabi")
synth = load_pkg_module("synth")

HBM_COPY_RATE = 6.29e12   # bytes/s, a float4 copy on this part

ap = argparse.ArgumentParser()
ap.add_argument("--cols", type=int, default=9000)
ap.add_argument("--rows", type=int, default=4000)
ap.add_argument("--out", default="")
a = ap.parse_args()
cols, rows = a.cols, a.rows
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return sorted(v)[len(v) // 2]


say("A %dx%d composite delivered as a smaller JPEG (quality 90, 4:2:0): resize + encode on the device against download + Pillow on one host thread, one MI355X" % (cols, rows))
c = pf.Context(0)
top, imgs = synth.make_stitch_set(cols, rows, 1234, 5, "cuda")
top = top.cpu().numpy(); imgs = [im.cpu().numpy() for im in imgs]
comp = c.stitch_step(imgs[0], top, 20)   # stays resident in "ch_final"
d_comp = c.dev_alloc(comp.nbytes)        # the copy the host path downloads
c.upload(d_comp, comp)
host = np.empty_like(comp)
params = pf.jpeg_params(quality=90, subsampling=1)

for out_cols, out_rows, f, name in ((4096, 2048, pf.RESIZE_LANCZOS, "LANCZOS"), (1024, 512, pf.RESIZE_BOX, "BOX")):
    small = np.empty((out_rows, out_cols, 4), np.uint8)
    d_small = c.dev_alloc(small.nbytes)
    c.stitch_result_resized_dev(out_cols, out_rows, d_small, f); c.jpeg_encode_dev(d_small, out_cols, out_rows, params)   # warm-up: tables and scratch
    say()
    say("%dx%d %s (seconds; %d bytes raw in, %d raw out)" % (out_cols, out_rows, name, comp.nbytes, small.nbytes))
    say("run  host: download   resize   repack  libjpeg-turbo    total | device: resize   encode    total   file bytes")
    tot = {"host": [], "device": []}
    for run in range(3):
        t0 = time.perf_counter()
        c.download(host, d_comp)
        t1 = time.perf_counter()
        ref_small = np.asarray(Image.fromarray(host, "RGBA").resize((out_cols, out_rows), f))
        t2 = time.perf_counter()
        rgb = np.ascontiguousarray(ref_small[..., [2, 1, 0]])
        t3 = time.perf_counter()
        buf = io.BytesIO()
        Image.fromarray(rgb, "RGB").save(buf, format="JPEG", quality=90, subsampling=2, restart_marker_blocks=pf.jpeg_restart_interval(1))
        t4 = time.perf_counter()
        ref = buf.getvalue()
        t5 = time.perf_counter()
        c.stitch_result_resized_dev(out_cols, out_rows, d_small, f)
        t6 = time.perf_counter()
        data = c.jpeg_encode_dev(d_small, out_cols, out_rows, params)
        t7 = time.perf_counter()
        tot["host"].append(t4 - t0); tot["device"].append(t7 - t5)
        say("%d    %14.4f %8.4f %8.4f %14.4f %8.4f | %14.4f %8.4f %8.4f %12d" % (run + 1, t1 - t0, t2 - t1, t3 - t2, t4 - t3, t4 - t0, t6 - t5, t7 - t6, t7 - t5, len(data)))
    c.download(small, d_small)
    say("the device's resized image %s Pillow's, byte for byte; its JPEG %s libjpeg-turbo's of that image" % ("IS" if np.array_equal(small, ref_small) else "IS NOT", "IS" if data == ref else "IS NOT"))
    for k in ("host", "device"):
        say("%-8s median %.4f s, max - min %.4f s" % (k, med(tot[k]), max(tot[k]) - min(tot[k])))
    say("ratio of the medians: %.1f" % (med(tot["host"]) / med(tot["device"])))
    c.profile_enable(1); c.profile_reset()
    c.stitch_result_resized_dev(out_cols, out_rows, d_small, f); c.jpeg_encode_dev(d_small, out_cols, out_rows, params)
    prof = c.profile()
    c.profile_enable(0)
    say("event times of one more run: %s" % ", ".join("%s %.3f ms" % (k, prof[k][0]) for k in ("resize_h", "resize_v", "jpeg_blocks", "jpeg_sizes", "jpeg_write") if k in prof))
    moved = {"resize_h": 4 * (cols * rows + out_cols * rows), "resize_v": 4 * (out_cols * rows + out_cols * out_rows)}
    for k in ("resize_h", "resize_v"):
        if k in prof:
            floor_ms = moved[k] / HBM_COPY_RATE * 1e3
            say("%s moves %.1f MB (image in, image out; tables apart): %.0f GB/s, %.3f ms at the copy rate, %.2f of it" %
                (k, moved[k] / 1e6, moved[k] / 1e6 / prof[k][0], floor_ms, floor_ms / prof[k][0]))
    c.dev_free(d_small)

c.dev_free(d_comp)
c.close()

if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
