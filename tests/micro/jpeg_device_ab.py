"""The device JPEG encoder against the only host route there is, on a machine with the GPU (profiles/jpeg_device_ab.txt).

One 9000x4000 composite resident in HBM (the result of a stitch step on a config-4 rig, synth.make_stitch_set seed 1234), quality 90,
4:2:0 and 4:4:4, three runs of each path, alternated, host clock:
  host      pf_download of the raw composite, then Pillow's libjpeg-turbo encode with the same settings (ONE host thread of SIMD code; the
            BGRA -> RGB repack it needs first is timed apart)
  device    pf_jpeg_encode_dev (colour, DCT, quantisation, entropy coding in kernels, the entropy-coded segment down, header on the host);
            the kernels' share comes from the library's own event timing in a fourth run
Then the device PNG of the same composite (pf_png_encode_dev: time and size), and the restart interval: the product's R against R / 4,
R / 2 and 2 R, through the lab build's PANOFLOW_JPEG_RESTART, time (median of three), file size and the kernels' event times.
  python tests/micro/jpeg_device_ab.py [--cols 9000 --rows 4000] [--out profiles/jpeg_device_ab.txt]"""
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


say("Device JPEG encoder against download + libjpeg-turbo on one host thread: %dx%d, quality 90, one MI355X" % (cols, rows))
c = pf.Context(0)
top, imgs = synth.make_stitch_set(cols, rows, 1234, 5, "cuda")
top = top.cpu().numpy(); imgs = [im.cpu().numpy() for im in imgs]
comp = c.stitch_step(imgs[0], top, 20)
d_comp = c.dev_alloc(comp.nbytes)
c.upload(d_comp, comp)
host = np.empty_like(comp)
npx = cols * rows

for sub, name in ((1, "4:2:0"), (0, "4:4:4")):
    p = pf.jpeg_params(quality=90, subsampling=sub)
    R = pf.jpeg_restart_interval(sub)
    c.jpeg_encode_dev(d_comp, cols, rows, p)   # warm-up: the encoder's scratch is allocated here
    say()
    say("%s, restart interval %d MCUs (seconds; %d bytes raw)" % (name, R, comp.nbytes))
    say("run  host: download   repack  libjpeg-turbo    total   file bytes | device: pf_jpeg_encode_dev   file bytes")
    tot = {"host": [], "device": []}
    for run in range(3):
        t0 = time.perf_counter()
        c.download(host, d_comp)
        t1 = time.perf_counter()
        rgb = np.ascontiguousarray(host[..., [2, 1, 0]])
        t2 = time.perf_counter()
        buf = io.BytesIO()
        Image.fromarray(rgb, "RGB").save(buf, format="JPEG", quality=90, subsampling=2 if sub else 0, restart_marker_blocks=R)
        t3 = time.perf_counter()
        ref = buf.getvalue()
        t4 = time.perf_counter()
        data = c.jpeg_encode_dev(d_comp, cols, rows, p)
        t5 = time.perf_counter()
        tot["host"].append(t3 - t0); tot["device"].append(t5 - t4)
        say("%d    %14.4f %8.4f %14.4f %8.4f %12d | %27.4f %12d" % (run + 1, t1 - t0, t2 - t1, t3 - t2, t3 - t0, len(ref), t5 - t4, len(data)))
    say("the device's file %s libjpeg-turbo's, byte for byte" % ("IS" if data == ref else "IS NOT"))
    for k in ("host", "device"):
        say("%-8s median %.4f s, max - min %.4f s" % (k, med(tot[k]), max(tot[k]) - min(tot[k])))
    say("ratio of the medians: %.1f;  file %.4f of raw" % (med(tot["host"]) / med(tot["device"]), len(data) / comp.nbytes))
    c.profile_enable(1); c.profile_reset()
    t0 = time.perf_counter(); c.jpeg_encode_dev(d_comp, cols, rows, p); t1 = time.perf_counter()
    prof = c.profile()
    c.profile_enable(0)
    say("where the device path's time goes (one more run, %.4f s with event timing on): %s; the rest is two drains, the segment's copy to pageable "
        "host memory and the worst-case buffer" % (t1 - t0, ", ".join("%s %.2f ms" % (k, prof[k][0]) for k in ("jpeg_blocks", "jpeg_sizes", "jpeg_write") if k in prof)))
    if "jpeg_blocks" in prof:
        traffic = npx * (4 + (3 if sub else 6))
        say("k_jpeg_blocks moves %.0f MB (4 B/px in, %d out): %.0f GB/s" % (traffic / 1e6, 3 if sub else 6, traffic / 1e6 / prof["jpeg_blocks"][0]))

say()
c.png_encode_dev(d_comp, cols, rows)
t = []
for run in range(3):
    t0 = time.perf_counter(); png = c.png_encode_dev(d_comp, cols, rows); t.append(time.perf_counter() - t0)
say("device PNG of the same composite (pf_png_encode_dev): median %.4f s, %d bytes, %.4f of raw" % (med(t), len(png), len(png) / comp.nbytes))
c.dev_free(d_comp)
c.close()

say()
say("The restart interval, lab build (PANOFLOW_JPEG_RESTART), quality 90: median of three pf_jpeg_encode_dev calls, the file's size, and the")
say("kernels' event times of a fourth call (sizes = size pass + scan).  An interval of more than 192 blocks is staged in LDS in two rounds.")
lab = pf.Context(0, exp=True)
d_comp = lab.dev_alloc(comp.nbytes)
lab.upload(d_comp, comp)
for sub, name in ((1, "4:2:0"), (0, "4:4:4")):
    p = pf.jpeg_params(quality=90, subsampling=sub)
    R = pf.jpeg_restart_interval(sub)
    for r in (R // 4, R // 2, R, 2 * R):
        os.environ["PANOFLOW_JPEG_RESTART"] = str(r)
        lab.jpeg_encode_dev(d_comp, cols, rows, p, cap=pf.jpeg_bound(cols, rows, p) * 2)
        t = []
        for run in range(3):
            t0 = time.perf_counter(); data = lab.jpeg_encode_dev(d_comp, cols, rows, p, cap=pf.jpeg_bound(cols, rows, p) * 2); t.append(time.perf_counter() - t0)
        assert int.from_bytes(data[data.index(b"\xff\xdd") + 4:][:2], "big") == r
        lab.profile_enable(1); lab.profile_reset()
        lab.jpeg_encode_dev(d_comp, cols, rows, p, cap=pf.jpeg_bound(cols, rows, p) * 2)
        prof = lab.profile()
        lab.profile_enable(0)
        say("%s  R = %3d%s  %.4f s (max - min %.4f)  %d bytes   %s" % (name, r, " (product)" if r == R else "          ", med(t), max(t) - min(t), len(data),
                                                                      ", ".join("%s %.2f ms" % (k[5:], prof[k][0]) for k in ("jpeg_blocks", "jpeg_sizes", "jpeg_write") if k in prof)))
del os.environ["PANOFLOW_JPEG_RESTART"]
lab.dev_free(d_comp)
lab.close()

if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
