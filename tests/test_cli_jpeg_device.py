"""pano_stitch -jpeg_device 1: the results come out as .jpg in place of the .png, and each is, byte for byte, the serial model's
(tests/jpeg_model.py) encoding of the image the run without the flag writes as a PNG; the panels stay PNG; without the flag nothing
changes: PNG results only, the default writer's bytes."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeg_model as M
from conftest import PKG

EXE = os.path.join(PKG, "tools", "pano_stitch")
STEMS = ("ProcessResult1", "ProcessResult2", "FinalResult")
COMMON = ["-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", "3"]


def _write_rig(synth, d, cols, rows, seed, n):
    top, imgs = synth.make_stitch_set(cols, rows, seed, 5)
    os.makedirs(d, exist_ok=True)
    Image.fromarray(top.numpy()[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(d, "top.tif"))
    for i, im in enumerate(imgs[:n]):
        Image.fromarray(im.numpy()[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(d, "%d.tif" % (i + 1)))


def _run(args, ok=True):
    out = subprocess.run([EXE] + args, capture_output=True, text=True)
    if ok:
        assert out.returncode == 0, out.stderr
        assert "TotalRunTime (sec) = " in out.stdout
    return out


def _results_are_the_models(plain_dir, jpeg_dir, quality=90, subsampling=1, gpano=0):
    for stem in STEMS:
        want_img = np.ascontiguousarray(np.array(Image.open(os.path.join(plain_dir, stem + ".png")))[..., [2, 1, 0, 3]])
        assert want_img[..., 3].any()                                # a real composite, not an empty canvas
        got = open(os.path.join(jpeg_dir, stem + ".jpg"), "rb").read()
        assert got == M.encode(want_img, quality, subsampling, gpano=gpano), stem
        assert not os.path.exists(os.path.join(jpeg_dir, stem + ".png"))
        im = Image.open(os.path.join(jpeg_dir, stem + ".jpg"))
        assert im.format == "JPEG" and im.size == (want_img.shape[1], want_img.shape[0])


@pytest.mark.gpu
def test_lone_chain_with_and_without_jpeg_device(tmp_path, synth):
    a, b, c, d = (str(tmp_path / n) for n in ("plain", "jpeg", "both", "off"))
    _write_rig(synth, a, 480, 240, 77, 3)
    for other in (b, c, d):
        shutil.copytree(a, other)
    _run(["-test_dir", a] + COMMON + ["-visualize", "1"])
    # without the flag: PNG only
    assert sorted(f for f in os.listdir(a) if f.endswith((".png", ".jpg"))) == sorted(s + ".png" for s in STEMS)
    _run(["-test_dir", b] + COMMON + ["-jpeg_device", "1"])
    _results_are_the_models(a, b)
    # with -png_device 1 as well: results JPEG, panels device PNG (the same pixels as the default writer's panels); 2:1, so gpano is taken
    _run(["-test_dir", c] + COMMON + ["-jpeg_device", "1", "-png_device", "1", "-visualize", "1", "-jpeg_quality", "75", "-jpeg_subsampling", "444", "-jpeg_gpano", "1"])
    _results_are_the_models(a, c, 75, 0, gpano=1)
    panels = sorted(os.listdir(os.path.join(a, "disparity")))
    assert len(panels) == 6 and panels == sorted(os.listdir(os.path.join(c, "disparity"))) and all(p.endswith(".png") for p in panels)
    for p in panels:
        assert np.array_equal(np.array(Image.open(os.path.join(a, "disparity", p))), np.array(Image.open(os.path.join(c, "disparity", p))))
    # off when the flag says so: the files of the run without it
    _run(["-test_dir", d] + COMMON + ["-jpeg_device", "0", "-jpeg_quality", "10"])
    for stem in STEMS:
        assert open(os.path.join(d, stem + ".png"), "rb").read() == open(os.path.join(a, stem + ".png"), "rb").read()
        assert not os.path.exists(os.path.join(d, stem + ".jpg"))
    # refusals before any work
    for bad in (["-jpeg_quality", "0"], ["-jpeg_subsampling", "422"]):
        out = _run(["-test_dir", d] + COMMON + ["-jpeg_device", "1"] + bad, ok=False)
        assert out.returncode != 0 and "VrCamException" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [[], ["-static_rig", "1"], ["-static_rig", "1", "-rig_chain", "1"]], ids=["batch", "static_rig", "rig_chain"])
def test_test_dirs_with_and_without_jpeg_device(tmp_path, synth, mode):
    plain = [str(tmp_path / ("plain%d" % k)) for k in range(2)]
    dev = [str(tmp_path / ("jpeg%d" % k)) for k in range(2)]
    for k in range(2):
        _write_rig(synth, plain[k], 320, 240, 500 + k, 3)
        shutil.copytree(plain[k], dev[k])
    _run(["-test_dirs", ",".join(plain)] + COMMON + mode)
    _run(["-test_dirs", ",".join(dev)] + COMMON + mode + ["-jpeg_device", "1"])
    for k in range(2):
        _results_are_the_models(plain[k], dev[k])
    # not 2:1: gpano ends the run
    out = _run(["-test_dirs", ",".join(dev)] + COMMON + mode + ["-jpeg_device", "1", "-jpeg_gpano", "1"], ok=False)
    assert out.returncode != 0 and "gpano" in out.stderr
