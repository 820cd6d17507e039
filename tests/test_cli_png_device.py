"""pano_stitch -png_device 1: the files the device encoder writes decode to exactly the images the default writer's files hold, for the
lone chain and for -test_dirs, and the timing lines stay."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import png_decode_ref as R
from conftest import PKG

EXE = os.path.join(PKG, "tools", "pano_stitch")
NAMES = ("ProcessResult1.png", "ProcessResult2.png", "FinalResult.png")


def _write_rig(synth, d, cols, rows, seed, n):
    top, imgs = synth.make_stitch_set(cols, rows, seed, 5)
    os.makedirs(d, exist_ok=True)
    Image.fromarray(top.numpy()[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(d, "top.tif"))
    for i, im in enumerate(imgs[:n]):
        Image.fromarray(im.numpy()[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(d, "%d.tif" % (i + 1)))


def _run(args):
    out = subprocess.run([EXE] + args, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "TotalRunTime (sec) = " in out.stdout
    for i in (1, 2, 3):
        assert "Part%d Finished!RUNTIME (sec) = " % i in out.stdout
    return out


def _same_images(plain_dir, dev_dir):
    for name in NAMES:
        dev_bytes = open(os.path.join(dev_dir, name), "rb").read()
        want = np.array(Image.open(os.path.join(plain_dir, name)))[..., [2, 1, 0, 3]]
        got = R.decode(dev_bytes)                                  # the strict reader ...
        assert np.array_equal(got, want), "%s: %d bytes differ" % (name, int((got != want).sum()))
        pil = np.array(Image.open(os.path.join(dev_dir, name)))[..., [2, 1, 0, 3]]   # ... and an independent one
        assert np.array_equal(pil, want)
        assert want[..., 3].any()                                  # a real composite, not an empty canvas


@pytest.mark.gpu
def test_lone_chain_with_and_without_png_device(tmp_path, synth):
    a, b = str(tmp_path / "plain"), str(tmp_path / "dev")
    _write_rig(synth, a, 480, 320, 77, 3)
    shutil.copytree(a, b)
    common = ["-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", "3"]
    _run(["-test_dir", a] + common)
    _run(["-test_dir", b] + common + ["-png_device", "1"])
    _same_images(a, b)
    # off when the flag says so: the default writer's bytes
    c = str(tmp_path / "off")
    shutil.copytree(a, c, ignore=shutil.ignore_patterns("*.png"))
    _run(["-test_dir", c] + common + ["-png_device", "0"])
    for name in NAMES:
        assert open(os.path.join(c, name), "rb").read() == open(os.path.join(a, name), "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [[], ["-static_rig", "1"]], ids=["batch", "static_rig"])
def test_test_dirs_with_and_without_png_device(tmp_path, synth, mode):
    """-static_rig 1 still brings the first directory's composite down (the next plan is made from it); the directories of
    make_stitch_set share their masks whatever the seed, as frames of one rig do"""
    plain = [str(tmp_path / ("plain%d" % k)) for k in range(2)]
    dev = [str(tmp_path / ("dev%d" % k)) for k in range(2)]
    for k in range(2):
        _write_rig(synth, plain[k], 320, 240, 500 + k, 3)
        shutil.copytree(plain[k], dev[k])
    common = ["-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", "3"]
    _run(["-test_dirs", ",".join(plain)] + common + mode)
    _run(["-test_dirs", ",".join(dev)] + common + mode + ["-png_device", "1"])
    for k in range(2):
        _same_images(plain[k], dev[k])
