"""pano_stitch -tiff_device 1 -tiff_inflate 1: deflate inputs at one row per strip are inflated on the GPU and give the oracle chain's
pixels; without -png_device the files are byte-equal to the host path's.  That the two flags really take the device path shows in the
one documented difference: a valid stream that is short, which the host reader zero-fills, ends the run with an error naming the strip."""
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest
from PIL import Image

import inflate_model as im
import png_decode_ref as R
import tiff_model as tm
from conftest import PKG
from test_cli_io import _oracle_chain

EXE = os.path.join(PKG, "tools", "pano_stitch")
COLS, ROWS, STEPS = 480, 320, 2
NAMES = ("ProcessResult1.png", "FinalResult.png")
COMMON = ["-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", str(STEPS)]
DEVICE = ["-tiff_device", "1", "-tiff_inflate", "1"]
pytestmark = pytest.mark.gpu


def _run(args, ok=True):
    out = subprocess.run([EXE] + args, capture_output=True, text=True)
    assert (out.returncode == 0) == ok, out.stdout + out.stderr
    return out


def _images(d):
    return [R.decode(open(os.path.join(d, name), "rb").read()) for name in NAMES]


@pytest.fixture(scope="module")
def rig(tmp_path_factory, synth, orc):
    """one rig of two steps as Pillow deflate files at one row per strip, and the oracle's chain"""
    d = str(tmp_path_factory.mktemp("tiff_inflate") / "rig")
    top, imgs = synth.make_stitch_set(COLS, ROWS, 600, 5)
    os.makedirs(d)
    for name, img in [("top", top)] + [(str(i + 1), img) for i, img in enumerate(imgs[:STEPS])]:
        Image.fromarray(img.numpy()[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(d, name + ".tif"), compression="tiff_adobe_deflate", tiffinfo={278: 1})
    f = tm.parse(open(os.path.join(d, "1.tif"), "rb").read())
    assert f[259][0] in (8, 32946) and f[278][0] == 1 and len(f[273]) == ROWS
    return d, _oracle_chain(orc, top.numpy(), [img.numpy() for img in imgs[:STEPS]], 20)


def _copy(d, tmp_path, tag):
    out = str(tmp_path / tag)
    shutil.copytree(d, out)
    return out


def test_rig_chain_on_deflate_inputs(rig, tmp_path):
    d, want = rig
    mode = ["-static_rig", "1", "-rig_chain", "1"]
    dev = _copy(d, tmp_path, "dev")
    _run(["-test_dirs", dev] + COMMON + mode + ["-png_device", "1"] + DEVICE)
    for name, got, w in zip(NAMES, _images(dev), want):
        assert np.array_equal(got, w), name
    # without -png_device the composites come down and the default writer's bytes are the host path's
    plain_host, plain_dev = _copy(d, tmp_path, "plain_host"), _copy(d, tmp_path, "plain_dev")
    _run(["-test_dirs", plain_host] + COMMON + mode)
    _run(["-test_dirs", plain_dev] + COMMON + mode + DEVICE)
    for name in NAMES:
        assert open(os.path.join(plain_dev, name), "rb").read() == open(os.path.join(plain_host, name), "rb").read(), name


def test_a_short_stream_ends_the_run_only_with_both_flags(rig, tmp_path):
    """strip 200 of 1.tif is a valid zlib stream of 100 of its 1920 bytes: the host reader zero-fills the rest, and so does
    -tiff_device 1 alone (the file goes to the host reader); with -tiff_inflate 1 the device path refuses the file"""
    d = _copy(rig[0], tmp_path, "short")
    img = np.array(Image.open(os.path.join(d, "1.tif")))
    data = im.write_tiff(img, zlib.compress, streams={200: zlib.compress(img[200].tobytes()[:100])})
    with open(os.path.join(d, "1.tif"), "wb") as f:
        f.write(data)
    _run(["-test_dir", d] + COMMON)
    _run(["-test_dir", d] + COMMON + ["-tiff_device", "1"])
    out = _run(["-test_dir", d] + COMMON + DEVICE, ok=False)
    assert "strip 200 decoded 100 of 1920 bytes" in out.stderr and "1.tif" in out.stderr, out.stderr
