"""pano_stitch -tiff_device 1: inputs decoded on the GPU give the pixels the host reader gives -- in the rig chain with every image
resident (and -png_device 1 encoding the composites where they lie), in the plain chain, and through the host fallback for deflate
files -- and all of them are the oracle chain's.  That the flag really takes the device path shows in the one documented difference: a
short strip, which the host reader zero-fills, ends the run with an error that names it."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import png_decode_ref as R
import tiff_model as tm
from conftest import PKG
from test_cli_io import _oracle_chain

EXE = os.path.join(PKG, "tools", "pano_stitch")
COLS, ROWS, STEPS = 480, 320, 2
NAMES = ("ProcessResult1.png", "FinalResult.png")
COMMON = ["-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", str(STEPS)]
pytestmark = pytest.mark.gpu


def _write_rig(synth, d, seed, compression):
    top, imgs = synth.make_stitch_set(COLS, ROWS, seed, 5)
    os.makedirs(d, exist_ok=True)
    kw = dict(compression=compression, tiffinfo={278: 1}) if compression == "tiff_lzw" else dict(compression=compression)
    for name, im in [("top", top)] + [(str(i + 1), im) for i, im in enumerate(imgs[:STEPS])]:
        Image.fromarray(im.numpy()[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(d, name + ".tif"), **kw)
    return top.numpy(), [im.numpy() for im in imgs[:STEPS]]


def _run(args, ok=True):
    out = subprocess.run([EXE] + args, capture_output=True, text=True)
    assert (out.returncode == 0) == ok, out.stdout + out.stderr
    return out


def _images(d):
    return [R.decode(open(os.path.join(d, name), "rb").read()) for name in NAMES]


@pytest.fixture(scope="module")
def rigs(tmp_path_factory, synth, orc):
    """two directories of one rig as LZW files at one row per strip, and the oracle's chain for each"""
    base = tmp_path_factory.mktemp("tiff_device")
    dirs, want = [], []
    for k in range(2):
        d = str(base / ("rig%d" % k))
        top, imgs = _write_rig(synth, d, 500 + k, "tiff_lzw")
        assert tm.parse(open(os.path.join(d, "1.tif"), "rb").read())[278][0] == 1
        dirs.append(d); want.append(_oracle_chain(orc, top, imgs, 20))
    return dirs, want


def _copies(dirs, tmp_path, tag):
    out = [str(tmp_path / ("%s%d" % (tag, k))) for k in range(len(dirs))]
    for src, dst in zip(dirs, out):
        shutil.copytree(src, dst)
    return out


def test_rig_chain_with_every_image_resident(rigs, tmp_path):
    dirs, want = rigs
    mode = ["-static_rig", "1", "-rig_chain", "1", "-png_device", "1"]
    host, dev = _copies(dirs, tmp_path, "host"), _copies(dirs, tmp_path, "dev")
    _run(["-test_dirs", ",".join(host)] + COMMON + mode)
    out = _run(["-test_dirs", ",".join(dev)] + COMMON + mode + ["-tiff_device", "1"])
    assert "Rig plan of 2 steps made!" in out.stdout and "TotalRunTime (sec) = " in out.stdout
    for k in range(2):
        for name, a, b, w in zip(NAMES, _images(host[k]), _images(dev[k]), want[k]):
            assert np.array_equal(a, b) and np.array_equal(b, w), "%s of directory %d" % (name, k)
    # without -png_device the composites come down and the default writer's bytes are the host path's
    plain_host, plain_dev = _copies(dirs, tmp_path, "plain_host"), _copies(dirs, tmp_path, "plain_dev")
    _run(["-test_dirs", ",".join(plain_host)] + COMMON + mode[:4])
    _run(["-test_dirs", ",".join(plain_dev)] + COMMON + mode[:4] + ["-tiff_device", "1"])
    for k in range(2):
        for name in NAMES:
            assert open(os.path.join(plain_dev[k], name), "rb").read() == open(os.path.join(plain_host[k], name), "rb").read()


def test_plain_chain(rigs, tmp_path):
    dirs, want = rigs
    host, dev = _copies(dirs[:1], tmp_path, "host"), _copies(dirs[:1], tmp_path, "dev")
    _run(["-test_dir", host[0]] + COMMON)
    _run(["-test_dir", dev[0]] + COMMON + ["-tiff_device", "1"])
    for name, w in zip(NAMES, want[0]):
        a, b = open(os.path.join(host[0], name), "rb").read(), open(os.path.join(dev[0], name), "rb").read()
        assert a == b and np.array_equal(R.decode(b), w), name


def test_deflate_directory_goes_through_the_host_fallback(tmp_path, synth, orc):
    d = str(tmp_path / "deflate")
    top, imgs = _write_rig(synth, d, 77, "tiff_adobe_deflate")
    _run(["-test_dir", d] + COMMON + ["-tiff_device", "1"])
    for got, w in zip(_images(d), _oracle_chain(orc, top, imgs, 20)):
        assert np.array_equal(got, w)


def test_a_short_strip_ends_the_run_only_on_the_device_path(rigs, tmp_path):
    """strip 200 of 1.tif ends in an early EOI (two bytes of 1920): the host reader zero-fills it, the device path refuses the file"""
    dirs, _ = rigs
    d = _copies(dirs[:1], tmp_path, "short")[0]
    img = np.array(Image.open(os.path.join(d, "1.tif")))
    data = tm.write_tiff(img, 5, rows_per_strip=1, strip_bytes={200: tm.lzw_pack([256, 65, 66, 257])})
    with open(os.path.join(d, "1.tif"), "wb") as f:
        f.write(data)
    _run(["-test_dir", d] + COMMON)
    out = _run(["-test_dir", d] + COMMON + ["-tiff_device", "1"], ok=False)
    assert "strip 200 decoded 2 of 1920 bytes" in out.stderr and "1.tif" in out.stderr, out.stderr
