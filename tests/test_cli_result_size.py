"""pano_stitch -result_size WxH [-result_filter F]: every result file is written at W x H, and its pixels are the serial model's
(tests/resize_model.py) resize of the image the run without the flag writes; the JPEG form carries the scaled size in its frame header
and in the GPano packet; without a device encoder the run is refused; without the flag the files are what they were: the default
writer's bytes, and with -png_device 1 the device encoder's file of the full-size composite."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeg_model
import resize_model as M
from conftest import PKG

EXE = os.path.join(PKG, "tools", "pano_stitch")
STEMS = ("ProcessResult1", "FinalResult")
COMMON = ["-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", "2"]


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


def _bgra(path):
    return np.ascontiguousarray(np.array(Image.open(path))[..., [2, 1, 0, 3]])


def _pngs_are_the_models(plain_dir, sized_dir, out_cols, out_rows, f):
    for stem in STEMS:
        full = _bgra(os.path.join(plain_dir, stem + ".png"))
        assert full[..., 3].any()                                    # a real composite, not an empty canvas
        got = _bgra(os.path.join(sized_dir, stem + ".png"))
        want = M.resize(full, out_cols, out_rows, f)
        assert got.shape == want.shape and np.array_equal(got, want), stem


def _jpegs_are_the_models(plain_dir, sized_dir, out_cols, out_rows, f, gpano=0):
    for stem in STEMS:
        want = M.resize(_bgra(os.path.join(plain_dir, stem + ".png")), out_cols, out_rows, f)
        got = open(os.path.join(sized_dir, stem + ".jpg"), "rb").read()
        assert got == jpeg_model.encode(want, gpano=gpano), stem
        im = Image.open(os.path.join(sized_dir, stem + ".jpg"))
        assert im.format == "JPEG" and im.size == (out_cols, out_rows)   # the frame header
        if gpano:
            xmp = im.applist[1][1].decode("latin-1")
            for field in ('GPano:FullPanoWidthPixels="%d"' % out_cols, 'GPano:FullPanoHeightPixels="%d"' % out_rows,
                          'GPano:CroppedAreaImageWidthPixels="%d"' % out_cols, 'GPano:CroppedAreaImageHeightPixels="%d"' % out_rows):
                assert field in xmp, field


@pytest.mark.gpu
def test_lone_chain(tmp_path, synth, pf):
    plain, png, jpg, host, off, vis = (str(tmp_path / n) for n in ("plain", "png", "jpg", "host", "off", "vis"))
    _write_rig(synth, plain, 480, 240, 77, 2)
    for other in (png, jpg, host, off, vis):
        shutil.copytree(plain, other)
    _run(["-test_dir", plain] + COMMON)
    # the resident composite, resized in HBM; the default filter is lanczos
    _run(["-test_dir", png] + COMMON + ["-png_device", "1", "-result_size", "200x100"])
    _pngs_are_the_models(plain, png, 200, 100, M.LANCZOS)
    _run(["-test_dir", jpg] + COMMON + ["-jpeg_device", "1", "-jpeg_gpano", "1", "-result_size", "256x128", "-result_filter", "bicubic"])
    _jpegs_are_the_models(plain, jpg, 256, 128, M.BICUBIC, gpano=1)
    assert not any(os.path.exists(os.path.join(jpg, stem + ".png")) for stem in STEMS)
    # -fused 0 holds its result on the host: sent up once, resized there (an upscale in width)
    _run(["-test_dir", host] + COMMON + ["-fused", "0", "-png_device", "1", "-result_size", "500x77", "-result_filter", "box"])
    _pngs_are_the_models(plain, host, 500, 77, M.BOX)
    # the panels are not scaled
    _run(["-test_dir", vis] + COMMON + ["-png_device", "1", "-visualize", "1", "-result_size", "200x100", "-result_filter", "hamming"])
    _pngs_are_the_models(plain, vis, 200, 100, M.HAMMING)
    panels = sorted(os.listdir(os.path.join(vis, "disparity")))
    assert len(panels) == 4 and all(Image.open(os.path.join(vis, "disparity", p)).size == (3 * 480, 240) for p in panels)
    # without the flag: the default writer's bytes as before, and -png_device 1 alone writes the device encoder's file of the full composite
    _run(["-test_dir", off] + COMMON + ["-png_device", "1"])
    ctx = pf.Context(0)
    try:
        for stem in STEMS:
            full = _bgra(os.path.join(plain, stem + ".png"))
            assert open(os.path.join(off, stem + ".png"), "rb").read() == ctx.png_encode(full), stem
    finally:
        ctx.close()
    again = str(tmp_path / "again")
    shutil.copytree(jpg, again)
    for stem in STEMS:
        os.remove(os.path.join(again, stem + ".jpg"))
    _run(["-test_dir", again] + COMMON)
    for stem in STEMS:
        assert open(os.path.join(again, stem + ".png"), "rb").read() == open(os.path.join(plain, stem + ".png"), "rb").read()
    # refusals before any work
    for bad, word in ((["-result_size", "200x100"], "needs -png_device 1 or -jpeg_device 1"),
                      (["-png_device", "1", "-result_size", "200"], "-result_size must be WxH"),
                      (["-png_device", "1", "-result_size", "0x100"], "-result_size must be WxH"),
                      (["-png_device", "1", "-result_size", "200x100", "-result_filter", "nearest"], "-result_filter must be"),
                      (["-png_device", "1", "-result_filter", "box"], "needs -result_size"),
                      (["-jpeg_device", "1", "-jpeg_gpano", "1", "-result_size", "200x120"], "2:1")):
        out = _run(["-test_dir", off] + COMMON + bad, ok=False)
        assert out.returncode != 0 and "VrCamException" in out.stderr and word in out.stderr, (bad, out.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [[], ["-static_rig", "1", "-rig_chain", "1"], ["-static_rig", "1", "-rig_chain", "1", "-tiff_device", "1"]],
                         ids=["batch", "rig_chain", "rig_chain_device"])
def test_test_dirs(tmp_path, synth, mode):
    plain = [str(tmp_path / ("plain%d" % k)) for k in range(2)]
    sized = [str(tmp_path / ("sized%d" % k)) for k in range(2)]
    for k in range(2):
        _write_rig(synth, plain[k], 320, 240, 500 + k, 2)
        shutil.copytree(plain[k], sized[k])
    _run(["-test_dirs", ",".join(plain)] + COMMON + mode)
    _run(["-test_dirs", ",".join(sized)] + COMMON + mode + ["-png_device", "1", "-result_size", "130x97", "-result_filter", "bilinear"])
    for k in range(2):
        _pngs_are_the_models(plain[k], sized[k], 130, 97, M.BILINEAR)
    _run(["-test_dirs", ",".join(sized)] + COMMON + mode + ["-jpeg_device", "1", "-result_size", "160x120"])
    for k in range(2):
        _jpegs_are_the_models(plain[k], sized[k], 160, 120, M.LANCZOS)
    out = _run(["-test_dirs", ",".join(sized)] + COMMON + mode + ["-result_size", "160x120"], ok=False)
    assert out.returncode != 0 and "needs -png_device 1 or -jpeg_device 1" in out.stderr
