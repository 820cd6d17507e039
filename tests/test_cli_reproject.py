"""pano_stitch -level yaw,pitch,roll and -cube N [-cube_filter F]: the levelled result and the six faces are the reprojection model's
(tests/reproject_model.py) images of the result the same run writes unturned; -result_size and the encoders come after the turn; the
faces carry no GPano packet; without a device encoder, or with a malformed flag, the run ends before any output."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

import jpeg_model
import reproject_model as M
import resize_model
from conftest import PKG

EXE = os.path.join(PKG, "tools", "pano_stitch")
STEMS = ("ProcessResult1", "FinalResult")
COMMON = ["-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", "2"]
COLS, ROWS = 320, 240
YPR = (30.0, -10.0, 5.0)
LEVEL = ["-level", "30,-10,5"]


def _write_rig(synth, d, seed):
    top, imgs = synth.make_stitch_set(COLS, ROWS, seed, 5)
    os.makedirs(d, exist_ok=True)
    Image.fromarray(top.numpy()[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(d, "top.tif"))
    for i, im in enumerate(imgs[:2]):
        Image.fromarray(im.numpy()[..., [2, 1, 0, 3]], "RGBA").save(os.path.join(d, "%d.tif" % (i + 1)))


def _run(args, ok=True):
    out = subprocess.run([EXE] + args, capture_output=True, text=True)
    if ok:
        assert out.returncode == 0, out.stderr
        assert "TotalRunTime (sec) = " in out.stdout
    return out


def _bgra(path):
    return np.ascontiguousarray(np.array(Image.open(path))[..., [2, 1, 0, 3]])


def _levelled(full):
    return M.reproject(full, full.shape[1], full.shape[0], M.EQUIRECT, filter=M.BICUBIC, rot=M.rotation(*YPR))


def _faces_are_the_models(src, d, stem, n, flt, ext="png"):
    for face, name in enumerate(M.FACE_NAMES):
        want = M.reproject(src, n, n, M.CUBE, face, flt)
        path = os.path.join(d, "%s_%s.%s" % (stem, name, ext))
        if ext == "png":
            got = _bgra(path)
            assert got.shape == want.shape and np.array_equal(got, want), (stem, name)
        else:
            assert open(path, "rb").read() == jpeg_model.encode(want), (stem, name)   # gpano = 0: a face is no sphere


@pytest.mark.gpu
def test_lone_chain(tmp_path, synth):
    plain, both, cube, jpg, host = (str(tmp_path / n) for n in ("plain", "both", "cube", "jpg", "host"))
    _write_rig(synth, plain, 77)
    for other in (both, cube, jpg, host):
        shutil.copytree(plain, other)
    _run(["-test_dir", plain] + COMMON)
    full = {stem: _bgra(os.path.join(plain, stem + ".png")) for stem in STEMS}
    assert all(f[..., 3].any() for f in full.values())
    # the resident composite turned in HBM; the faces are cut from the turned one.  The chain itself ran unturned: step 2's result is
    # the turned plain result, not a stitch onto a turned step 1
    _run(["-test_dir", both] + COMMON + ["-png_device", "1", "-cube", "16"] + LEVEL)
    for stem in STEMS:
        lev = _levelled(full[stem])
        assert np.array_equal(_bgra(os.path.join(both, stem + ".png")), lev), stem
        _faces_are_the_models(lev, both, stem, 16, M.BICUBIC)
    # -cube alone leaves the result what -png_device 1 writes; bilinear faces from the unturned composite
    _run(["-test_dir", cube] + COMMON + ["-png_device", "1", "-cube", "16", "-cube_filter", "bilinear"])
    for stem in STEMS:
        assert np.array_equal(_bgra(os.path.join(cube, stem + ".png")), full[stem]), stem
        _faces_are_the_models(full[stem], cube, stem, 16, M.BILINEAR)
    # the turn comes before -result_size and the encoder; a 2:1 result may declare a sphere, the faces never do
    _run(["-test_dir", jpg] + COMMON + ["-jpeg_device", "1", "-jpeg_gpano", "1", "-result_size", "160x80", "-result_filter", "bicubic", "-cube", "16"] + LEVEL)
    for stem in STEMS:
        lev = _levelled(full[stem])
        want = resize_model.resize(lev, 160, 80, resize_model.BICUBIC)
        assert open(os.path.join(jpg, stem + ".jpg"), "rb").read() == jpeg_model.encode(want, gpano=1), stem
        _faces_are_the_models(lev, jpg, stem, 16, M.BICUBIC, ext="jpg")
        assert not os.path.exists(os.path.join(jpg, stem + ".png"))
    # -fused 0 holds its result on the host: sent up once, turned there
    _run(["-test_dir", host] + COMMON + ["-fused", "0", "-png_device", "1", "-cube", "7"] + LEVEL)
    for stem in STEMS:
        lev = _levelled(full[stem])
        assert np.array_equal(_bgra(os.path.join(host, stem + ".png")), lev), stem
        _faces_are_the_models(lev, host, stem, 7, M.BICUBIC)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [[], ["-static_rig", "1", "-rig_chain", "1", "-tiff_device", "1"]], ids=["batch", "rig_chain_device"])
def test_test_dirs(tmp_path, synth, mode):
    plain = [str(tmp_path / ("plain%d" % k)) for k in range(2)]
    turned = [str(tmp_path / ("turned%d" % k)) for k in range(2)]
    for k in range(2):
        _write_rig(synth, plain[k], 500 + k)
        shutil.copytree(plain[k], turned[k])
    _run(["-test_dirs", ",".join(plain)] + COMMON + mode)
    _run(["-test_dirs", ",".join(turned)] + COMMON + mode + ["-png_device", "1", "-cube", "16"] + LEVEL)
    for k in range(2):
        for stem in STEMS:
            lev = _levelled(_bgra(os.path.join(plain[k], stem + ".png")))
            assert np.array_equal(_bgra(os.path.join(turned[k], stem + ".png")), lev), (k, stem)
            _faces_are_the_models(lev, turned[k], stem, 16, M.BICUBIC)


def test_refusals_end_the_run_before_any_output(tmp_path):
    # (no device is touched: the directory holds no image, and the run never gets as far as to look)
    d = str(tmp_path / "empty")
    os.makedirs(d)
    for bad, word in ((["-level", "10,0,0"], "-level needs -png_device 1 or -jpeg_device 1"),
                      (["-cube", "16"], "-cube needs -png_device 1 or -jpeg_device 1"),
                      (["-png_device", "1", "-level", "10,0"], "-level must be yaw,pitch,roll"),
                      (["-png_device", "1", "-level", "10,0,0,0"], "-level must be yaw,pitch,roll"),
                      (["-png_device", "1", "-level", "10,nan,0"], "-level must be yaw,pitch,roll"),
                      (["-png_device", "1", "-level", "a,b,c"], "-level must be yaw,pitch,roll"),
                      (["-jpeg_device", "1", "-cube", "0"], "-cube must be"),
                      (["-jpeg_device", "1", "-cube", "16x16"], "-cube must be"),
                      (["-jpeg_device", "1", "-cube", "70000"], "-cube must be"),
                      (["-png_device", "1", "-cube", "16", "-cube_filter", "lanczos"], "-cube_filter must be"),
                      (["-png_device", "1", "-cube_filter", "bilinear"], "-cube_filter needs -cube")):
        out = _run(["-test_dir", d] + COMMON + bad, ok=False)
        assert out.returncode != 0 and "VrCamException" in out.stderr and word in out.stderr, (bad, out.stderr)
        assert os.listdir(d) == []
