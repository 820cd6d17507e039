"""pano_stitch -test_dirs ... -static_rig 1 -rig_chain 1: one rig plan from the first directory's images and every directory's whole
chain in one pf_rig_stitch_batch call give the files of -static_rig 1 alone; a directory off the rig ends the run by name before any
solve.  The argument refusals need no device."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

from conftest import PKG

EXE = os.path.join(PKG, "tools", "pano_stitch")
COLS, ROWS, STEPS = 523, 261, 3


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", PKG, "-j8", "examples"])
    return EXE


def _refused(exe, args, message):
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode != 0, r.stdout
    assert "VrCamException: " in r.stderr and message in r.stderr, r.stderr


def test_rig_chain_argument_errors(exe, tmp_path):
    a = tmp_path / "a"; a.mkdir()
    b = tmp_path / "b"; b.mkdir()
    common = ["-top_img", "top.tif", "-flow_alg", "pixflow_low"]
    dirs = "%s,%s" % (a, b)
    _refused(exe, ["-test_dirs", dirs, "-rig_chain", "1"] + common, "-rig_chain 1 needs -static_rig 1")
    _refused(exe, ["-test_dirs", dirs, "-static_rig", "0", "-rig_chain", "1"] + common, "-rig_chain 1 needs -static_rig 1")
    _refused(exe, ["-test_dir", str(a), "-rig_chain", "1"] + common, "-rig_chain 1 needs -test_dirs")
    # a valid list whose images are missing fails reading them, still before any device call
    _refused(exe, ["-test_dirs", dirs, "-static_rig", "1", "-rig_chain", "1"] + common, "failed to load image")


def _save(path, bgra):
    Image.fromarray(bgra[..., [2, 1, 0, 3]], "RGBA").save(path)


def _pixels(path):
    return np.asarray(Image.open(path).convert("RGBA"))


@pytest.mark.gpu
def test_rig_chain_run(exe, tmp_path, synth):
    planned, chained = [], []
    for k, seed in enumerate((77, 78, 79)):
        top, imgs = synth.make_stitch_set(COLS, ROWS, seed, STEPS)
        d = tmp_path / ("rig%d" % k); d.mkdir()
        _save(d / "top.tif", top.numpy())
        for i, im in enumerate(imgs):
            _save(d / ("%d.tif" % (i + 1)), im.numpy())
        p = tmp_path / ("chain%d" % k)
        shutil.copytree(d, p)
        planned.append(d); chained.append(p)
    common = ["-in_flight", "2", "-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", str(STEPS), "-static_rig", "1"]
    r = subprocess.run([exe, "-test_dirs", ",".join(map(str, planned))] + common, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "-test_dirs", ",".join(map(str, chained)), "-rig_chain", "1"] + common, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "TotalRunTime (sec) = " in r.stdout
    names = ["ProcessResult%d.png" % i for i in range(1, STEPS)] + ["FinalResult.png"]
    for d, p in zip(planned, chained):
        for name in names:
            assert (d / name).read_bytes() == (p / name).read_bytes(), "%s/%s differs from the -static_rig 1 run's" % (p.name, name)
    # a fourth directory of the rig whose 2.tif has one more transparent pixel
    odd = tmp_path / "odd"
    shutil.copytree(planned[1], odd)
    for name in names:
        os.remove(odd / name)
    im = _pixels(odd / "2.tif").copy()
    ys, xs = np.nonzero(im[..., 3] == 255)
    im[ys[len(ys) // 2], xs[len(ys) // 2]] = 0
    Image.fromarray(im, "RGBA").save(odd / "2.tif")
    r = subprocess.run([exe, "-test_dirs", ",".join(map(str, chained + [odd])), "-rig_chain", "1"] + common, capture_output=True, text=True)
    assert r.returncode != 0, r.stdout
    assert "VrCamException: -rig_chain: step 2: the alpha masks of directory %s " % odd in r.stderr, r.stderr
    assert "frame 3 differs from the rig plan at step 2 in 1 pixels" in r.stderr, r.stderr
    assert not (odd / "ProcessResult1.png").exists(), "the failed run wrote a composite"
