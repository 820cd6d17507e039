"""pano_stitch -test_dirs ... -static_rig 1: the directories of one rig run on one stitch plan per step and get the files of the
run without the flag; a directory whose masks differ ends the run by name.  The argument refusals need no device."""
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


def test_static_rig_argument_errors(exe, tmp_path):
    a = tmp_path / "a"; a.mkdir()
    b = tmp_path / "b"; b.mkdir()
    common = ["-top_img", "top.tif", "-flow_alg", "pixflow_low"]
    dirs = "%s,%s" % (a, b)
    _refused(exe, ["-test_dir", str(a), "-static_rig", "1"] + common, "-static_rig 1 needs -test_dirs")
    _refused(exe, ["-inputs", "4", "-test_dir", str(a), "-static_rig", "1"] + common, "-static_rig 1 needs -test_dirs")
    _refused(exe, ["-test_dirs", dirs, "-static_rig", "1", "-test_dir", str(a)] + common, "-test_dirs and -test_dir are exclusive")
    _refused(exe, ["-test_dirs", dirs, "-static_rig", "1", "-fused", "0"] + common, "-fused 0 is not supported")
    _refused(exe, ["-test_dirs", dirs, "-static_rig", "1", "-visualize", "1"] + common, "does not support -visualize 1")
    _refused(exe, ["-test_dirs", dirs, "-static_rig", "1", "-inputs", "4"] + common, "does not support -inputs")
    # a valid list whose images are missing fails reading them, still before any device call
    _refused(exe, ["-test_dirs", dirs, "-static_rig", "1"] + common, "failed to load image")


def _save(path, bgra):
    Image.fromarray(bgra[..., [2, 1, 0, 3]], "RGBA").save(path)


def _pixels(path):
    return np.asarray(Image.open(path).convert("RGBA"))


@pytest.mark.gpu
def test_static_rig_run(exe, tmp_path, synth):
    plain, planned = [], []
    for k, seed in enumerate((77, 78, 79)):
        top, imgs = synth.make_stitch_set(COLS, ROWS, seed, STEPS)
        d = tmp_path / ("plain%d" % k); d.mkdir()
        _save(d / "top.tif", top.numpy())
        for i, im in enumerate(imgs):
            _save(d / ("%d.tif" % (i + 1)), im.numpy())
        p = tmp_path / ("rig%d" % k)
        shutil.copytree(d, p)
        plain.append(d); planned.append(p)
    common = ["-in_flight", "3", "-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", str(STEPS)]
    r = subprocess.run([exe, "-test_dirs", ",".join(map(str, plain))] + common, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "-test_dirs", ",".join(map(str, planned)), "-static_rig", "1"] + common, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for i in range(1, STEPS + 1):
        assert "Part%d Finished!RUNTIME (sec) = " % i in r.stdout
    names = ["ProcessResult%d.png" % i for i in range(1, STEPS)] + ["FinalResult.png"]
    for d, p in zip(plain, planned):
        for name in names:
            assert np.array_equal(_pixels(d / name), _pixels(p / name)), "%s/%s differs from the run without -static_rig" % (p.name, name)
    # a fourth directory of the rig whose 2.tif has one more transparent pixel
    odd = tmp_path / "odd"
    shutil.copytree(plain[1], odd)
    for name in names:
        os.remove(odd / name)
    im = _pixels(odd / "2.tif").copy()
    ys, xs = np.nonzero(im[..., 3] == 255)
    im[ys[len(ys) // 2], xs[len(ys) // 2]] = 0
    Image.fromarray(im, "RGBA").save(odd / "2.tif")
    r = subprocess.run([exe, "-test_dirs", ",".join(map(str, planned + [odd])), "-static_rig", "1"] + common, capture_output=True, text=True)
    assert r.returncode != 0, r.stdout
    assert "VrCamException: -static_rig: step 2: the alpha masks of directory %s " % odd in r.stderr, r.stderr
    assert "frame 3 differs from the stitch plan in 1 pixels" in r.stderr, r.stderr
    assert not (odd / "ProcessResult2.png").exists(), "the failed step wrote a composite"


@pytest.mark.gpu
def test_cpp_stitch_plan_and_planned_step(tmp_path, synth):
    """stitch_tools::StitchPlan (getMap / getBlend / overlapPixels) and the stitchStep overload that takes one, through
    examples/stitch_pair: the planned composite, the plan's map and its ramp are the object-by-object sequence's."""
    exe = os.path.join(PKG, "examples", "stitch_pair")
    top, imgs = synth.make_stitch_set(COLS, ROWS, 77, 1)
    (tmp_path / "L.bgra").write_bytes(imgs[0].numpy().tobytes())
    (tmp_path / "R.bgra").write_bytes(top.numpy().tobytes())
    prefix = str(tmp_path / "out")
    r = subprocess.run([exe, str(COLS), str(ROWS), str(tmp_path / "L.bgra"), str(tmp_path / "R.bgra"), "pixflow_search_20", prefix, "plan"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    read = lambda suffix: open(prefix + suffix, "rb").read()
    assert read(".planned.bgra") == read(".final.bgra"), "the planned stitchStep differs from the object-by-object sequence"
    assert read(".plan_map.u8") == read(".map.u8")
    assert read(".plan_blend.f32") == read(".blend.f32")
    mp = np.frombuffer(read(".map.u8"), np.uint8)
    assert "plan overlap pixels = %d" % int((mp == 150).sum()) in r.stdout, r.stdout
