"""pano_stitch -test_dirs: argument errors are refused with a VrCamException message before any device call (no GPU needed)."""
import os
import subprocess

import pytest

from conftest import PKG

EXE = os.path.join(PKG, "tools", "pano_stitch")


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", PKG, "-j8", "examples"])
    return EXE


def _refused(exe, args, message):
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode != 0, r.stdout
    assert "VrCamException: " in r.stderr and message in r.stderr, r.stderr


def test_test_dirs_argument_errors(exe, tmp_path):
    a = tmp_path / "a"; a.mkdir()
    b = tmp_path / "b"; b.mkdir()
    common = ["-top_img", "top.tif", "-flow_alg", "pixflow_low"]
    dirs = "%s,%s" % (a, b)
    _refused(exe, ["-test_dirs", dirs, "-test_dir", str(a)] + common, "-test_dirs and -test_dir are exclusive")
    _refused(exe, ["-test_dirs", dirs, "-fused", "0"] + common, "-fused 0 is not supported")
    _refused(exe, ["-test_dirs", dirs, "-visualize", "1"] + common, "does not support -visualize 1")
    _refused(exe, ["-test_dirs", ""] + common, "empty directory list")
    _refused(exe, ["-test_dirs", "%s,,%s" % (a, b)] + common, "empty directory name")
    _refused(exe, ["-test_dirs", "%s,%s" % (a, tmp_path / "missing")] + common, "no such directory: %s" % (tmp_path / "missing"))
    _refused(exe, ["-test_dirs", dirs, "-in_flight", "0"] + common, "-in_flight must be 1..32")
    _refused(exe, ["-test_dirs", dirs, "-flow_alg", "pixflow_low"], "missing required command line argument: top_img")
    # a valid list whose images are missing fails reading them, still before any device call
    _refused(exe, ["-test_dirs", dirs] + common, "failed to load image")
