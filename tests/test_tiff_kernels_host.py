"""CPU tier: the TIFF decoder's kernels (csrc/kernels_tiff.hip) compiled as host code over the stand-in for the HIP runtime header
(tests/cpp/hip_host_shim) and run thread for thread by tests/cpp/tiff_kernels_host.cpp under the address and undefined-behaviour
sanitizers, every buffer at its exact size.  Every case of tests/tiff_cases.py decodes to its image; every malformed stream sets its
strip's status to what the serial model (tests/tiff_model.py) says, decodes the same bytes before it stops, produces no sanitizer report
and terminates."""
import os
import subprocess

import numpy as np
import pytest

import tiff_cases
import tiff_model as tm
from conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tiff_kernels_host") / "tiff_kernels_host")
    src = os.path.join(ROOT, "tests", "cpp", "tiff_kernels_host.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-x", "c++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "tests", "cpp", "hip_host_shim"), "-pthread", "-o", path, src], check=True)
    return path


def run(exe, tmp_path, files):
    """{name: file bytes} -> {name: (BGRA image, [(decoded, expected, reason)])}"""
    args, names = [], sorted(files)
    for k, name in enumerate(names):
        p = str(tmp_path / ("%d" % k))
        with open(p + ".tif", "wb") as f:
            f.write(files[name])
        args += [p + ".tif", p + ".bgra", p + ".status"]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
    res = {}
    for k, name in enumerate(names):
        f = tm.parse(files[name])
        img = np.fromfile(str(tmp_path / ("%d.bgra" % k)), np.uint8).reshape(f[257][0], f[256][0], 4)
        status = [tuple(int(v) for v in line.split()) for line in open(str(tmp_path / ("%d.status" % k)))]
        res[name] = (img, status)
    return res


def test_code_geometry(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]


def test_every_case_decodes_to_its_image(exe, tmp_path, synth):
    cases = tiff_cases.cases(synth)
    res = run(exe, tmp_path, {k: c.file for k, c in cases.items()})
    wrong = [k for k, c in cases.items() if not np.array_equal(res[k][0], tm.expected_bgra(c.img)) or any(a != b or r for a, b, r in res[k][1])]
    assert not wrong, wrong


def test_malformed_streams_are_refused_as_the_model_says(exe, tmp_path):
    bad = tiff_cases.malformed()
    res = run(exe, tmp_path, bad)
    for name, data in sorted(bad.items()):
        want_img, want_status = tm.decode(data)
        img, status = res[name]
        assert any(a != b for a, b, _ in status), name
        # a strip that filled up carries no reason; a short one carries the model's
        assert [(a, b, r if a != b else 0) for a, b, r in status] == [(a, b, r if a != b else 0) for a, b, r in want_status], name
        assert np.array_equal(img, want_img), name   # the bytes decoded before the stop, zeros after
    assert len(res["random_lzw_strips"][1]) == 200
