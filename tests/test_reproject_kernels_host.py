"""CPU tier: the reprojection kernel (csrc/kernels_reproject.hip) compiled as host code over a stand-in for the HIP runtime header
(tests/cpp/hip_host_shim), run thread for thread by the stand-alone program tests/cpp/reproject_kernels_host.cpp under the address and
undefined-behaviour sanitizers with -ffp-contract=off, every buffer at its exact size, with the library's own tables
(csrc/reproject_math.hpp); the images and the coordinate planes equal the model's (tests/reproject_model.py), bit for bit, on the
case list the device test uses (tests/reproject_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

import reproject_cases
from conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("reproject_kernels_host") / "reproject_kernels_host")
    src = os.path.join(ROOT, "tests", "cpp", "reproject_kernels_host.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-x", "c++", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "tests", "cpp", "hip_host_shim"), "-pthread", "-o", path, src], check=True)
    return path


def test_host_run_kernel_gives_the_models_bits(exe, tmp_path):
    cases = reproject_cases.cases()
    for s in reproject_cases.SOURCES:
        reproject_cases.source_cached(s).tofile(str(tmp_path / (s + ".bgra")))
    with open(str(tmp_path / "cases.txt"), "w") as f:
        for (name, s, proj, w, h, face, hfov, r, flt) in cases:
            rows, cols = reproject_cases.source_cached(s).shape[:2]
            nums = [float(hfov).hex()] + [float(x).hex() for x in reproject_cases.ROTATIONS[r]]
            f.write("%s %d %d %d %d %d %d %d %s\n" % (str(tmp_path / (s + ".bgra")), cols, rows, w, h, proj, face, flt, " ".join(nums)))
    out = subprocess.run([exe, str(tmp_path / "cases.txt"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("%d cases ok" % len(cases)), out.stdout[-3000:] + out.stderr[-3000:]
    blob = np.fromfile(str(tmp_path / "out.bin"), dtype=np.uint8)
    at, differ = 0, []
    for case in cases:
        w, h = case[3], case[4]
        n = w * h * 4
        img = blob[at:at + n].reshape(h, w, 4)
        fx = blob[at + n:at + 2 * n].view(np.int32).reshape(h, w)
        fy = blob[at + 2 * n:at + 3 * n].view(np.int32).reshape(h, w)
        at += 3 * n
        mfx, mfy = reproject_cases.model_coords(case)
        if not (np.array_equal(fx, mfx) and np.array_equal(fy, mfy)):
            differ.append(case[0] + " (coordinates)")
        elif not np.array_equal(img, reproject_cases.model_image(case)):
            differ.append(case[0])
    assert at == blob.size
    assert not differ, "%d of %d cases are not the model's: %s" % (len(differ), len(cases), differ[:20])
