"""CPU tier: the JPEG encoder's kernels (csrc/kernels_jpeg.hip) compiled as host code over a stand-in for the HIP runtime header
(tests/cpp/hip_host_shim), run thread for thread by the stand-alone program tests/cpp/jpeg_kernels_host.cpp under the address and
undefined-behaviour sanitizers, every buffer at its exact size, on every branch case (tests/jpeg_cases.py) at its own quality and
subsampling and on the small shapes at both; the files equal the serial model's (tests/jpeg_model.py), byte for byte."""
import os
import subprocess

import pytest

import jpeg_cases
import jpeg_model
from conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("jpeg_kernels_host") / "jpeg_kernels_host")
    src = os.path.join(ROOT, "tests", "cpp", "jpeg_kernels_host.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-x", "c++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "tests", "cpp", "hip_host_shim"), "-pthread", "-o", path, src], check=True)
    return path


def host_cases():
    """(name, image, quality, subsampling): every branch case as it is named, and (the smaller ones) at the other subsampling; the small shapes at both"""
    out = []
    for name, case in sorted(jpeg_cases.branch_cases().items()):
        out.append((name, case.img, case.quality, case.subsampling))
        if case.img.shape[0] * case.img.shape[1] <= 128 * 64:     # (a workgroup is 192 or 256 host threads: the larger images once)
            out.append((name + "_other", case.img, case.quality, 1 - case.subsampling))
    for name, img in sorted(jpeg_cases.small_shapes().items()):
        out += [(name + "_444", img, 90, 0), (name + "_420", img, 50, 1)]
    return out


def test_host_run_kernels_give_the_models_bytes(exe, tmp_path):
    cases = host_cases()
    assert set(jpeg_cases.BRANCHES) <= {c[0] for c in cases}
    args = []
    for k, (name, img, quality, sub) in enumerate(cases):
        raw = str(tmp_path / ("%d.bgra" % k))
        img.tofile(raw)
        args += [raw, str(img.shape[1]), str(img.shape[0]), str(quality), str(sub), str(tmp_path / ("%d.jpg" % k))]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
    differ = []
    for k, (name, img, quality, sub) in enumerate(cases):
        with open(str(tmp_path / ("%d.jpg" % k)), "rb") as f:
            if f.read() != jpeg_model.encode(img, quality, sub):
                differ.append(name)
    assert not differ, "files that are not the model's: %s" % differ
