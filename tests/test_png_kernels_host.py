"""CPU tier: the PNG encoder's kernels (csrc/kernels_png.hip) compiled as host code over a stand-in for the HIP runtime header
(tests/cpp/hip_host_shim), run thread for thread by the stand-alone program tests/cpp/png_kernels_host.cpp under the address and
undefined-behaviour sanitizers, every buffer at its exact size, every file inflated with zlib and compared with its image; build_code
on frequency tables that reach both length limits; the compaction scan with up to five sizes per thread against a serial prefix sum;
and the kernels' files against the serial model's (tests/png_model.py), byte for byte."""
import os
import subprocess

import pytest

import png_cases
import png_model
from conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("png_kernels_host") / "png_kernels_host")
    src = os.path.join(ROOT, "tests", "cpp", "png_kernels_host.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-x", "c++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "tests", "cpp", "hip_host_shim"), "-pthread", "-o", path, src, "-lz"], check=True)
    return path


def test_png_kernels_on_the_host(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
    assert "limit 7: longest 7" in out.stdout and "limit 15: longest 15" in out.stdout


def test_scan_with_several_elements_per_thread(exe):
    out = subprocess.run([exe, "scan"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
    for n, per in ((1, 1), (1023, 1), (1024, 1), (1025, 2), (2048, 2), (2049, 3), (5000, 5)):
        assert "k_png_scan n = %d (%d per thread)" % (n, per) in out.stdout


def host_cases():
    """the branch cases of one or two segments and few rows (every row costs the host a dozen barriers of 256 threads), and two of the
    older shapes: rows around 256 bytes, and a stream of exactly one segment and a row"""
    cases = {k: v for k, v in png_cases.branch_cases().items() if v.shape[0] <= 127}
    small = png_cases.small_cases(png_model.SEG)
    for k in ("noise_65x3", "smooth_65x3", "smooth_1x5"):
        cases[k] = small[k]
    cases["ramp_sub"] = png_cases.ramp_sub()
    return cases


def test_host_run_kernels_give_the_models_bytes(exe, tmp_path):
    cases = host_cases()
    assert {"parse_runs", "parse_chunks", "parse_segment_cross", "limit15_2736x1", "limit7_512x1", "lengths_repeat_26x1", "tail_1_4095x1", "tail_3_32x127", "threshold_equal"} <= set(cases)
    args = []
    for k, (name, img) in enumerate(sorted(cases.items())):
        raw = str(tmp_path / ("%d.bgra" % k))
        img.tofile(raw)
        args += [raw, str(img.shape[1]), str(img.shape[0]), str(tmp_path / ("%d.png" % k))]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
    differ = []
    for k, (name, img) in enumerate(sorted(cases.items())):
        with open(str(tmp_path / ("%d.png" % k)), "rb") as f:
            if f.read() != png_model.encode(img)[0]:
                differ.append(name)
    assert not differ, "files that are not the model's: %s" % differ
