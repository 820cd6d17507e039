"""CPU tier: the JPEG encoder's kernels (csrc/kernels_jpeg.hip) compiled as host code over a stand-in for the HIP runtime header
(tests/cpp/hip_host_shim), run thread for thread by the stand-alone program tests/cpp/jpeg_kernels_host.cpp under the address and
undefined-behaviour sanitizers, every buffer at its exact size, on every branch case (tests/jpeg_cases.py) at its own quality and
subsampling and on the small shapes at both, at the product's restart interval; on two cases at every kind of interval the coder admits
(jpeg_cases.INTERVALS: one MCU, a partial and a full second round of its threads); the files equal the serial model's
(tests/jpeg_model.py), byte for byte.  And the compaction scan alone, with several elements per thread."""
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
    """(name, image, quality, subsampling, restart), at the product's interval: every branch case as it is named, and (the smaller ones)
    at the other subsampling; the small shapes at both"""
    out = []
    for name, case in sorted(jpeg_cases.branch_cases().items()):
        out.append((name, case.img, case.quality, case.subsampling))
        if case.img.shape[0] * case.img.shape[1] <= 128 * 64:     # (a workgroup is 192 or 256 host threads: the larger images once)
            out.append((name + "_other", case.img, case.quality, 1 - case.subsampling))
    for name, img in sorted(jpeg_cases.small_shapes().items()):
        out += [(name + "_444", img, 90, 0), (name + "_420", img, 50, 1)]
    return [c + (jpeg_model.RESTART[c[3]],) for c in out]


def interval_cases():
    """two cases at every admitted kind of interval, both subsamplings: noise whose intervals span several windows, and 17 x 17 (34 x 34)
    MCUs, whose intervals cross MCU rows and whose markers wrap"""
    out = []
    for name in ("hostile_noise_q100", "marker_index_wraps"):
        case = jpeg_cases.branch_cases()[name]
        for sub in (0, 1):
            out += [("%s_%s_R%d" % (name, "420" if sub else "444", r), case.img, case.quality, sub, r) for r in jpeg_cases.INTERVALS[sub]]
    return out


def _run_and_compare(exe, tmp_path, cases, processes=1):
    """the cases dealt out to `processes` runs of the program side by side (its threads mostly wait at barriers)"""
    args = [[] for _ in range(processes)]
    for k, (name, img, quality, sub, restart) in enumerate(cases):
        raw = str(tmp_path / ("%d.bgra" % k))
        img.tofile(raw)
        args[k % processes] += [raw, str(img.shape[1]), str(img.shape[0]), str(quality), str(sub), str(restart), str(tmp_path / ("%d.jpg" % k))]
    runs = [subprocess.Popen([exe] + a, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for a in args if a]
    for run in runs:
        stdout, stderr = run.communicate(timeout=900)
        assert run.returncode == 0 and stdout.strip().endswith("ok"), stdout[-3000:] + stderr[-3000:]
    differ = []
    for k, (name, img, quality, sub, restart) in enumerate(cases):
        with open(str(tmp_path / ("%d.jpg" % k)), "rb") as f:
            if f.read() != jpeg_model.encode(img, quality, sub, restart):
                differ.append(name)
    assert not differ, "files that are not the model's: %s" % differ


def test_host_run_kernels_give_the_models_bytes(exe, tmp_path):
    cases = host_cases()
    assert set(jpeg_cases.BRANCHES) <= {c[0] for c in cases}
    _run_and_compare(exe, tmp_path, cases)


def test_host_run_kernels_give_the_models_bytes_at_every_admitted_interval(exe, tmp_path):
    cases = interval_cases()
    assert len(cases) == 24 and {c[4] for c in cases if c[3]} == {1, 2, 31, 33, 63, 64} and {c[4] for c in cases if not c[3]} == {1, 2, 63, 65, 127, 128}
    _run_and_compare(exe, tmp_path, cases, processes=8)


def test_host_run_kernels_give_the_models_bytes_at_the_largest_side_across(exe, tmp_path):
    """65535 x 9: 256 tiles of k_jpeg_blocks across and a last MCU column a pixel short.  (9 x 65535 takes the host three times as long,
    some 20 s, and runs on the device only: tests/test_gpu_jpeg_intervals.py)"""
    img = jpeg_cases.long_image(True)
    _run_and_compare(exe, tmp_path, [("65535x9_444", img, 90, 0, jpeg_model.RESTART[0]), ("65535x9_420", img, 90, 1, jpeg_model.RESTART[1])], processes=2)


def test_an_interval_that_does_not_fit_is_refused(exe, tmp_path):
    img = jpeg_cases.smooth(16, 16)
    raw = str(tmp_path / "a.bgra")
    img.tofile(raw)
    for sub in (0, 1):
        for restart in (0, jpeg_cases.REFUSED_INTERVAL[sub]):
            out = subprocess.run([exe, raw, "16", "16", "90", str(sub), str(restart), str(tmp_path / "a.jpg")], capture_output=True, text=True, timeout=60)
            assert out.returncode == 2 and "does not fit" in out.stdout


def test_scan_with_several_elements_per_thread(exe):
    out = subprocess.run([exe, "scan"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
    for n, per in ((1, 1), (1023, 1), (1024, 1), (1025, 2), (2048, 2), (2049, 3), (5000, 5)):
        assert "n = %d (%d per thread)" % (n, per) in out.stdout
