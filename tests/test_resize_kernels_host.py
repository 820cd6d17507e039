"""CPU tier: the resize kernels (csrc/kernels_resize.hip) compiled as host code over a stand-in for the HIP runtime header
(tests/cpp/hip_host_shim), run thread for thread by the stand-alone program tests/cpp/resize_kernels_host.cpp under the address and
undefined-behaviour sanitizers, every buffer at its exact size, with the library's own tables (csrc/resize_table.hpp); the images equal
the serial model's (tests/resize_model.py), byte for byte, for all five filters."""
import os
import subprocess

import numpy as np
import pytest

import resize_cases
import resize_model
from conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("resize_kernels_host") / "resize_kernels_host")
    src = os.path.join(ROOT, "tests", "cpp", "resize_kernels_host.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-x", "c++", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "tests", "cpp", "hip_host_shim"), "-pthread", "-o", path, src], check=True)
    return path


def host_cases():
    """(name, image, out_cols, out_rows, filter): the model's shapes and the three-piece window at every filter; a crop of the all-pairs image
    (translucent alphas against every colour) doubled with BOX; one tile-edge shape per pass; the ringing image, opaque and translucent, whose
    overshoot the clamp and the un-premultiply's min(255, ...) must catch in every channel (resize_cases.ringing_case asserts that it does)"""
    out = []
    for shape in resize_cases.MODEL_SHAPES + [resize_cases.PIECE_SHAPE]:
        cols, rows, out_cols, out_rows = shape
        for f in resize_cases.FILTER_IDS:
            out.append(("%dx%d_to_%dx%d_f%d" % (shape + (f,)), resize_cases.image(cols, rows), out_cols, out_rows, f))
    pairs = np.ascontiguousarray(resize_cases.all_pairs()[96:112, :, :])
    out.append(("pairs_box", pairs, 512, 32, resize_model.BOX))
    for shape in [s for s in resize_cases.edge_shapes() if 65 in s[2:]]:
        cols, rows, out_cols, out_rows = shape
        out.append(("edge_%dx%d_to_%dx%d" % shape, resize_cases.image(cols, rows), out_cols, out_rows, resize_model.BICUBIC))
    for shape in resize_cases.RINGING_SHAPES:
        for f in resize_cases.RINGING_FILTERS:
            for rest_alpha in (255, 128):
                img = resize_cases.ringing_case(shape, f, rest_alpha)[0]
                out.append(("ringing_%dx%d_to_%dx%d_b%dx%d_f%d_a%d" % (shape + (f, rest_alpha)), img, shape[2], shape[3], f))
    return out


def test_host_run_kernels_give_the_models_bytes(exe, tmp_path):
    cases = host_cases()
    args = []
    for k, (name, img, out_cols, out_rows, f) in enumerate(cases):
        raw = str(tmp_path / ("%d.bgra" % k))
        img.tofile(raw)
        args += [raw, str(img.shape[1]), str(img.shape[0]), str(out_cols), str(out_rows), str(f), str(tmp_path / ("%d.out" % k))]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
    differ = []
    for k, (name, img, out_cols, out_rows, f) in enumerate(cases):
        got = np.fromfile(str(tmp_path / ("%d.out" % k)), dtype=np.uint8).reshape(out_rows, out_cols, 4)
        if not np.array_equal(got, resize_model.resize(img, out_cols, out_rows, f)):
            differ.append(name)
    assert not differ, "images that are not the model's: %s" % differ


def test_host_run_single_passes_give_the_models_bytes(exe, tmp_path):
    """one pass alone with its fusions chosen (resize_cases.pass_cases): the un-premultiply and the premultiply over all 65536 pairs, and the
    clamp's raw bytes with neither"""
    cases = resize_cases.pass_cases()
    args = []
    for k, (name, img, axis, n_out, f, premul, unpremul, want, cls) in enumerate(cases):
        raw = str(tmp_path / ("%d.bgra" % k))
        img.tofile(raw)
        args += ["pass", raw, str(img.shape[1]), str(img.shape[0]), str(axis), str(n_out), str(f), str(premul), str(unpremul), str(tmp_path / ("%d.out" % k))]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
    differ = []
    for k, (name, img, axis, n_out, f, premul, unpremul, want, cls) in enumerate(cases):
        got = np.fromfile(str(tmp_path / ("%d.out" % k)), dtype=np.uint8).reshape(want.shape)
        if not np.array_equal(got, want):
            differ.append("%s: %s" % (name, resize_cases.differing_by_class(got, want, cls)))
    assert not differ, "passes that are not the model's: %s" % differ
