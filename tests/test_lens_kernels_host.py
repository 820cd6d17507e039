"""CPU tier: the lens remap kernel (csrc/kernels_lens.hip) compiled as host code over a stand-in for the HIP runtime header
(tests/cpp/hip_host_shim), run thread for thread by the stand-alone program tests/cpp/lens_kernels_host.cpp under the address and
undefined-behaviour sanitizers with -ffp-contract=off, every buffer at its exact size, with the library's own tables
(csrc/reproject_math.hpp); the canvases and the coordinate planes equal the model's (tests/lens_model.py), bit for bit, on the case
list the device test uses (tests/lens_cases.py).  The cases run as batches of three with three different lenses (one launch, one
image per blockIdx.z), with fewer workgroups than tiles."""
import os
import subprocess

import numpy as np
import pytest

import lens_cases
from conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lens_kernels_host") / "lens_kernels_host")
    src = os.path.join(ROOT, "tests", "cpp", "lens_kernels_host.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-x", "c++", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "tests", "cpp", "hip_host_shim"), "-pthread", "-o", path, src], check=True)
    return path


def _lens_line(lens):
    nums = [lens.focal_px, lens.a, lens.b, lens.c, lens.dd, lens.shift_x, lens.shift_y, lens.min_cos] + lens.rot
    return "%d %d %d %d %s\n" % ((lens.model,) + lens.crop + (" ".join(float(x).hex() for x in nums),))


def test_host_run_kernel_gives_the_models_bits(exe, tmp_path):
    cases = lens_cases.cases()
    for p in lens_cases.PHOTOS:
        lens_cases.photo_cached(p).tofile(str(tmp_path / (p + ".bgra")))
    # batches of three cases that share what a launch shares (photo, canvas, filter), in the list's order otherwise
    shared = {}
    for c in cases:
        shared.setdefault((c.photo, c.cols, c.rows, c.lens.filter), []).append(c)
    order, threes = [], 0
    with open(str(tmp_path / "cases.txt"), "w") as f:
        for (p, w, h, flt), members in shared.items():
            rows, cols = lens_cases.photo_cached(p).shape[:2]
            for at in range(0, len(members), 3):
                group = members[at:at + 3]
                threes += len(group) == 3 and len({_lens_line(c.lens) for c in group}) == 3
                f.write("group %d %s %d %d %d %d %d\n" % (len(group), str(tmp_path / (p + ".bgra")), cols, rows, w, h, flt))
                for c in group:
                    f.write(_lens_line(c.lens))
                order.extend(group)
    assert len(order) == len(cases) and threes >= len(cases) // 4
    out = subprocess.run([exe, str(tmp_path / "cases.txt"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("%d cases ok" % len(cases)), out.stdout[-3000:] + out.stderr[-3000:]
    blob = np.fromfile(str(tmp_path / "out.bin"), dtype=np.uint8)
    at, differ = 0, []
    for case in order:
        w, h = case.cols, case.rows
        n = w * h * 4
        img = blob[at:at + n].reshape(h, w, 4)
        fx = blob[at + n:at + 2 * n].view(np.int32).reshape(h, w)
        fy = blob[at + 2 * n:at + 3 * n].view(np.int32).reshape(h, w)
        at += 3 * n
        mfx, mfy = lens_cases.model_coords(case)
        if not (np.array_equal(fx, mfx) and np.array_equal(fy, mfy)):
            differ.append(case.name + " (coordinates)")
        elif not np.array_equal(img, lens_cases.model_image(case)):
            differ.append(case.name)
    assert at == blob.size
    assert not differ, "%d of %d cases are not the model's: %s" % (len(differ), len(cases), differ[:20])
