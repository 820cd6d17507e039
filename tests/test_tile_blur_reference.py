"""CPU tier of the streamed tile smoothing: the reference the GPU tests use for an explicit (step, k) is pinned against the oracle's
own smoothing, and the plan that cuts a tile's window into LDS pieces (csrc/tile_stream_plan.hpp) is checked for every geometry."""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import PKG, ROOT
from tile_blur_ref import random_inputs, tile_pass_reference


def test_tile_loop_equals_oracle_blend_smooth(orc):
    """raster loop over the active tiles + the rows/400 blur == orc_blend_smooth, bit for bit, on an 800x600 canvas"""
    cols, rows = 800, 600
    step, k1, k2 = min(cols, rows) // 200, rows // 130, rows // 400
    blend, md = random_inputs(cols, rows, step, 7)
    got, n_active = tile_pass_reference(orc, blend, md, step, k1)
    assert n_active > 10000 and not np.array_equal(got, blend)
    assert k2 > 0
    orc.lib().orc_box_blur_roi(got.ctypes.data_as(C.c_void_p), cols, rows, 0, 0, cols, rows, k2)
    assert np.array_equal(got, orc.blend_smooth(blend, md))


def test_tile_stream_plan_every_geometry(tmp_path):
    exe = str(tmp_path / "tile_stream_plan_test")
    src = os.path.join(ROOT, "tests", "cpp", "tile_stream_plan_test.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(PKG, "csrc"), "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
