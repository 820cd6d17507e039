"""CPU tier of the flow visualisers (CPU/OpticalFlow.cpp:147-204): csrc/libm_exact.hpp's atan2f_exact equals the host libm's atan2f
bit for bit, the restated HSV2BGR has the properties OpenCV's conversion implies, and the serial host reference
(tests/cpp/flow_vis_ref.cpp, which the GPU tests hold the kernels to) gives hand-checked pixels on a small flow."""
import ctypes as C
import os
import platform
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "flow_vis_ref.cpp")


def build_ref(outdir):
    so = os.path.join(str(outdir), "libflow_vis_ref.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", "-o", so, SRC], check=True)
    lib = C.CDLL(so)
    lib.ref_atan2f_check.restype = C.c_long
    lib.ref_atan2f_check.argtypes = [C.c_long, C.c_int]
    for f in ("ref_grey_disparity", "ref_color_wheel"):
        getattr(lib, f).argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    for f in ("ref_vector_field", "ref_panel"):
        getattr(lib, f).argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.ref_hsv2bgr_all.argtypes = [C.c_void_p]
    return lib


class Ref:
    """numpy wrappers of the host reference"""

    def __init__(self, lib):
        self.l = lib

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(C.c_void_p)

    def grey(self, flow):
        f = np.ascontiguousarray(flow, np.float32); rows, cols, _ = f.shape
        out = np.empty((rows, cols), np.uint8); self.l.ref_grey_disparity(self._p(f), cols, rows, self._p(out)); return out

    def wheel(self, flow):
        f = np.ascontiguousarray(flow, np.float32); rows, cols, _ = f.shape
        out = np.empty((rows, cols, 3), np.uint8); self.l.ref_color_wheel(self._p(f), cols, rows, self._p(out)); return out

    def field(self, flow, image):
        f = np.ascontiguousarray(flow, np.float32); im = np.ascontiguousarray(image, np.uint8); rows, cols, _ = f.shape
        out = np.empty((rows, cols, 4), np.uint8); self.l.ref_vector_field(self._p(f), self._p(im), cols, rows, self._p(out)); return out

    def panel(self, flow, image):
        f = np.ascontiguousarray(flow, np.float32); im = np.ascontiguousarray(image, np.uint8); rows, cols, _ = f.shape
        out = np.empty((rows, 3 * cols, 4), np.uint8); self.l.ref_panel(self._p(f), self._p(im), cols, rows, self._p(out)); return out


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return Ref(build_ref(tmp_path_factory.mktemp("flow_vis_ref")))


def test_atan2f_restatement_equals_host_libm(ref):
    # all 2^32 y with x = +-1, 2^30 random (y, x) bit patterns, the special-case grid (flow_vis_ref.cpp: ref_atan2f_check)
    bad = ref.l.ref_atan2f_check(1 << 30, max(1, min(os.cpu_count() or 1, 16)))
    lib, ver = platform.libc_ver()
    if bad and (lib, ver) != ("glibc", "2.35"):
        # the restatement is glibc 2.35's float atan2f (fdlibm); a different libm is a property of the host, not a defect
        pytest.skip("host libm is %s %s, not the glibc 2.35 that csrc/libm_exact.hpp restates: %d mismatches" % (lib, ver, bad))
    assert bad == 0


def test_hsv2bgr_properties(ref):
    out = np.empty((181, 256, 256, 3), np.uint8)
    ref.l.ref_hsv2bgr_all(out.ctypes.data_as(C.c_void_p))
    v = np.arange(256, dtype=np.uint8)
    # S = 0: grey at the value
    assert (out[:, 0, :, :] == v[None, :, None]).all()
    # V is the largest channel, and equals V
    assert (out.max(axis=3) == v[None, None, :]).all()
    # the hue wraps: H = 0 and H = 180 are the same colour
    assert np.array_equal(out[0], out[180])
    # the six primaries / secondaries at full S, V (OpenCV's sector table, BGR)
    assert out[0, 255, 255].tolist() == [0, 0, 255] and out[60, 255, 255].tolist() == [0, 255, 0] and out[120, 255, 255].tolist() == [255, 0, 0]
    assert out[30, 255, 255].tolist() == [0, 255, 255] and out[90, 255, 255].tolist() == [255, 255, 0] and out[150, 255, 255].tolist() == [255, 0, 255]


def test_host_reference_hand_checked_pixels(ref):
    rows, cols = 40, 50
    flow = np.zeros((rows, cols, 2), np.float32)
    flow[..., 0] = 3.0
    # a constant x component: normalize's scale is 0 -> all zeros
    assert (ref.grey(flow) == 0).all()
    # a ramp: min -> 0, max -> 255
    ramp = flow.copy(); ramp[..., 0] = np.arange(cols, dtype=np.float32)[None, :]
    g = ref.grey(ramp)
    assert g[:, 0].tolist() == [0] * rows and g[:, -1].tolist() == [255] * rows
    # zero vector: hue byte 0 (NaN direction), S = V = int(255 * 0.25) = 63 -> HSV2BGR(0, 63, 63)
    z = np.zeros((rows, cols, 2), np.float32)
    w = ref.wheel(z)
    s = 63 / 255.0
    expect = [round(63 * (1 - s)), round(63 * (1 - s)), 63]   # sector 0: b = v (1 - s), g = v (1 - s h) with h = 0, r = v
    assert w[5, 5].tolist() == expect
    # flow along +x: hue (0 + pi) / 2 pi = 0.5 -> H = 90 (cyan); magnitude >= max(cols, rows) / 20 -> full brightness
    px = np.zeros((rows, cols, 2), np.float32); px[..., 0] = 10.0
    assert ref.wheel(px)[0, 0].tolist() == [255, 255, 0]
    # one arrow on a blank image touches only pixels within 2 px of its segment (25 x 25: the grid point (12, 12) is the only one)
    img = np.full((25, 25, 4), 200, np.uint8)
    one = np.zeros((25, 25, 2), np.float32)
    one[12, 12] = (5.0, 3.0)
    out = ref.field(one, img)
    changed = np.argwhere((out != img).any(axis=2))
    assert len(changed) > 0
    mag = np.hypot(5.0, 3.0); fx, fy = np.float32(5.0) / np.float32(mag + 0.1), np.float32(3.0) / np.float32(mag + 0.1)
    p0 = np.array([12.0, 12.0]); p1 = np.array([int(12 + fx * 7), int(12 + fy * 7)], float)
    for y, x in changed:
        q = np.array([x, y], float); d = p1 - p0
        t = np.clip(np.dot(q - p0, d) / np.dot(d, d), 0, 1)
        assert np.linalg.norm(q - (p0 + t * d)) <= 2.0, (x, y)
    # the arrow darkens its own pixels (colour 0, 0, 0) and raises alpha towards 255
    assert out[12, 13, 0] < 200 and out[12, 13, 3] > 200
