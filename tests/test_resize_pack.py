"""CPU tier: RzAcc::pack() of the resize kernels (csrc/kernels_resize.hip), compiled as host code over the stand-in for the HIP runtime
header, against its specification min(255, max(0, (int)c >> 22)) in every byte position for ALL 2^32 accumulator values
(tests/cpp/resize_pack_check.cpp).  pack() is written as a clamp of the sum followed by the shift, so that no kernel holds gfx950's
v_ashr_pk_u8_i32 (tests/test_pack_isa.py); this holds the rewrite to the bytes of the plain form.

The set is not reduced.  Measured: the loop takes 7.0 s on the 8 host threads it uses at most (g++ -O2; 51 s of CPU time, which is
what a single-CPU host would wait); the compile takes about 2 s."""
import os
import subprocess

from conftest import ROOT


def test_pack_equals_its_specification_for_every_accumulator(tmp_path):
    exe = str(tmp_path / "resize_pack_check")
    src = os.path.join(ROOT, "tests", "cpp", "resize_pack_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++20", "-x", "c++", "-ffp-contract=off", "-I", os.path.join(ROOT, "tests", "cpp", "hip_host_shim"), "-pthread",
                    "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip() == "ok 4294967296", out.stdout[-2000:] + out.stderr[-2000:]
