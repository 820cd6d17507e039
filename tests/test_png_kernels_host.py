"""CPU tier: the PNG encoder's kernels (csrc/kernels_png.hip) compiled as host code over a stand-in for the HIP runtime header
(tests/cpp/hip_host_shim), run thread for thread by the stand-alone program tests/cpp/png_kernels_host.cpp under the address and
undefined-behaviour sanitizers, every buffer at its exact size, every file inflated with zlib and compared with its image."""
import os
import subprocess

from conftest import ROOT


def test_png_kernels_on_the_host(tmp_path):
    exe = str(tmp_path / "png_kernels_host")
    src = os.path.join(ROOT, "tests", "cpp", "png_kernels_host.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-x", "c++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "tests", "cpp", "hip_host_shim"), "-pthread", "-o", exe, src, "-lz"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
