"""CPU tier: csrc/png_frame.hpp (CRC-32, Adler-32 combine, chunk writer, size bound of the device PNG encoder) through the stand-alone
program tests/cpp/png_frame_check.cpp, built with the address and undefined-behaviour sanitizers and run directly."""
import os
import subprocess

from conftest import ROOT


def test_png_frame_check(tmp_path):
    exe = str(tmp_path / "png_frame_check")
    src = os.path.join(ROOT, "tests", "cpp", "png_frame_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout + out.stderr
