"""CPU tier: csrc/jpeg_frame.hpp (header writer, quality scaling, code tables, XMP segment, size bound of the device JPEG encoder) through
the stand-alone program tests/cpp/jpeg_frame_check.cpp, built with the address and undefined-behaviour sanitizers and run directly.  The
headers it compares against are those of files Pillow (libjpeg-turbo) writes here, for every quality and both subsamplings."""
import io
import os
import subprocess

import numpy as np
from PIL import Image

from conftest import ROOT


def test_jpeg_frame_check(tmp_path):
    exe = str(tmp_path / "jpeg_frame_check")
    src = os.path.join(ROOT, "tests", "cpp", "jpeg_frame_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src], check=True)
    args = []
    rng = np.random.default_rng(1)
    for quality in range(1, 101):
        for sub in (0, 1):
            cols, rows = (300 + quality, 517 - quality) if sub else (quality, 1 + quality % 7)
            restart = 64 if sub == 0 else 32
            buf = io.BytesIO()
            Image.fromarray(rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8), "RGB").save(buf, format="JPEG", quality=quality, subsampling=2 if sub else 0,
                                                                                             restart_marker_blocks=restart)
            data = buf.getvalue()
            head = data[:data.index(b"\xff\xda") + 14]       # up to and including SOS
            path = str(tmp_path / ("h_%d_%d.bin" % (quality, sub)))
            with open(path, "wb") as f:
                f.write(head)
            args += [path, str(cols), str(rows), str(quality), str(sub), str(restart)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
    assert "200 headers compared" in out.stdout
