"""CPU tier: the TIFF header parser (csrc/tiff_parse.hpp) under the address and undefined-behaviour sanitizers, by the stand-alone program
tests/cpp/tiff_parse_check.cpp -- truncation at every length, hostile IFDs, agreement with tools/image_io.hpp read_tiff -- and
pf_tiff_probe, which needs no device, on the files of tests/tiff_cases.py."""
import os
import subprocess

import pytest

import tiff_cases
import tiff_model as tm
from conftest import ROOT


def test_parser_under_sanitizers(tmp_path):
    exe = str(tmp_path / "tiff_parse_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "tiff_parse_check.cpp"), "-lz"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
    assert "FillOrder 2" in out.stdout and "ACCEPTED" not in out.stdout


def test_probe_needs_no_device(pf, synth):
    pf.build()
    cases = tiff_cases.cases(synth)
    for name, c in sorted(cases.items()):
        info = pf.tiff_probe(c.file)
        f = tm.parse(c.file)
        rows, cols, spp = c.img.shape
        assert (info.cols, info.rows, info.samples, info.compression, info.predictor) == (cols, rows, spp, f[259][0], f.get(317, [1])[0]), name
        assert info.rows_per_strip == min(f[278][0], rows) and info.n_strips == len(f[273]) and info.big_endian == (c.file[:2] == b"MM"), name
        assert info.device_decodable == 1, name
    img = tiff_cases.smooth(37, 65, 4, 3)
    assert pf.tiff_probe(tiff_cases.pillow_tiff(img, "tiff_adobe_deflate")).device_decodable == 0
    for bad, word in ((tm.write_tiff(img, 1, extra_tags=[(322, 4, [16]), (323, 4, [16]), (324, 4, [8])]), "tiled"),
                      (tm.write_tiff(img, 1, extra_tags=[(258, 3, [16, 16, 16, 16])]), "8-bit"),
                      (tm.write_tiff(img, 1, extra_tags=[(266, 3, [2])]), "FillOrder"),
                      (tm.write_tiff(img, 5)[:-40], "truncated"), (b"II*\0", "TIFF"), (b"", "TIFF")):
        with pytest.raises(pf.PanoflowError, match=word):
            pf.tiff_probe(bad)
