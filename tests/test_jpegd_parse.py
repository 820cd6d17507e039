"""CPU tier: the JPEG header parser (csrc/jpeg_parse.hpp) under the address and undefined-behaviour sanitizers, by the stand-alone
program tests/cpp/jpeg_parse_check.cpp: every truncation of a file up to its scan, hostile lengths and counts, one patched header per
refusal of the contract, a progressive and a CMYK file of Pillow's; what it accepts, what it refuses and why, and the tables it derives
are the model's (tests/jpegd_model.py parse).  And pf_jpeg_probe, which needs no device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import jpegd_cases as jc
import jpegd_model as jm
from conftest import ROOT


def _model_line(data):
    try:
        i = jm.parse(data)
    except jm.Refused as e:
        return "P %s" % e
    h = 1469598103934665603
    def mix(v):
        nonlocal h
        h = ((h ^ (v & 0xffffffff)) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    for c in range(i["ncomp"]):
        for t in (i["dc"][c], i["ac"][c]):
            for l in range(1, 18):
                mix(t["maxcode"][l])
            for l in range(1, 17):
                mix(0 if t["maxcode"][l] < 0 else t["valoff"][l])
        for v in i["quant"][c]:
            mix(int(v))
    return "A %d %d %d %d %d %d %d %d %d" % (i["cols"], i["rows"], i["ncomp"], i["hs"], i["vs"], i["restart"], i["begin"], i["end"], h)


def hostile(base):
    """lengths and counts that point past the buffer, or nowhere"""
    out = []
    for marker in (0xE0, 0xDB, 0xC0, 0xC4, 0xDA):
        k = base.index(bytes([0xFF, marker]))
        for L in (0, 1, 2, 3, 0xFFFF, len(base) - k - 2, len(base) - k - 1):
            v = bytearray(base); v[k + 2:k + 4] = struct.pack(">H", L & 0xFFFF); out.append(bytes(v))
    k = base.index(b"\xff\xc4")
    for count in (255, 200, 17):
        v = bytearray(base); v[k + 5] = count; out.append(bytes(v))            # a DHT that counts more symbols than it holds
        v = bytearray(base); v[k + 5 + 15] = count; out.append(bytes(v))
    v = bytearray(base); v[k + 4] = 0x24; out.append(bytes(v))                  # table class 2, id 4
    k = base.index(b"\xff\xc0")
    for nf in (0, 2, 4, 5, 255):
        v = bytearray(base); v[k + 9] = nf; out.append(bytes(v))
    k = base.index(b"\xff\xda")
    for ns in (0, 1, 2, 4, 255):
        v = bytearray(base); v[k + 4] = ns; out.append(bytes(v))
    out.append(base[:k + 14] + b"\xff" * 40)                                    # fill bytes and no end
    out.append(base[:2] + b"\xff" * 100)
    out.append(base[:2] + b"\x00" * 100)
    return out


def test_parser_under_sanitizers_agrees_with_the_model(tmp_path):
    exe = str(tmp_path / "jpeg_parse_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "jpeg_parse_check.cpp")], check=True)
    base = jc.pil_jpeg(jc.scene(32, 24, 1), 80, "420", False, 2)
    begin = jm.parse(base)["begin"]
    files = [base[:k] for k in range(begin + 3)] + [base[:k] + b"\xff\xd9" for k in range(begin + 3)]
    files += hostile(base)
    refused = sorted(jc.refusals().items())
    files += [d for _, (d, _) in refused]
    files += [d for _, d in jc.grid_cases()] + [d for _, d in jc.interval_cases()]
    pack = str(tmp_path / "in.pack"); out = str(tmp_path / "out.txt")
    with open(pack, "wb") as f:
        f.write(struct.pack("<I", len(files)))
        for d in files:
            f.write(struct.pack("<I", len(d))); f.write(d)
    run = subprocess.run([exe, pack, out], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), run.stdout[-3000:] + run.stderr[-3000:]
    lines = open(out).read().split("\n")[:-1]
    assert len(lines) == len(files)
    wrong = [(k, line, _model_line(d)) for k, (d, line) in enumerate(zip(files, lines)) if line != _model_line(d)]
    assert not wrong, "parser and model disagree (index, parser, model): %s" % wrong[:10]
    n = 2 * (begin + 3) + len(hostile(base))
    assert all(l.startswith("P") for l in lines[:begin + 3])                     # no truncation up to the scan is accepted
    for (name, (_, word)), line in zip(refused, lines[n:n + len(refused)]):
        assert line.startswith("P") and word in line, (name, line)
    assert all(l.startswith("A") for l in lines[n + len(refused):])


def test_probe_needs_no_device(pf):
    pf.build()
    for name, data in jc.grid_cases() + jc.interval_cases():
        info = pf.jpeg_probe(data); m = jm.parse(data)
        sub = 0 if m["ncomp"] == 1 else {(1, 1): 444, (2, 1): 422, (2, 2): 420}[(m["hs"], m["vs"])]
        assert (info.cols, info.rows, info.components, info.subsampling, info.restart_interval, info.device_decodable) == \
               (m["cols"], m["rows"], m["ncomp"], sub, m["restart"], 1), name
    for name, (data, word) in sorted(jc.refusals().items()):
        info = pf.jpeg_probe(data)
        assert info.device_decodable == 0 and word in info.reason.decode(), name
    for bad in (b"", b"\xff", b"II*\0"):
        with pytest.raises(pf.PanoflowError, match="not a JPEG"):
            pf.jpeg_probe(bad)
