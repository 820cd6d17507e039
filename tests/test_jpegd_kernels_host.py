"""CPU tier: the JPEG decoder's kernels (csrc/kernels_jpegd.hip) compiled as host code over a stand-in for the HIP runtime header
(tests/cpp/hip_host_shim), run thread for thread by the stand-alone program tests/cpp/jpegd_kernels_host.cpp under the address and
undefined-behaviour sanitizers, every buffer at its exact size.  Every case (tests/jpegd_cases.py) at the product's subsequence size and
the seam cases at the smallest as well: pixels, coefficient planes, component planes and final entry states equal the serial model's
(tests/jpegd_model.py).  Every single-bit flip and every truncation of one small scan, and 200 scans of random bytes: the kernels accept
and refuse what the model does, stop at the same MCU, and give the model's pixels where the damaged scan is accepted."""
import os
import struct
import subprocess

import numpy as np
import pytest

import jpegd_cases as jc
import jpegd_model as jm
from conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("jpegd_kernels_host") / "jpegd_kernels_host")
    src = os.path.join(ROOT, "tests", "cpp", "jpegd_kernels_host.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-x", "c++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "tests", "cpp", "hip_host_shim"), "-pthread", "-o", path, src], check=True)
    return path


def _decode_all(exe, tmp_path, S, cases, processes=8):
    """(name, file) cases through the program at subsequence size S -> per case the parsed output"""
    args = [[] for _ in range(processes)]
    for k, (name, data) in enumerate(cases):
        src = str(tmp_path / ("%d_%d.jpg" % (S, k)))
        with open(src, "wb") as f:
            f.write(data)
        args[k % processes] += [src, str(tmp_path / ("%d_%d.bin" % (S, k)))]
    runs = [subprocess.Popen([exe, "decode", str(S)] + a, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for a in args if a]
    for run in runs:
        stdout, stderr = run.communicate(timeout=900)
        assert run.returncode == 0 and stdout.strip().endswith("ok"), stdout[-3000:] + stderr[-3000:]
    out = []
    for k, (name, data) in enumerate(cases):
        raw = open(str(tmp_path / ("%d_%d.bin" % (S, k))), "rb").read()
        head = struct.unpack("8i", raw[:32])
        info = jm.parse(data)
        npx = info["cols"] * info["rows"] * 4
        at = 32
        bgra = np.frombuffer(raw, np.uint8, npx, at).reshape(info["rows"], info["cols"], 4); at += npx
        coef = np.frombuffer(raw, np.int16, head[5] // 2, at).reshape(-1, 64); at += head[5]
        planes = np.frombuffer(raw, np.uint8, head[6], at); at += head[6]
        states = np.frombuffer(raw, np.uint32, head[2] * 4, at).reshape(-1, 4)
        out.append(dict(parsed=head[0], event=head[1], nsub=head[2], rounds=head[3], launches=head[4], bgra=bgra, coef=coef, planes=planes, states=states))
    return out


def _compare(cases, got, S):
    wrong = []
    for (name, data), g in zip(cases, got):
        m = jm.decode(data)
        assert m["accept"], name
        ok = g["parsed"] == 1 and g["event"] == -1 and g["nsub"] == jm.n_subsequences(m["info"], S)
        ok = ok and np.array_equal(g["bgra"], jm.bgra(m["rgb"])) and np.array_equal(g["coef"], m["coef"])
        ok = ok and np.array_equal(g["planes"], np.concatenate([p.reshape(-1) for p in m["planes"]]))
        want = jm.entry_states(m, S)
        have = g["states"][:-1]
        ok = ok and np.array_equal(have[:, 0], want[:, 0]) and np.array_equal(have[:, 1] & 0xff, want[:, 1]) and np.array_equal(have[:, 1] >> 8, want[:, 2])
        if not ok:
            wrong.append(name)
    assert not wrong, "cases whose kernels' results are not the model's at S = %d: %s" % (S, wrong)


def test_every_case_at_the_products_subsequence_size(exe, tmp_path):
    cases = jc.all_valid_cases() + jc.model_only_cases()
    got = _decode_all(exe, tmp_path, jc.S_PRODUCT, cases)
    _compare(cases, got, jc.S_PRODUCT)
    by_name = {c[0]: g for c, g in zip(cases, got)}
    # the subsequence beyond a workgroup's lanes is reached by a second launch; a smooth file's lanes are not all true after one round
    assert by_name["more_than_lanes-S%d" % jc.S_PRODUCT]["launches"] >= 2
    assert by_name["word_split-S%d" % jc.S_PRODUCT]["rounds"] > 1
    assert by_name["no_block_completes-S%d-handmade" % jc.S_PRODUCT]["rounds"] > 1


def test_the_seam_cases_at_the_smallest_subsequence_size(exe, tmp_path):
    cases = [(n, d) for n, _, d in jc.seam_cases()]
    got = _decode_all(exe, tmp_path, jc.S_MIN, cases)
    _compare(cases, got, jc.S_MIN)
    by_name = {c[0]: g for c, g in zip(cases, got)}
    assert by_name["more_than_lanes-S%d" % jc.S_MIN]["launches"] >= 2
    for what in ("no_block_completes", "word_split", "ff_split", "block_ends_on_boundary"):
        assert by_name["%s-S%d" % (what, jc.S_MIN)]["rounds"] > 1, what


def _variants_agree(exe, tmp_path, S, files, tag, processes=8):
    runs = []
    for p in range(processes):      # the files dealt out to runs side by side: p, p + processes, ...
        pack = str(tmp_path / ("%s_%d.pack" % (tag, p)))
        part = files[p::processes]
        with open(pack, "wb") as f:
            f.write(struct.pack("<I", len(part)))
            for d in part:
                f.write(struct.pack("<I", len(d))); f.write(d)
        runs.append(subprocess.Popen([exe, "variants", str(S), pack, str(tmp_path / ("%s_%d.txt" % (tag, p)))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    lines = [None] * len(files)
    for p, run in enumerate(runs):
        stdout, stderr = run.communicate(timeout=900)
        assert run.returncode == 0 and stdout.strip().endswith("ok"), stdout[-3000:] + stderr[-3000:]
        lines[p::processes] = open(str(tmp_path / ("%s_%d.txt" % (tag, p)))).read().split("\n")[:-1]
    assert len(lines) == len(files)
    wrong = []; kinds = {"P": 0, "R": 0, "A": 0}
    for k, (d, line) in enumerate(zip(files, lines)):
        try:
            m = jm.decode(d)
        except jm.Refused:
            want = "P"
        else:
            if m["accept"]:
                h = 1469598103934665603
                for b in jm.bgra(m["rgb"]).tobytes():
                    h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
                want = "A %d" % h
            else:
                want = "R %d" % m["event_mcu"]
        kinds[want[0]] += 1
        if line != want:
            wrong.append((k, line, want))
    assert not wrong, "%d of %d variants differ from the model (index, kernels, model): %s" % (len(wrong), len(files), wrong[:10])
    return kinds


def _small_scan():
    data = jc.pil_jpeg(jc.scene(24, 16, jc.SEED + 5), 60, "420", False, 1)
    info = jm.parse(data)
    assert 100 <= info["end"] - info["begin"] <= 160
    return data, info


def test_every_bit_flip_and_truncation_of_a_small_scan(exe, tmp_path):
    S = jc.S_MIN        # several lanes over the scan, so that a flip also moves what the lanes after it synchronise on
    data, info = _small_scan()
    b, e = info["begin"], info["end"]
    files = []
    for k in range(b, e):
        for bit in range(8):
            v = bytearray(data); v[k] ^= 1 << bit; files.append(bytes(v))
    for k in range(b, e):
        files.append(data[:k] + data[e:])
    kinds = _variants_agree(exe, tmp_path, S, files, "flips%d" % S)
    assert kinds["R"] > 100 and kinds["A"] > 100 and kinds["P"] > 0     # the three outcomes all occur


def test_scans_of_random_bytes(exe, tmp_path):
    data, info = _small_scan()
    rng = np.random.default_rng(jc.SEED)
    files = []
    for k in range(200):
        n = int(rng.integers(1, 600))
        seg = bytes(rng.integers(0, 256, n, dtype=np.uint8)).replace(b"\xff", b"\xff\x00" if k % 2 else b"\xfe")
        files.append(data[:info["begin"]] + seg + data[info["end"]:])
    _variants_agree(exe, tmp_path, jc.S_MIN, files, "random")
