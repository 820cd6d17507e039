"""CPU tier: the device inflate kernel (csrc/kernels_tiff.hip k_tiff_inflate) compiled as host code over the stand-in for the HIP
runtime header (tests/cpp/hip_host_shim) and run thread for thread by tests/cpp/tiff_inflate_host.cpp under the address and
undefined-behaviour sanitizers, every buffer at its exact size.  The judge is libz's own uncompress (tests/inflate_model.py): every
well-formed case of tests/inflate_cases.py gives its image and a clean status; every malformed strip gets the judge's verdict and reason
class; every single-bit flip and every truncation of a small stream gets the judge's verdict, and the judge's bytes where accepted.
The bytes a refused strip leaves behind are not compared: zlib's partial output is no contract and the library zero-fills."""
import os
import subprocess

import numpy as np
import pytest

import inflate_cases as ic
import inflate_model as im
import tiff_model as tm
from conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tiff_inflate_host") / "tiff_inflate_host")
    src = os.path.join(ROOT, "tests", "cpp", "tiff_inflate_host.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-x", "c++", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "tests", "cpp", "hip_host_shim"), "-pthread", "-o", path, src], check=True)
    return path


def run(exe, tmp_path, files):
    """{name: file bytes} -> {name: (BGRA image, [(decoded, expected, reason)])}"""
    args, names = [], sorted(files)
    for k, name in enumerate(names):
        p = str(tmp_path / ("%d" % k))
        with open(p + ".tif", "wb") as f:
            f.write(files[name])
        args += [p + ".tif", p + ".bgra", p + ".status"]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-3000:] + out.stderr[-3000:]
    res = {}
    for k, name in enumerate(names):
        f = tm.parse(files[name])
        img = np.fromfile(str(tmp_path / ("%d.bgra" % k)), np.uint8).reshape(f[257][0], f[256][0], 4)
        status = [tuple(int(v) for v in line.split()) for line in open(str(tmp_path / ("%d.status" % k)))]
        res[name] = (img, status)
    return res


def accepted(status):
    return [a == b and r == 0 for a, b, r in status]


def test_every_case_decodes_to_its_image(exe, tmp_path, synth):
    cases = ic.cases(synth)
    res = run(exe, tmp_path, {k: c.file for k, c in cases.items()})
    wrong = [k for k, c in cases.items() if not np.array_equal(res[k][0], tm.expected_bgra(c.img)) or not all(accepted(res[k][1]))]
    assert not wrong, wrong


def test_malformed_strips_get_the_judges_verdict_and_reason(exe, tmp_path):
    bad = ic.malformed()
    res = run(exe, tmp_path, {k: b.file for k, b in bad.items()})
    for name, b in sorted(bad.items()):
        _, verdicts = im.decode(b.file)
        status = res[name][1]
        assert accepted(status) == [ok for ok, _ in verdicts] and not accepted(status)[b.strip], (name, status)
        assert status[b.strip][2] == verdicts[b.strip][1] == b.reason, (name, status)
        if b.reason == im.REASON_OK:
            assert status[b.strip][0] < status[b.strip][1], (name, status)   # short, and says how short


def _held_to_the_judge(data, img, status):
    want_img, verdicts = im.decode(data)
    got = accepted(status)
    assert got == [ok for ok, _ in verdicts], [s for s, (a, (b, _)) in enumerate(zip(got, verdicts)) if a != b][:20]
    rows = np.array(got)   # one row per strip
    assert np.array_equal(img[rows], want_img[rows])
    return got


def test_every_single_bit_flip_gets_the_judges_verdict(exe, tmp_path):
    raw, dyn, fix = ic.flip_streams()
    assert len(dyn) <= 160 and len(fix) <= 160 and dyn[2] & 6 == 4 and fix[2] & 6 == 2   # a dynamic and a fixed block
    files = {"dyn": ic.every_flip(dyn), "fix": ic.every_flip(fix)}
    res = run(exe, tmp_path, files)
    for name, stream in (("dyn", dyn), ("fix", fix)):
        got = _held_to_the_judge(files[name], *res[name])
        assert len(got) == 8 * len(stream) and 0 < sum(got) < len(got) // 4


def test_every_truncation_gets_the_judges_verdict(exe, tmp_path):
    raw, dyn, fix = ic.flip_streams()
    files = {"dyn": ic.every_truncation(dyn), "fix": ic.every_truncation(fix)}
    res = run(exe, tmp_path, files)
    for name, stream in (("dyn", dyn), ("fix", fix)):
        got = _held_to_the_judge(files[name], *res[name])
        assert got[-1] and not got[len(stream) // 2]   # a trailer cut by one byte is accepted; half a stream is not
        assert all(r == 0 for a, b, r in res[name][1] if a < b)   # a cut stream ends early: no reason


def test_every_clip_of_a_stream_is_accepted_as_the_judge_accepts_it(exe, tmp_path):
    """one stream in a strip of every size up to its payload's: the strip's end cuts a literal run, a match or nothing; zlib fills the
    strip and reads nothing behind a cut match, so the end-of-block and the trailer (the whole payload's) are never met"""
    toks = ic.clip_tokens()
    payload = im.expand(toks)
    files = {}
    for form, stream in (("fix", im.fixed_stream(toks)), ("dyn", im.dynamic_stream(toks)[0])):
        for n, data in ic.every_clip(stream, payload).items():
            files["%s_%03d" % (form, n)] = data
    # ... and with one or two random bit flips, at every size: whatever the verdict, it is the judge's
    rnd = np.random.RandomState(7)
    for form, stream in (("fix", im.fixed_stream(toks)), ("dyn", im.dynamic_stream(toks)[0])):
        for n in range(3, len(payload) + 1, 3):
            for k in range(4):
                b = bytearray(stream)
                for bit in rnd.randint(16, 8 * len(stream), 1 + k % 2):
                    b[bit >> 3] ^= 1 << (bit & 7)
                files["%s_%03d_flip%d" % (form, n, k)] = im.write_tiff(np.zeros((1, n // 3, 3), np.uint8), None, streams={0: bytes(b)})
    res = run(exe, tmp_path, files)
    for name, data in files.items():
        got = _held_to_the_judge(data, *res[name])
        if "flip" not in name:
            assert got == [True] and res[name][0].reshape(-1, 4)[:, 2::-1].tobytes() == payload[:int(name[4:])], name


def test_random_strips_terminate(exe, tmp_path):
    data = ic.random_strips(200)
    img, status = run(exe, tmp_path, {"random": data})["random"]
    assert len(status) == 200
    _held_to_the_judge(data, img, status)
