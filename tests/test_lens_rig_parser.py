"""CPU tier: pano_stitch's reader of lens descriptions (tools/lens_rig.hpp, a subset of Hugin's .pto) as the stand-alone program
tests/cpp/lens_rig_parse.cpp under the address and undefined-behaviour sanitizers: a good file with back-references, a crop, ignored
letters and ignored lines gives the values written, and every malformed `i` line is an error that names its line."""
import os
import subprocess

import pytest

from conftest import ROOT

GOOD = """# hugin project file
#hugin_ptoversion 2
p f2 w256 h128 v360  E0 R0 n"TIFF_m c:LZW r:CROP"
m g1 i0 f0 m2 p0.00784314

# image lines
#-hugin  cropFactor=1
i w6000 h4000 f3 v121.5 Ra0 Rb0 Rc0 Rd0 Re0 Eev0 Er1 Eb1 r0.5 p-1.25 y0 TrX0 TrY0 TrZ0 Tpy0 Tpp0 j0 a0.01 b-0.05 c0.02 d1.5 e-2.25 g0 t0 Va1 Vb0 Vc0 Vd0 Vx0 Vy0  Vm5 n"1.tif"
i w=0 h=0 f=0 v=0 Ra=0 Rb=0 Eev0.1 r-0.25 p2 y72 a=0 b=0 c=0 d=0 e=0 g0 t0 Va=0 n"shots/2.tif"
i w3000 h3000 f2 v185 y0 p90 r0 a0 b0 c0 d-3 e4.5 S100,2900,150,2850 n"top image.tif"\r
i w=2 h=2 f=2 v=2 y180 p=1 r=0 a=0 b==0 c=0 d=2 e=2 n"4.tif"
v Ra0 Rb0
k 1
i w800 h600 f0 v65 y0 p0 r0 a0 b0 c0 d0 e0 n"view.png"
i w800 h600 f100 v150 y0 p0 r0 a0 b0 c0 d0 e0 n"s.tif"
i w800 h600 f101 v1.5e2 y0 p0 r0 a0 b0 c0 d0 e0 C0,800,0,600 n"e.tif"
"""

I = 'i w100 h80 f0 v60 y0 p0 r0 a0 b0 c0 d0 e0 n"1.tif"'

# (name, text, the line the error names, a word of the message)
BAD = [
    ("unknown_f", "# c\n" + I.replace("f0", "f4") + "\n", 2, "unknown f"),
    ("unknown_f_large", I.replace("f0", "f1e300") + "\n", 1, "unknown f"),
    ("cylindrical", I + "\n" + I.replace("f0", "f1") + "\n", 2, "unknown f"),
    ("missing_letter", "\n\n" + I.replace(" e0", "") + "\n", 3, "no 'e'"),
    ("missing_v", I.replace(" v60", "") + "\n", 1, "no 'v'"),
    ("missing_name", I.replace(' n"1.tif"', "") + "\n", 1, "no n"),
    ("unterminated_name", I[:-1] + "\n", 1, "unterminated"),
    ("bad_number", I + "\n" + I.replace("p0", "p0.5.1") + "\n", 2, "bad number in 'p0.5.1'"),
    ("bad_number_tail", I.replace("v60", "v60deg") + "\n", 1, "bad number"),
    ("not_finite", I.replace("y0", "y1e999") + "\n", 1, "bad number"),
    ("nan", I.replace("a0", "a-nan") + "\n", 1, "bad number"),
    ("fractional_width", I.replace("w100", "w100.5") + "\n", 1, "whole number"),
    ("huge_width", I.replace("w100", "w70000") + "\n", 1, "1..65535"),
    ("wide_rectilinear", I.replace("v60", "v180") + "\n", 1, "field of view"),
    ("dangling_reference", I + "\n" + I.replace("v60", "v=1") + "\n", 2, "does not come earlier"),
    ("dangling_reference_first", I.replace("h80", "h=0") + "\n", 1, "does not come earlier"),
    ("negative_reference", I + "\n" + I.replace("v60", "v=-1") + "\n", 2, "does not come earlier"),
    ("reference_not_a_number", I + "\n" + I.replace("v60", "v=x") + "\n", 2, "bad number"),
    ("short_crop", I.replace("f0", "f2 S1,2,3") + "\n", 1, "crop"),
    ("long_crop", I.replace("f0", "f2 S1,2,3,4,5") + "\n", 1, "crop"),
    ("empty_crop", I.replace("f0", "f2 S10,10,0,5") + "\n", 1, "crop"),
]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lens_rig_parse") / "lens_rig_parse")
    src = os.path.join(ROOT, "tests", "cpp", "lens_rig_parse.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", path, src], check=True)
    return path


def _run(exe, tmp_path, text):
    path = str(tmp_path / "rig.pto")
    with open(path, "w", newline="") as f:
        f.write(text)
    return subprocess.run([exe, path], capture_output=True, text=True, timeout=60)


def test_a_good_file(exe, tmp_path):
    out = _run(exe, tmp_path, GOOD.replace("b==0", "b=0"))
    assert out.returncode == 0 and not out.stderr, out.stdout + out.stderr
    rows = [line.rsplit(" ", 13) if line.endswith("-") else line.rsplit(" ", 16) for line in out.stdout.splitlines()]
    assert [r[0] for r in rows] == ["1.tif", "shots/2.tif", "top image.tif", "4.tif", "view.png", "s.tif", "e.tif"]
    nums = lambda r: [int(x) for x in r[1:4]] + [float.fromhex(x) for x in r[4:13]]
    #                       w     h     f  v      y      p      r      a     b      c     d    e
    assert nums(rows[0]) == [6000, 4000, 3, 121.5, 0.0, -1.25, 0.5, 0.01, -0.05, 0.02, 1.5, -2.25] and rows[0][13:] == ["-"]
    assert nums(rows[1]) == [6000, 4000, 3, 121.5, 72.0, 2.0, -0.25, 0.01, -0.05, 0.02, 1.5, -2.25] and rows[1][13:] == ["-"]
    assert nums(rows[2]) == [3000, 3000, 2, 185.0, 0.0, 90.0, 0.0, 0.0, 0.0, 0.0, -3.0, 4.5] and rows[2][13:] == ["100", "2900", "150", "2850"]
    # back-references to image 2, to image 1 (p) and to image 0 (r, a, b, c)
    assert nums(rows[3]) == [3000, 3000, 2, 185.0, 180.0, 2.0, 0.5, 0.01, -0.05, 0.02, -3.0, 4.5] and rows[3][13:] == ["-"]
    assert nums(rows[4]) == [800, 600, 0, 65.0] + [0.0] * 8
    assert nums(rows[5])[:4] == [800, 600, 100, 150.0] and nums(rows[6])[:4] == [800, 600, 101, 150.0]
    assert rows[6][13:] == ["0", "800", "0", "600"]


def test_a_file_without_images_is_empty(exe, tmp_path):
    out = _run(exe, tmp_path, "# nothing\np f2 w100 h50 v360\nimage lines start with i and a blank\nix w1\n")
    assert out.returncode == 0 and out.stdout == "" and not out.stderr


@pytest.mark.parametrize("name,text,line,word", BAD, ids=[b[0] for b in BAD])
def test_a_malformed_line_is_an_error_with_its_number(exe, tmp_path, name, text, line, word):
    out = _run(exe, tmp_path, text)
    assert out.returncode == 1 and not out.stderr, out.stdout + out.stderr
    assert out.stdout.startswith("error: line %d: " % line) and word in out.stdout, out.stdout


def test_a_doubled_equals_sign_is_a_bad_number(exe, tmp_path):
    out = _run(exe, tmp_path, GOOD)
    assert out.returncode == 1 and out.stdout.startswith("error: line 11: bad number in 'b==0'"), out.stdout
