"""pano_stitch -lens_rig FILE -canvas WxH: the run's inputs are raw photos, remapped on the GPU onto the canvas before anything else
sees them.  A small sphere is photographed by a rig of five cameras and a top camera (tests/reproject_model.py's rectilinear views),
the photos are written as TIFFs beside a .pto that describes the rig, and the run must write the files, byte for byte, that a run
without the flag writes over the canvases the model makes of the same photos (tests/lens_model.py) -- once in a mode that holds its
images on the host and once in -rig_chain 1 -tiff_device 1, where the photos are decoded and remapped in device memory."""
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import lens_model as M
import reproject_model as R
from conftest import PKG

EXE = os.path.join(PKG, "tools", "pano_stitch")
STEMS = ("ProcessResult1", "ProcessResult2", "ProcessResult3", "ProcessResult4", "FinalResult")
COMMON = ["-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", "5"]
CANVAS = (256, 128)

# (file, w, h, hfov, yaw, pitch, roll, a, b, c, d, e): five upright cameras 72 degrees apart and one looking up; the second camera has
# a roll, a polynomial and a shifted centre, so that every letter of the description reaches the pixels
RIG = [("top.tif", 128, 128, 130.0, 0.0, 90.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)]
RIG += [("%d.tif" % i, 96, 128, 90.0, (i - 0.5) * 72.0 - 180.0, 0.0, 3.0 if i == 2 else 0.0) + ((0.01, -0.02, 0.005, 1.5, -2.25) if i == 2 else (0.0,) * 5)
        for i in range(1, 6)]


def _pto():
    lines = ["# a rig of five cameras and a top camera", "p f2 w%d h%d v360 n\"TIFF_m\"" % CANVAS, ""]
    for k, (name, w, h, v, y, p, r, a, b, c, d, e) in enumerate(RIG):
        size = "w%d h%d f0 v%r" % (w, h, v) if k < 2 else "w=1 h=1 f=1 v=1"   # the cameras after the first upright one refer back to it
        lines.append("i %s Ra0 Rb0 Eev0 Er1 Eb1 r%r p%r y%r TrX0 j0 a%r b%r c%r d%r e%r g0 t0 Va1 Vb0 Vx0 n\"%s\"" % (size, r, p, y, a, b, c, d, e, name))
    return "\n".join(lines) + "\n"


def _lens(entry):
    name, w, h, v, y, p, r, a, b, c, d, e = entry
    return M.Lens(M.RECTILINEAR, M.focal(M.RECTILINEAR, w, v), filter=M.BICUBIC, a=a, b=b, c=c, dd=1.0 - (a + b + c), shift_x=d, shift_y=e, rot=M.rotation(y, p, r))


def _sphere(seed):
    """an opaque 512 x 256 texture: smooth blobs and some grain for the flow to hold on to"""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(40, 216, (16, 32, 3)).astype(np.float64)
    img = np.kron(coarse, np.ones((16, 16, 1)))
    for axis in (0, 1):   # soften the blocks' edges
        img = (np.roll(img, 3, axis) + np.roll(img, -3, axis) + 2.0 * img) / 4.0
    img += rng.integers(-12, 13, img.shape)
    out = np.empty((256, 512, 4), np.uint8)
    out[..., :3] = np.clip(np.rint(img), 0, 255)
    out[..., 3] = 255
    return out


def _save(path, bgra):
    Image.fromarray(np.ascontiguousarray(bgra[..., [2, 1, 0, 3]]), "RGBA").save(path)


def _write_rig(raw_dir, canvas_dir, seed):
    """the rig's photos of a sphere into raw_dir with the .pto, and the model's canvases of them into canvas_dir"""
    sphere = _sphere(seed)
    os.makedirs(raw_dir); os.makedirs(canvas_dir)
    with open(os.path.join(raw_dir, "rig.pto"), "w") as f:
        f.write(_pto())
    for entry in RIG:
        name, w, h, v, y, p, r = entry[:7]
        photo = R.reproject(sphere, w, h, R.RECTILINEAR, filter=R.BICUBIC, hfov_deg=v, rot=R.rotation(y, p, r))
        assert photo[..., 3].min() == 255
        _save(os.path.join(raw_dir, name), photo)
        canvas = M.remap(photo, CANVAS[0], CANVAS[1], _lens(entry))
        assert 0.02 < (canvas[..., 3] > 0).mean() < 0.5
        _save(os.path.join(canvas_dir, name), canvas)


def _run(args, ok=True):
    out = subprocess.run([EXE] + args, capture_output=True, text=True)
    if ok:
        assert out.returncode == 0, out.stderr
        assert "TotalRunTime (sec) = " in out.stdout
    return out


def _same_files(a, b):
    for stem in STEMS:
        got, want = (open(os.path.join(d, stem + ".png"), "rb").read() for d in (a, b))
        assert got == want, stem
    final = np.array(Image.open(os.path.join(a, "FinalResult.png")))
    assert (final[..., 3] > 0).mean() > 0.5   # the rig covers most of the sphere: the chain stitched something


@pytest.mark.gpu
def test_lone_chain_remaps_inside_the_image_read(tmp_path):
    raw, ref = str(tmp_path / "raw"), str(tmp_path / "ref")
    _write_rig(raw, ref, 11)
    _run(["-test_dir", ref] + COMMON)
    _run(["-test_dir", raw] + COMMON + ["-lens_rig", os.path.join(raw, "rig.pto"), "-canvas", "%dx%d" % CANVAS])
    _same_files(raw, ref)


@pytest.mark.gpu
def test_rig_chain_on_the_device_remaps_the_decoded_buffers(tmp_path):
    mode = ["-static_rig", "1", "-rig_chain", "1", "-tiff_device", "1", "-png_device", "1"]
    raws = [str(tmp_path / ("raw%d" % k)) for k in range(2)]
    refs = [str(tmp_path / ("ref%d" % k)) for k in range(2)]
    for k in range(2):
        _write_rig(raws[k], refs[k], 500 + k)
    _run(["-test_dirs", ",".join(refs)] + COMMON + mode)
    _run(["-test_dirs", ",".join(raws)] + COMMON + mode + ["-lens_rig", os.path.join(raws[0], "rig.pto"), "-canvas", "%dx%d" % CANVAS])
    for k in range(2):
        _same_files(raws[k], refs[k])
    assert open(os.path.join(raws[0], "FinalResult.png"), "rb").read() != open(os.path.join(raws[1], "FinalResult.png"), "rb").read()


def test_refusals_end_the_run_before_any_output(tmp_path):
    # (no device is touched: every refusal comes before the first library call that needs one)
    d = str(tmp_path / "run")
    os.makedirs(d)
    rig = str(tmp_path / "rig.pto"); bad = str(tmp_path / "bad.pto"); none = str(tmp_path / "none.pto")
    open(rig, "w").write(_pto())
    open(bad, "w").write("# a comment\n" + _pto().replace("f0", "f7"))
    open(none, "w").write("p f2 w256 h128 v360\n")
    Image.fromarray(np.zeros((8, 8, 4), np.uint8), "RGBA").save(os.path.join(d, "top.tif"))
    before = sorted(os.listdir(d))
    for flags, word in ((["-lens_rig", rig], "-lens_rig FILE and -canvas WxH go together"),
                        (["-canvas", "256x128"], "-lens_rig FILE and -canvas WxH go together"),
                        (["-lens_rig", rig, "-canvas", "256"], "-canvas must be WxH"),
                        (["-lens_rig", rig, "-canvas", "0x128"], "-canvas must be WxH"),
                        (["-lens_rig", rig, "-canvas", "256x128x3"], "-canvas must be WxH"),
                        (["-lens_rig", rig, "-canvas", "70000x128"], "-canvas must be WxH"),
                        (["-lens_rig", str(tmp_path / "missing.pto"), "-canvas", "256x128"], "cannot read"),
                        (["-lens_rig", bad, "-canvas", "256x128"], "bad.pto: line 5: unknown f"),
                        (["-lens_rig", none, "-canvas", "256x128"], "describes no image"),
                        # the top image is there, but it is 8 x 8 and its description says 128 x 128
                        (["-lens_rig", rig, "-canvas", "256x128"], "top.tif is 8x8, not the 128x128 of its description"),
                        (["-lens_rig", rig, "-canvas", "256x128", "-top_img", "roof.tif"], "failed to load")):
        out = _run(["-test_dir", d] + COMMON + flags, ok=False)
        assert out.returncode != 0 and "VrCamException" in out.stderr and word in out.stderr, (flags, out.stderr)
        assert sorted(os.listdir(d)) == before
    os.rename(os.path.join(d, "top.tif"), os.path.join(d, "roof.tif"))
    out = _run(["-test_dir", d, "-top_img", "roof.tif"] + COMMON[2:] + ["-lens_rig", rig, "-canvas", "256x128"], ok=False)
    assert out.returncode != 0 and "describes no image named roof.tif" in out.stderr, out.stderr
