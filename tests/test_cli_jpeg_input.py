"""pano_stitch -input_ext jpg: the rig test of tests/test_cli_lens.py with the photos saved as quality-95 JPEGs, which the run decodes on
the GPU (pf_jpeg_decode*) before the lens remap.  A run over the JPEGs must write, byte for byte, the files of a run over TIFFs that hold
Pillow's decode of the same JPEGs -- in the lone chain, whose image read calls pf_jpeg_decode, and in -rig_chain 1 -tiff_device 1, where
a directory's photos are decoded by pf_jpeg_decode_batch_dev into the buffers the remap reads.  Without -lens_rig the flag is refused."""
import os

import numpy as np
import pytest
from PIL import Image

import reproject_model as R
import test_cli_lens as L

COMMON_JPG = ["-top_img", "top.jpg", "-flow_alg", "pixflow_search_20", "-steps", "5", "-input_ext", "jpg"]
SUBSAMPLING = {"top.tif": 2, "1.tif": 0, "2.tif": 1, "3.tif": 2, "4.tif": 2, "5.tif": 0}     # 4:2:0, 4:4:4 and 4:2:2 among the cameras


def _write_rig(jpg_dir, tif_dir, seed):
    """the rig's photos of a sphere as JPEGs into jpg_dir, Pillow's decode of each as a TIFF into tif_dir, a .pto beside each"""
    sphere = L._sphere(seed)
    os.makedirs(jpg_dir); os.makedirs(tif_dir)
    with open(os.path.join(tif_dir, "rig.pto"), "w") as f:
        f.write(L._pto())
    with open(os.path.join(jpg_dir, "rig.pto"), "w") as f:
        f.write(L._pto().replace(".tif\"", ".jpg\""))
    for entry in L.RIG:
        name, w, h, v, y, p, r = entry[:7]
        photo = R.reproject(sphere, w, h, R.RECTILINEAR, filter=R.BICUBIC, hfov_deg=v, rot=R.rotation(y, p, r))
        jpg = os.path.join(jpg_dir, name.replace(".tif", ".jpg"))
        kw = dict(restart_marker_blocks=3) if name == "3.tif" else {}
        Image.fromarray(np.ascontiguousarray(photo[..., [2, 1, 0]])).save(jpg, "JPEG", quality=95, subsampling=SUBSAMPLING[name], optimize=name == "4.tif", **kw)
        decoded = np.asarray(Image.open(jpg).convert("RGB"))
        Image.fromarray(np.dstack([decoded, np.full(decoded.shape[:2], 255, np.uint8)]), "RGBA").save(os.path.join(tif_dir, name))


@pytest.mark.gpu
def test_lone_chain_decodes_inside_the_image_read(tmp_path):
    jpg, tif = str(tmp_path / "jpg"), str(tmp_path / "tif")
    _write_rig(jpg, tif, 11)
    canvas = ["-canvas", "%dx%d" % L.CANVAS]
    L._run(["-test_dir", tif] + L.COMMON + ["-lens_rig", os.path.join(tif, "rig.pto")] + canvas)
    L._run(["-test_dir", jpg] + COMMON_JPG + ["-lens_rig", os.path.join(jpg, "rig.pto")] + canvas)
    L._same_files(jpg, tif)


@pytest.mark.gpu
def test_rig_chain_on_the_device_decodes_into_the_remaps_buffers(tmp_path):
    mode = ["-static_rig", "1", "-rig_chain", "1", "-tiff_device", "1", "-png_device", "1"]
    jpgs = [str(tmp_path / ("jpg%d" % k)) for k in range(2)]
    tifs = [str(tmp_path / ("tif%d" % k)) for k in range(2)]
    for k in range(2):
        _write_rig(jpgs[k], tifs[k], 500 + k)
    canvas = ["-canvas", "%dx%d" % L.CANVAS]
    L._run(["-test_dirs", ",".join(tifs)] + L.COMMON + mode + ["-lens_rig", os.path.join(tifs[0], "rig.pto")] + canvas)
    L._run(["-test_dirs", ",".join(jpgs)] + COMMON_JPG + mode + ["-lens_rig", os.path.join(jpgs[0], "rig.pto")] + canvas)
    for k in range(2):
        L._same_files(jpgs[k], tifs[k])
    assert open(os.path.join(jpgs[0], "FinalResult.png"), "rb").read() != open(os.path.join(jpgs[1], "FinalResult.png"), "rb").read()


def test_the_flag_is_refused_without_a_lens_rig_before_any_output(tmp_path):
    # (no device is touched: the refusals come before the first library call that needs one)
    d = str(tmp_path / "run")
    os.makedirs(d)
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(os.path.join(d, "top.jpg"), "JPEG")
    Image.fromarray(np.zeros((8, 8, 4), np.uint8), "RGBA").save(os.path.join(d, "top.tif"))
    before = sorted(os.listdir(d))
    for flags, word in ((["-top_img", "top.jpg", "-input_ext", "jpg"], "-input_ext jpg needs -lens_rig FILE and -canvas WxH"),
                        (["-top_img", "top.tif", "-input_ext", "jpg"], "-input_ext jpg needs -lens_rig FILE and -canvas WxH"),
                        (["-top_img", "top.tif", "-input_ext", "png"], "-input_ext must be tif or jpg"),
                        (["-top_img", "top.jpg"], "a JPEG input needs -lens_rig FILE and -canvas WxH")):
        out = L._run(["-test_dir", d, "-flow_alg", "pixflow_search_20", "-steps", "5"] + flags, ok=False)
        assert out.returncode != 0 and "VrCamException" in out.stderr and word in out.stderr, (flags, out.stderr)
        assert sorted(os.listdir(d)) == before
