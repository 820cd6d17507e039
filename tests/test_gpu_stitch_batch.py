"""Batched stitch step (pf_stitch_step_batch / pf_stitch_step_batch_dev): frame k of a batch gives exactly the bytes that
pf_stitch_step gives for frame k's own sequence of calls, whatever the grouping into launches and lanes."""
import ctypes as C
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest
from PIL import Image

from conftest import PKG

PCT = 20   # pixflow_search_20
EXE = os.path.join(PKG, "tools", "pano_stitch")


def _rig(synth, cols, rows, seed):
    top, imgs = synth.make_stitch_set(cols, rows, seed, 5, "cuda")
    return top.cpu().numpy(), [im.cpu().numpy() for im in imgs]


def _chain(c, top, imgs):
    outs = []
    for i, L in enumerate(imgs):
        outs.append(c.stitch_step(L, top if i == 0 else None, PCT))
    return outs


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _ndiff(a, b):
    return int((a != b).sum())


@pytest.fixture(scope="module")
def rigs1200(synth, pf):
    return [_rig(synth, 1200, 600, 1234 + k) for k in range(3)]


@pytest.fixture(scope="module")
def rigs800(synth, pf):
    return [_rig(synth, 800, 400, 1234 + k) for k in range(4)]


@pytest.fixture(scope="module")
def chains1200(pf, rigs1200):
    c = pf.Context(0)
    ref = [_chain(c, top, imgs) for top, imgs in rigs1200]
    c.close()
    return ref


@pytest.fixture(scope="module")
def frames800(pf, rigs800):
    """19 independent single steps at 800x400 (tile smoothing: step 2, k 3) and their pf_stitch_step results"""
    Ls, Rs = [], []
    for k in range(19):
        top, imgs = rigs800[k % 4]
        Ls.append(imgs[k % 5]); Rs.append(top)
    c = pf.Context(0)
    ref = [c.stitch_step(L, R, PCT) for L, R in zip(Ls, Rs)]
    c.close()
    return Ls, Rs, ref


@pytest.mark.gpu
def test_batch_chains_equal_single_chains(pf, rigs1200, chains1200):
    c = pf.Context(0)
    for i in range(5):
        Ls = [imgs[i] for _, imgs in rigs1200]
        outs = c.stitch_step_batch(Ls, [top for top, _ in rigs1200] if i == 0 else None, PCT, in_flight=3)
        for k, out in enumerate(outs):
            ref = chains1200[k][i]
            assert np.array_equal(out, ref), "frame %d step %d: %d bytes differ from its stitch_step chain" % (k, i + 1, _ndiff(out, ref))
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cols,rows", [(640, 320), (400, 820)], ids=["640x320", "400x820"])
def test_batch_step_equals_oracle_chain(pf, orc, synth, cols, rows):
    """640x320 has no box blur (k2 = rows/400 = 0).  400x820 is the smallest canvas at which all three ramp stages run
    non-trivially for a frame with blockIdx.z > 0: step 2, k1 6 (resident tile pass), k2 2."""
    rigs = [synth.make_stitch_set(cols, rows, s, 1) for s in (1234, 1235)]
    rigs = [(t.numpy(), [im.numpy() for im in ims]) for t, ims in rigs]
    c = pf.Context(0)
    outs = c.stitch_step_batch([ims[0] for _, ims in rigs], [t for t, _ in rigs], PCT, in_flight=2)
    lone = [c.stitch_step(ims[0], t, PCT) for t, ims in rigs]
    c.close()
    step, k2 = min(cols, rows) // 200, rows // 400
    for k, (top, ims) in enumerate(rigs):
        L, R = ims[0], top
        mp, ovl, ovr, blend, md = orc.stitch_prepare(L, R, True)
        if (cols, rows) == (400, 820):   # the geometry is what this case is for
            active = int((md[0:rows - step:step, 0:cols - step:step] > step).sum())
            assert k2 >= 2 and active >= 1000, "frame %d: k2 %d, %d active tiles" % (k, k2, active)
        f0, f1 = orc.flow_bidir(ovl, ovr, PCT)
        merged = orc.combine_novel_views(ovl, ovr, f0, f1, blend)
        ref = orc.stitch_gather(L, R, merged, mp)
        assert np.array_equal(outs[k], ref), "frame %d: %d bytes differ from the oracle chain" % (k, _ndiff(outs[k], ref))
        assert np.array_equal(lone[k], ref), "frame %d: stitch_step differs from the oracle chain in %d bytes" % (k, _ndiff(lone[k], ref))


@pytest.mark.gpu
@pytest.mark.parametrize("in_flight", [1, 4, 16, 19])
def test_groups_and_lanes(pf, frames800, in_flight):
    Ls, Rs, ref = frames800
    c = pf.Context(0)
    outs = c.stitch_step_batch(Ls, Rs, PCT, in_flight=in_flight)
    for k in range(len(Ls)):
        assert np.array_equal(outs[k], ref[k]), "in_flight %d frame %d: %d bytes differ" % (in_flight, k, _ndiff(outs[k], ref[k]))
    c.close()


@pytest.mark.gpu
def test_tile_wavefront_across_frames(pf, rigs800):
    """frames whose overlaps (and so active smoothing tiles) lie in different columns, and one with no overlap at all (the two
    images cover disjoint column windows), in one tile-smoothing launch"""
    top, imgs = rigs800[0]
    top2, imgs2 = rigs800[1]
    pairs = [(imgs[0], top), (imgs[2], top2), (imgs2[4], top), (imgs[0], imgs[2]), (imgs[3], imgs2[2])]
    c = pf.Context(0)
    ref = [c.stitch_step(L, R, PCT) for L, R in pairs]
    mp = c.stitch_match(imgs[0], imgs[2])[0]
    assert not (mp == 150).any(), "the no-overlap frame has an overlap"
    outs = c.stitch_step_batch([p[0] for p in pairs], [p[1] for p in pairs], PCT, in_flight=len(pairs))
    for k in range(len(pairs)):
        assert np.array_equal(outs[k], ref[k]), "frame %d: %d bytes differ" % (k, _ndiff(outs[k], ref[k]))
    c.close()


@pytest.mark.gpu
def test_full_size_batch(pf, synth):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_9000x4000.npz")
    g = np.load(path)
    cols, rows, seed = int(g["cols"]), int(g["rows"]), int(g["seed"])
    assert int(g["max_pct"]) == PCT
    rigs = [_rig(synth, cols, rows, seed + k) for k in range(3)]
    assert [_sha(rigs[0][0])] + [_sha(im) for im in rigs[0][1]] == list(g["sha_inputs"]), "GPU-generated canvases differ from the fixture's"
    c = pf.Context(0)
    seq = [[_sha(o) for o in _chain(c, top, imgs)] for top, imgs in rigs[1:]]
    for i in range(5):
        outs = c.stitch_step_batch([imgs[i] for _, imgs in rigs], [top for top, _ in rigs] if i == 0 else None, PCT, in_flight=3)
        assert _sha(outs[0]) == str(g["sha_final"][i]), "frame 0 step %d differs from the oracle chain" % (i + 1)
        for k in (1, 2):
            assert _sha(outs[k]) == seq[k - 1][i], "frame %d step %d differs from its sequential chain" % (k, i + 1)
        del outs
    c.close()


@pytest.mark.gpu
def test_device_form_ping_pong(pf, rigs1200, chains1200):
    cols, rows = 1200, 600
    nb = cols * rows * 4
    c = pf.Context(0)
    bufs = []
    try:
        alloc = lambda: bufs.append(c.dev_alloc(nb)) or bufs[-1]
        dtop = [alloc() for _ in rigs1200]
        dL = [alloc() for _ in rigs1200]
        ping = [alloc() for _ in rigs1200]
        pong = [alloc() for _ in rigs1200]
        for k, (top, _) in enumerate(rigs1200):
            c.upload(dtop[k], top)
        dR = dtop
        for i in range(3):
            for k, (_, imgs) in enumerate(rigs1200):
                c.upload(dL[k], imgs[i])
            dout = ping if i % 2 == 0 else pong
            c.stitch_step_batch_dev(dL, dR, cols, rows, PCT, dout, in_flight=2)
            for k in range(len(rigs1200)):
                got = c.download(np.empty((rows, cols, 4), np.uint8), dout[k])
                assert np.array_equal(got, chains1200[k][i]), "frame %d step %d: %d bytes differ" % (k, i + 1, _ndiff(got, chains1200[k][i]))
            dR = dout
        # aliasing: an output on an input of the call, or on another output
        for douts in ([dL[0], pong[1], pong[2]], [pong[0], pong[0], pong[2]], [pong[0], dR[0], pong[2]]):
            with pytest.raises(pf.PanoflowError, match="overlaps"):
                c.stitch_step_batch_dev(dL, dR, cols, rows, PCT, douts, in_flight=2)
        # repeated inputs are fine
        c.stitch_step_batch_dev([dL[0], dL[0]], [dR[0], dR[0]], cols, rows, PCT, [pong[0], pong[1]], in_flight=2)
        a = c.download(np.empty((rows, cols, 4), np.uint8), pong[0]); b = c.download(np.empty((rows, cols, 4), np.uint8), pong[1])
        assert np.array_equal(a, b)
    finally:
        for p in bufs:
            c.dev_free(p)
        c.close()


@pytest.mark.gpu
def test_errors_and_isolation(pf, rigs800, frames800):
    top, imgs = rigs800[0]
    rows, cols = top.shape[:2]
    c = pf.Context(0)
    assert c.stitch_step_batch([], None, PCT) == []
    P = C.c_void_p * 1
    arr = P(imgs[0].ctypes.data)
    assert c.l.pf_stitch_step_batch(c.h, -1, arr, None, cols, rows, C.c_size_t(cols * 4), PCT, None, C.c_size_t(cols * 4), 1) == -1
    assert c.l.pf_stitch_step_batch(c.h, 1, None, None, cols, rows, C.c_size_t(cols * 4), PCT, None, C.c_size_t(cols * 4), 1) == -1
    assert c.l.pf_stitch_step_batch(c.h, 1, P(None), arr, cols, rows, C.c_size_t(cols * 4), PCT, None, C.c_size_t(cols * 4), 1) == -1
    assert c.l.pf_stitch_step_batch_dev(c.h, 1, None, None, cols, rows, PCT, None, 1) == -1
    assert c.l.pf_stitch_step_batch_dev(c.h, 0, arr, arr, cols, rows, PCT, arr, 1) == 0
    with pytest.raises(pf.PanoflowError, match="chain"):   # nothing to chain on yet
        c.stitch_step_batch([imgs[0]], None, PCT)
    with pytest.raises(pf.PanoflowError, match="max_percentage"):
        c.stitch_step_batch([imgs[0]], [top], 101)
    c.stitch_step_batch([imgs[0], imgs[1]], [top, top], PCT, want_out=False)
    with pytest.raises(pf.PanoflowError, match="chain"):   # frame 2 has no previous composite
        c.stitch_step_batch([imgs[1], imgs[2], imgs[3]], None, PCT)
    with pytest.raises(pf.PanoflowError, match="chain"):   # another size
        c.stitch_step_batch([imgs[0][:, :640].copy()], None, PCT)
    # the slots survived the refusals: frame 1 (a None entry) chains on its composite, frame 0 starts anew
    a = c.stitch_step_batch([imgs[1], imgs[2]], [top, None], PCT)
    s = pf.Context(0)
    ref = _chain(s, top, [imgs[1], imgs[2]])
    assert np.array_equal(a[0], ref[0]) and np.array_equal(a[1], ref[1])
    # a size change refuses chaining
    small = [im[:320, :640].copy() for im in (imgs[0], top)]
    c.stitch_step_batch([small[0]], [small[1]], PCT)
    with pytest.raises(pf.PanoflowError, match="chain"):
        c.stitch_step_batch([imgs[0]], None, PCT)
    # a pf_stitch_step chain (with a prefetch) interleaved with batch calls gives its uninterrupted bytes
    ref = _chain(s, top, imgs)
    Ls, Rs, _ = frames800
    out = []
    for i, L in enumerate(imgs):
        if i + 1 < len(imgs):
            c.stitch_prefetch(imgs[i + 1])
        out.append(c.stitch_step(L, top if i == 0 else None, PCT))
        c.stitch_step_batch(Ls[:3], Rs[:3] if i == 0 else None, PCT, in_flight=2, want_out=False)
        with pytest.raises(pf.PanoflowError):
            c.stitch_visualize()
    for i in range(len(imgs)):
        assert np.array_equal(out[i], ref[i]), "interleaved chain step %d: %d bytes differ" % (i + 1, _ndiff(out[i], ref[i]))
    s.close(); c.close()


def _bgra_to_rgba(a):
    return a[..., [2, 1, 0, 3]]


@pytest.mark.gpu
def test_cli_test_dirs(tmp_path, synth, pf):
    cols, rows, n = 480, 320, 3
    dirs = []
    for k, seed in enumerate((77, 78)):
        top, imgs = synth.make_stitch_set(cols, rows, seed, n)
        d = tmp_path / ("single%d" % k); d.mkdir()
        Image.fromarray(_bgra_to_rgba(top.numpy()), "RGBA").save(d / "top.tif")
        for i, im in enumerate(imgs):
            Image.fromarray(_bgra_to_rgba(im.numpy()), "RGBA").save(d / ("%d.tif" % (i + 1)))
        b = tmp_path / ("batch%d" % k)
        shutil.copytree(d, b)
        dirs.append((d, b))
    for d, _ in dirs:
        r = subprocess.run([EXE, "-test_dir", str(d), "-top_img", "top.tif", "-flow_alg", "pixflow_search_20", "-steps", str(n)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    r = subprocess.run([EXE, "-test_dirs", ",".join(str(b) for _, b in dirs), "-in_flight", "2", "-top_img", "top.tif", "-flow_alg",
                        "pixflow_search_20", "-steps", str(n)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for i in range(1, n + 1):
        assert "Part%d Finished!RUNTIME (sec) = " % i in r.stdout
    assert "TotalRunTime (sec) = " in r.stdout
    names = ["ProcessResult%d.png" % i for i in range(1, n)] + ["FinalResult.png"]
    for d, b in dirs:
        for name in names:
            assert (d / name).read_bytes() == (b / name).read_bytes(), "%s/%s differs from the -test_dir run's" % (b.name, name)
