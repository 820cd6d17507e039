"""GPU tier: the streamed form of the blend ramp's tile smoothing (k_tile_blur<true>, csrc/kernels_misc.hip) -- canvases whose tile
window does not fit the LDS of a CU.  Every comparison is bit for bit: against the raster loop over the oracle's blur-on-a-ROI for
explicit tile geometries (tile_blur_ref.py, pinned by test_tile_blur_reference.py), against the oracle's own smoothing for a canvas
that derives such a geometry, and against an oracle fixture for a whole stitch step on it."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from tile_blur_ref import active_tiles, random_inputs, tile_pass_reference

pytestmark = pytest.mark.gpu

LDS = 160 * 1024


def _lds_resident(step, k):
    nr = step + k - 1
    return nr * step * 8 + nr * nr * 4


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def ctx(pf):
    c = pf.Context(0)
    yield c
    c.close()


# (cols, rows, step, k): two that fit (config 4's own geometry is 20 / 30), 203 KB, the 30000x15000 panorama's geometry (256 KB, odd
# k), a tall strip's (175 KB, even k), row sums alone beyond LDS (287 KB, three column strips), and a small odd window with
# one-pixel tiles' neighbours (step 3) where a chunk holds the whole window
GEOMETRIES = [(700, 520, 10, 30), (900, 400, 20, 30), (1200, 900, 40, 150), (640, 480, 75, 115), (500, 700, 5, 200), (1000, 800, 120, 180),
              (300, 260, 3, 17)]


@pytest.mark.parametrize("cols,rows,step,k", GEOMETRIES)
def test_explicit_geometry_vs_reference_loop(ctx, orc, cols, rows, step, k):
    blend, md = random_inputs(cols, rows, step, 1000 + step * 7 + k)
    ref, n_active = tile_pass_reference(orc, blend, md, step, k)
    assert n_active >= 20 and not np.array_equal(ref, blend)
    fits = _lds_resident(step, k) <= LDS
    streamed = ctx.stage_tile_blur(blend, md, step, k, form=1)
    assert np.array_equal(streamed, ref), "streamed form: %d of %d pixels differ" % (int((streamed != ref).sum()), ref.size)
    if fits:
        resident = ctx.stage_tile_blur(blend, md, step, k, form=0)
        assert np.array_equal(resident, ref) and np.array_equal(resident, streamed)
    chosen = ctx.stage_tile_blur(blend, md, step, k, form=-1)
    assert np.array_equal(chosen, ref)


def test_geometry_list_covers_what_it_claims():
    fit = [g for g in GEOMETRIES if _lds_resident(g[2], g[3]) <= LDS]
    assert len(fit) >= 2 and len(fit) <= len(GEOMETRIES) - 4
    assert any(g[3] % 2 == 0 for g in GEOMETRIES) and any(g[3] % 2 == 1 for g in GEOMETRIES)
    assert _lds_resident(40, 150) > LDS and _lds_resident(75, 115) > LDS and _lds_resident(5, 200) > LDS
    assert (120 + 180 - 1) * 120 * 8 > LDS   # row sums alone


def test_stage_tile_blur_argument_errors(pf, ctx):
    blend, md = random_inputs(1200, 900, 40, 5)
    ok = dict(step=40, k=150, form=1)
    for bad in (dict(step=0), dict(step=-3), dict(k=0), dict(k=-1), dict(step=900), dict(step=1200), dict(k=1801), dict(k=4000), dict(form=0),
                dict(form=2), dict(form=-2)):
        with pytest.raises(pf.PanoflowError):
            ctx.stage_tile_blur(blend, md, **dict(ok, **bad))
    # the reach of an even window is k/2, of an odd one (k-1)/2: 1799 (reach 899) is the widest a 900-row canvas takes
    assert ctx.l.pf_stage_tile_blur(ctx.h, None, md.ctypes.data_as(C.c_void_p), 1200, 900, 40, 150, 1) != 0
    assert ctx.l.pf_stage_tile_blur(ctx.h, blend.ctypes.data_as(C.c_void_p), None, 1200, 900, 40, 150, 1) != 0
    small_b, small_md = random_inputs(64, 48, 2, 6)
    with pytest.raises(pf.PanoflowError):
        ctx.stage_tile_blur(small_b, small_md, 2, 97, 1)     # reach 48 = rows
    out = ctx.stage_tile_blur(small_b, small_md, 2, 95, 1)   # reach 47: the widest window of a 48-row canvas
    assert out.shape == small_b.shape


def test_widest_window_of_a_small_canvas(ctx, orc):
    """reach = min(cols, rows) - 1: every border of the window is a reflection"""
    blend, md = random_inputs(64, 48, 2, 6)
    ref, n_active = tile_pass_reference(orc, blend, md, 2, 95)
    assert n_active >= 20
    assert np.array_equal(ctx.stage_tile_blur(blend, md, 2, 95, 1), ref)
    assert np.array_equal(ctx.stage_tile_blur(blend, md, 2, 95, 0), ref)


def test_tall_canvas_blend_smooth_vs_oracle(ctx, orc):
    """400x26200 derives step 2 / k 201, 166,448 B: refused before the streamed form.  About 2 % of the 2.6 M tiles are active, in
    clusters of adjacent tiles (what the CPU oracle can afford: ~2 s per percent)."""
    cols, rows, step = 400, 26200, 2
    assert _lds_resident(cols // 200, rows // 130) == 166448
    rng = np.random.default_rng(99)
    blend, _ = random_inputs(cols, rows, step, 98)
    md = np.zeros((rows, cols), np.float32)
    for _ in range(140):   # clusters of 20 x 20 tiles
        ty, tx = int(rng.integers(0, rows // step - 20)), int(rng.integers(0, cols // step - 20))
        md[ty * step:(ty + 20) * step, tx * step:(tx + 20) * step] = 3.0
    n_active = len(active_tiles(md, step)[0])
    assert n_active >= 20000
    ref = orc.blend_smooth(blend, md)
    got = ctx.stage_blend_smooth(blend, md)
    assert np.array_equal(got, ref), "%d of %d pixels differ" % (int((got != ref).sum()), ref.size)


def test_tall_canvas_stitch_step_vs_oracle_fixture(pf, synth):
    """One stitch step on 400x26200 (pixflow_low): map, ramp and MergedDis of pf_stitch_prepare and the composite of pf_stitch_step
    against the oracle fixture (tests/golden/make_tall_canvas_golden.py), then two frames through pf_stitch_step_batch against
    pf_stitch_step of each."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tall_canvas_400x26200.npz"))
    cols, rows, seed, pct, rs = int(g["cols"]), int(g["rows"]), int(g["seed"]), int(g["max_pct"]), int(g["row_stride"])
    assert pct == pf.max_percentage_by_name(str(g["algorithm"]))

    def gen(s, device):
        L, R = synth.make_canvas_pair(cols, rows, s, device)
        return L.cpu().numpy(), R.cpu().numpy()

    L, R = gen(seed, "cuda")
    if [_sha(L), _sha(R)] != list(g["sha_inputs"]):
        L, R = gen(seed, "cpu")
    assert [_sha(L), _sha(R)] == list(g["sha_inputs"]), "synthetic canvases differ from the ones the fixture was computed on"
    c = pf.Context(0, cols, rows)
    mp, ovl, ovr, bl, md = c.stitch_prepare(L, R)
    assert len(active_tiles(md, cols // 200)[0]) == int(g["active_tiles"]) >= 400000
    assert _sha(mp) == str(g["sha_map"]) and _sha(md) == str(g["sha_md"])
    assert _sha(bl) == str(g["sha_blend"]), "ramp differs from the oracle's in %d of %d sampled pixels" % (int((bl[::rs] != g["blend_sub"]).sum()), g["blend_sub"].size)
    del mp, ovl, ovr, bl, md
    out = c.stitch_step(L, R, pct)
    assert _sha(out) == str(g["sha_final"]), "composite differs from the oracle's in %d of %d sampled bytes" % (int((out[::rs] != g["final_sub"]).sum()), g["final_sub"].size)
    L2, R2 = gen(seed + 1, "cuda")
    out2 = c.stitch_step(L2, R2, pct)
    assert not np.array_equal(out2, out)
    both = c.stitch_step_batch([L, L2], [R, R2], pct, in_flight=2)
    assert np.array_equal(both[0], out) and np.array_equal(both[1], out2)
    c.close()
