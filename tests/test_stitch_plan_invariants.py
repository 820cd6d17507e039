"""What a stitch plan rests on, pinned against the CPU oracle: along the whole 5-step chain of a rig, the overlap map and the
smoothed blend ramp depend on the alpha masks alone (equal for two seeds of one rig geometry, whose composites differ), and a
composite's alpha is > 0 exactly where one of its inputs' is -- so the R mask of a chained step is content-independent too."""
import numpy as np
import pytest

PCT = 20   # pixflow_search_20
COLS, ROWS = 520, 260


def _oracle_chain(orc, synth, seed):
    top, imgs = synth.make_stitch_set(COLS, ROWS, seed, 5)
    R = top.numpy()
    steps = []
    for im in imgs:
        L = im.numpy()
        mp, ovl, ovr, blend, _ = orc.stitch_prepare(L, R, True)
        f0, f1 = orc.flow_bidir(ovl, ovr, PCT)
        merged = orc.combine_novel_views(ovl, ovr, f0, f1, blend)
        out = orc.stitch_gather(L, R, merged, mp)
        steps.append((L, R, mp, blend, out))
        R = out
    return steps


@pytest.fixture(scope="module")
def chains(orc, synth):
    return _oracle_chain(orc, synth, 1234), _oracle_chain(orc, synth, 4321)


def test_map_and_ramp_depend_on_the_masks_alone(chains):
    a, b = chains
    for i, ((_, _, mpa, bla, outa), (_, _, mpb, blb, outb)) in enumerate(zip(a, b)):
        assert np.array_equal(mpa, mpb), "step %d: the maps of the two seeds differ in %d pixels" % (i + 1, int((mpa != mpb).sum()))
        assert np.array_equal(bla.view(np.uint32), blb.view(np.uint32)), "step %d: the ramps of the two seeds differ" % (i + 1)
        assert (mpa == 150).any(), "step %d has no overlap: the case checks nothing" % (i + 1)
        assert not np.array_equal(outa, outb), "step %d: the two seeds give the same composite" % (i + 1)


def test_composite_alpha_is_the_union_of_its_inputs(chains):
    for chain in chains:
        for i, (L, R, _, _, out) in enumerate(chain):
            want = (L[..., 3] > 0) | (R[..., 3] > 0)
            got = out[..., 3] > 0
            assert np.array_equal(got, want), "step %d: composite alpha > 0 differs from L | R in %d pixels" % (i + 1, int((got != want).sum()))
