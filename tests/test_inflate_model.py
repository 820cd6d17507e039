"""CPU tier: the deflate writer and the judge (tests/inflate_model.py) and the case list (tests/inflate_cases.py) the device inflate
kernel is held to.  Every well-formed case is accepted by libz's uncompress with its payload and read by libtiff (through Pillow) to
its image; every malformed one is refused with the reason class it is named for; every branch case reaches its branch, shown from the
writer's own parameters."""
import zlib

import numpy as np
import pytest

import inflate_cases as ic
import inflate_model as im
import tiff_cases
import tiff_model as tm


@pytest.fixture(scope="module")
def cases(synth):
    return ic.cases(synth)


def test_the_writer_round_trips_through_zlib():
    toks = [1, 2, 3, (5, 2), 200, (258, 1), (3, 9)]
    for stream in (im.fixed_stream(toks), im.dynamic_stream(toks)[0]):
        assert zlib.decompress(stream) == im.expand(toks)
    w = im.BitWriter()
    im.stored_block(w, b"abc", False); im.fixed_block(w, [100, (4, 1)], False); im.dynamic_block(w, [7, 8], im.flat_lengths({7, 8, 256}, 257), [0], True)
    assert zlib.decompress(im.zstream(w.getvalue(), b"abcddddd\x07\x08")) == b"abcddddd\x07\x08"
    assert [im.length_symbol(v)[0] for v in (3, 10, 11, 257, 258)] == [257, 264, 265, 284, 285]
    assert [im.distance_symbol(v)[0] for v in (1, 4, 5, 24577, 32768)] == [0, 3, 4, 29, 29] and im.distance_symbol(32768)[2] == 8191


def test_every_case_is_accepted_with_its_payload(cases):
    for name, c in sorted(cases.items()):
        img, verdicts = im.decode(c.file)
        assert all(ok for ok, _ in verdicts) and np.array_equal(img, tm.expected_bgra(c.img)), name
        assert tm.parse(c.file)[259][0] in (8, 32946), name


def test_pillow_reads_every_case(cases):
    skipped = [k for k, c in cases.items() if not c.pillow]
    assert sorted(skipped) == ["tok_clipped_match_then_end_dynamic", "tok_clipped_match_then_end_fixed", "tok_clipped_match_then_invalid_symbol",
                               "tok_clipped_stored_block", "tok_over_long_stream", "tok_trailer_cut_by_one"]   # (libtiff wants a whole stream of the right size)
    for name, c in sorted(cases.items()):
        if c.pillow:
            assert np.array_equal(tiff_cases.pillow_read(c.file), c.img), name


def test_every_malformed_strip_is_refused_for_its_reason():
    bad = ic.malformed()
    assert {b.reason for b in bad.values()} == {im.REASON_OK, im.REASON_ZLIB_HEADER, im.REASON_BLOCK_HEADER, im.REASON_CODE_LENGTHS,
                                                im.REASON_INVALID_SYMBOL, im.REASON_FAR_BACK, im.REASON_DATA_CHECK}
    for name, b in sorted(bad.items()):
        verdicts = im.decode(b.file)[1]
        assert verdicts[b.strip] == (False, b.reason) and verdicts[1 - b.strip] == (True, 0), (name, verdicts)


def _block_types(stream):
    """(BFINAL, BTYPE) of the first block"""
    return stream[2] & 1, (stream[2] >> 1) & 3


def test_every_branch_case_reaches_its_branch(cases):
    f = {k: c.facts for k, c in cases.items()}
    strips = {k: im.strips(c.file) for k, c in cases.items()}
    # the shapes the issue names
    assert len(strips["pillow_65x37"]) == 1 and strips["pillow_65x37"][0][1] == 9620 and _block_types(strips["pillow_65x37"][0][0]) == (1, 2)
    assert tm.parse(cases["pillow_65x37_pred2"].file)[317] == [2]
    assert len(strips["pillow_stitch_480x320"]) == 320
    # (the transparent border's constant rows are fixed blocks either way; textured rows are dynamic blocks without the predictor)
    assert {_block_types(s)[1] for s, _ in strips["pillow_stitch_480x320"]} == {1, 2} and 1 in {_block_types(s)[1] for s, _ in strips["pillow_stitch_480x320_pred2"]}
    assert [n for _, n in strips["pillow_9000x4"]] == [36000] * 4
    geo = [k for k in cases if k.startswith("geom_")]
    assert {k[-1] for k in geo} == {"0", "1", "2", "3"} and {tm.parse(cases[k].file)[259][0] for k in geo} == {8, 32946}
    assert {cases[k].img.shape[2] for k in geo} == {3, 4} and {cases[k].file[:2] for k in geo} == {b"II", b"MM"}
    # zlib's strategies: stored, fixed, and streams that start with a non-final block
    assert _block_types(strips["zlib_stored"][0][0])[1] == 0 and _block_types(strips["zlib_stored_72000"][0][0]) == (0, 0)
    assert strips["zlib_stored_72000"][0][1] == 72000 > 65535
    assert _block_types(strips["zlib_fixed"][0][0])[1] == 1 and _block_types(strips["zlib_level9"][0][0])[1] == 2
    assert _block_types(strips["zlib_rle"][0][0]) == (0, 2) and _block_types(strips["zlib_huffman_only"][0][0]) == (0, 2)
    assert b"\x00\x00\xff\xff" in strips["sync_flush"][0][0]   # the empty stored block in the middle
    assert f["far_match_32768"] == dict(distance=32768, symbol=(29, 13, 8191)) and strips["far_match_32768"][0][1] >= 32771
    # explicit code lengths
    assert f["tok_lengths_1_to_15"] == dict(max_len=15, kraft=32768, dist_codes=0)
    assert f["tok_code_length_code_7_bits"]["cl_max"] == 7 and f["tok_code_length_code_7_bits"]["cl_kraft"] == 32768
    assert f["tok_code_length_code_7_bits"]["cl_used"][16] == 7 and set(f["tok_code_length_code_7_bits"]["cl_used"]) >= {0, 7, 8, 16, 18}
    for sym in (16, 17, 18):
        facts = f["tok_repeat_%d_crosses_hlit" % sym]
        assert any(q[0] == sym and q[2] < facts["nlen"] < q[2] + q[3] for q in facts["seq"]), sym
    assert f["tok_no_distance_code"]["dist_lens"] == [0] and f["tok_single_one_bit_distance_code"] == dict(dist_lens=[1], kraft=16384)
    # matches
    assert (258, 1) in f["tok_length_258_distance_1"]["tokens"]
    assert {(ln, d) for ln, d in (t for t in f["tok_distance_below_length_2_3_4"]["tokens"] if isinstance(t, tuple)) if d < ln} == {(10, 2), (11, 3), (13, 4)}
    assert f["tok_chain_three_deep"]["tokens"][3:6] == [(3, 3)] * 3
    toks = f["tok_token_straddles_turns"]["tokens"]
    assert isinstance(toks[ic.BATCH_TOKENS - 1], tuple) and isinstance(toks[ic.BATCH_TOKENS], tuple) and len(toks) > 2 * ic.BATCH_TOKENS
    turn2 = toks[ic.BATCH_TOKENS:2 * ic.BATCH_TOKENS]
    assert len(im.expand(toks)) > len(im.expand(toks[:ic.BATCH_TOKENS])) + ic.BATCH_BYTES or any(isinstance(t, tuple) for t in turn2)
    # ends
    assert f["tok_over_long_stream"]["stream_bytes"] == strips["tok_over_long_stream"][0][1] + 50
    assert im.uncompress(*strips["tok_over_long_stream"][0])[0] == -5 and im.uncompress(*strips["tok_ends_exactly_full"][0])[0] == 0
    assert im.uncompress(*strips["tok_trailer_cut_by_one"][0])[0] == -5 and im.uncompress(*strips["tok_bytes_after_trailer"][0])[0] == 0
    assert strips["tok_bytes_after_trailer"][0][0].endswith(b"\xa5" * 4)
    # a match across the strip's end: it starts inside the strip, ends past it, and what follows it is never read
    for name in ("tok_clipped_match_then_end_fixed", "tok_clipped_match_then_end_dynamic", "tok_clipped_match_then_invalid_symbol"):
        toks, expect = f[name]["tokens"], f[name]["expect"]
        assert isinstance(toks[-1], tuple) and len(im.expand(toks[:-1])) < expect == strips[name][0][1] < len(im.expand(toks))
        assert im.uncompress(*strips[name][0])[0] == -5
    assert _block_types(strips["tok_clipped_match_then_end_fixed"][0][0])[1] == 1 and _block_types(strips["tok_clipped_match_then_end_dynamic"][0][0])[1] == 2
    with pytest.raises(zlib.error, match="invalid literal/length code"):   # zlib with room to go on does meet the symbol
        zlib.decompress(strips["tok_clipped_match_then_invalid_symbol"][0][0])
    assert zlib.decompress(strips["tok_clipped_match_then_end_fixed"][0][0])[:90] == im.uncompress(*strips["tok_clipped_match_then_end_fixed"][0])[1]
    assert f["tok_clipped_stored_block"] == dict(stored=100, expect=90) and im.uncompress(*strips["tok_clipped_stored_block"][0])[0] == -5


def test_the_judge_accepts_every_clip():
    toks = ic.clip_tokens()
    payload = im.expand(toks)
    ends = {len(im.expand(toks[:k])) for k in range(len(toks) + 1)}   # token boundaries
    sizes = range(3, len(payload) + 1, 3)
    assert any(n in ends for n in sizes) and sum(n not in ends for n in sizes) >= 10   # most sizes cut a match
    for stream in (im.fixed_stream(toks), im.dynamic_stream(toks)[0]):
        for n, data in ic.every_clip(stream, payload).items():
            ok, got, _ = im.judge(*im.strips(data)[0])
            assert ok and got == payload[:n], n


def test_the_judge_on_flips_and_truncations():
    raw, dyn, fix = ic.flip_streams()
    assert zlib.decompress(dyn) == zlib.decompress(fix) == raw and len(raw) == 90
    for stream in (dyn, fix):
        verdicts = im.decode(ic.every_flip(stream))[1]
        n_ok = sum(ok for ok, _ in verdicts)
        assert len(verdicts) == 8 * len(stream) and 0 < n_ok < len(verdicts) // 4   # most flips are refused, some are accepted as full
        cut = im.decode(ic.every_truncation(stream))[1]
        assert [ok for ok, _ in cut][-4:] == [True] * 4 and not any(ok for ok, _ in cut[:len(stream) // 2])
