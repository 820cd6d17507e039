"""CPU tier of the device PNG encoder's tests: the strict reader the GPU tests judge by (tests/png_decode_ref.py) against hand-built
files, and the GPU tests' images against what they are named for -- both from numpy and stdlib zlib alone; the block-level inflate
against zlib; and the serial model of the encoder (tests/png_model.py): its files decode, and every branch case reaches its branch."""
import os
import re
import zlib

import numpy as np
import pytest

import png_cases
import png_decode_ref as R
import png_model as M


def _image(cols, rows, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 4), dtype=np.uint8)


@pytest.mark.parametrize("ftype", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("cols,rows", [(1, 1), (1, 4), (5, 1), (9, 7)])
def test_round_trip_each_filter(ftype, cols, rows):
    img = _image(cols, rows, 10 * ftype + cols)
    data = R.frame(cols, rows, zlib.compress(R.filter_rows(img, [ftype] * rows)))
    got, types = R.decode(data, want_types=True)
    assert np.array_equal(got, img) and list(types) == [ftype] * rows


def test_round_trip_mixed_filters_and_split_idat():
    img = _image(13, 10, 5)
    types = [0, 1, 2, 3, 4, 4, 3, 2, 1, 0]
    z = zlib.compress(R.filter_rows(img, types), 9)
    for idat_max in (None, 7, 1):
        got, t = R.decode(R.frame(13, 10, z, idat_max), want_types=True)
        assert np.array_equal(got, img) and list(t) == types


def _good():
    img = _image(6, 5, 3)
    return bytearray(R.frame(6, 5, zlib.compress(R.filter_rows(img, [4] * 5))))


def test_refuses_flipped_crc_bit_in_every_chunk():
    good = _good()
    R.decode(good)
    pos = 8
    while pos < len(good):
        n = int.from_bytes(good[pos:pos + 4], "big")
        for at in (pos + 8 + n, pos + 4):          # the CRC itself, and a byte the CRC covers
            bad = bytearray(good); bad[at] ^= 0x10
            with pytest.raises(R.PngError):
                R.decode(bad)
        pos += 12 + n


def test_refuses_truncated_stream_and_bad_fields():
    good = _good()
    for cut in (1, 4, 12, 13, 20):
        with pytest.raises(R.PngError):
            R.decode(good[:-cut])
    img = _image(6, 5, 3)
    raw = R.filter_rows(img, [0] * 5)
    z = zlib.compress(raw)
    with pytest.raises(R.PngError):                # deflate data cut short, chunk CRCs right
        R.decode(R.frame(6, 5, z[:-9]))
    with pytest.raises(R.PngError):                # wrong Adler-32
        R.decode(R.frame(6, 5, z[:-1] + bytes([z[-1] ^ 1])))
    with pytest.raises(R.PngError):                # bytes after the zlib stream
        R.decode(R.frame(6, 5, z + b"\0"))
    with pytest.raises(R.PngError):                # a row short
        R.decode(R.frame(6, 6, z))
    with pytest.raises(R.PngError):                # filter type 5
        R.decode(R.frame(6, 5, zlib.compress(bytes([5]) + raw[1:])))
    with pytest.raises(R.PngError):
        R.decode(good + b"\0")                     # bytes after IEND
    bad = bytearray(good); bad[0] = 0x88
    with pytest.raises(R.PngError):
        R.decode(bad)


# ---- the GPU tests' images are what they are named for ----
def test_noise_image_does_not_compress():
    img = png_cases.noise(300, 200, 1)
    for types in ([0] * 200, [2] * 200):
        raw = R.filter_rows(img, types)
        assert len(zlib.compress(raw, 9)) >= 0.99 * len(raw)


def test_constant_images_are_one_run():
    for bgra in ((0, 0, 0, 0), (7, 7, 7, 255)):
        img = png_cases.constant(300, 200, bgra)
        assert (img.reshape(-1, 4) == img[0, 0]).all()


def _filter_sums(img):
    """per row and filter type: the sum of absolute residuals, residual bytes read as signed"""
    rows = img.shape[0]
    out = np.zeros((rows, 5), np.int64)
    for f in range(5):
        res = np.frombuffer(R.filter_rows(img, [f] * rows), np.uint8).reshape(rows, -1)[:, 1:].astype(np.int64)
        out[:, f] = np.where(res < 128, res, 256 - res).sum(1)
    return out


def test_ramp_images_leave_one_filter_the_smallest_sum():
    s = _filter_sums(png_cases.ramp_sub())
    assert (s[:, 1] < s[:, 0]).all() and (s[:, 1] < s[:, 2]).all() and (s[:, 1] < s[:, 3]).all() and (s[:, 1] <= s[:, 4]).all()
    s = _filter_sums(png_cases.ramp_up())[1:]
    assert (s[:, 2] < s[:, 0]).all() and (s[:, 2] < s[:, 1]).all() and (s[:, 2] < s[:, 3]).all() and (s[:, 2] <= s[:, 4]).all()


def test_alpha_noise_is_noise_in_alpha_only():
    img = png_cases.alpha_noise(300, 200, 2)
    assert (img[:, :, :3] == img[0, 0, :3]).all()
    a = img[:, :, 3].tobytes()
    assert len(zlib.compress(a, 9)) >= 0.99 * len(a)


def test_exact_fit_shapes_fill_whole_segments(pf):
    if not os.path.exists(pf.SO_PATH):
        pytest.skip("libpanoflow.so is not built")
    S = pf.png_segment_bytes()
    names = sorted(png_cases.small_cases(S))
    for k in (1, 2):
        full = png_cases.fit_rows(S, k)
        lens = {}
        for rows in (full - 1, full, full + 1):
            name = "fit%d_noise_%dx%d" % (k, png_cases.FIT_COLS, rows)
            assert name in names
            img = png_cases.small_cases(S)[name]
            lens[rows] = len(R.filter_rows(img, [0] * rows))
        assert lens[full] == k * S
        assert lens[full - 1] == k * S - (4 * png_cases.FIT_COLS + 1) and lens[full + 1] == k * S + (4 * png_cases.FIT_COLS + 1)
    assert pf.png_bound(300, 200) >= 300 * 200 * 4 + 200


# ---- the block-level inflate ----
def _trace_inputs():
    rng = np.random.default_rng(11)
    text = b"".join(b"row %d of the table; " % (k % 37) for k in range(900))
    return {"empty": b"", "one": b"x", "text": text, "noise": rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(),
            "few_values": rng.integers(0, 3, 20000, dtype=np.uint8).tobytes(), "zeros": bytes(70000),
            "smooth": png_cases.smooth(65, 37).tobytes() + text[:3000]}


@pytest.mark.parametrize("level", [1, 9])
@pytest.mark.parametrize("name", sorted(_trace_inputs()))
def test_inflate_trace_agrees_with_zlib(name, level):
    src = _trace_inputs()[name]
    z = zlib.compress(src, level)
    raw, blocks = R.inflate_trace(z)
    assert raw == zlib.decompress(z) == src
    assert [b["bfinal"] for b in blocks] == [0] * (len(blocks) - 1) + [1]
    assert blocks[0]["start_bit"] == 0 and all(a["end_bit"] == b["start_bit"] for a, b in zip(blocks, blocks[1:]))
    # the tokens alone rebuild the bytes
    out = bytearray()
    for b in blocks:
        for t in b["tokens"]:
            if isinstance(t, int):
                out.append(t)
            else:
                for _ in range(t[0]):
                    out.append(out[-t[1]])
    assert bytes(out) == src


def _stored(data, final):
    return bytes([final]) + len(data).to_bytes(2, "little") + (len(data) ^ 0xffff).to_bytes(2, "little") + data


def _zwrap(deflate, raw):
    return b"\x78\x01" + deflate + zlib.adler32(raw).to_bytes(4, "big")


def test_inflate_trace_on_hand_built_stored_blocks():
    a, b = b"hello, ", b"stored blocks"
    z = _zwrap(_stored(a, 0) + _stored(b"", 0) + _stored(b, 0) + _stored(b"", 1), a + b)
    raw, blocks = R.inflate_trace(z)
    assert raw == zlib.decompress(z) == a + b
    assert [(k["btype"], k["bfinal"], len(k["tokens"])) for k in blocks] == [(0, 0, 7), (0, 0, 0), (0, 0, 13), (0, 1, 0)]
    assert [k["start_bit"] for k in blocks] == [0, 8 * 12, 8 * 17, 8 * 35] and blocks[0]["data_byte"] == 5 and blocks[-1]["end_bit"] == 8 * 40
    # a fixed-Huffman block ahead of a stored one: the stored block's header is the next three bits, its LEN on the next byte boundary
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    fixed = c.compress(b"abcabcabcabc") + c.flush(zlib.Z_SYNC_FLUSH)        # ends with an empty stored block, BFINAL = 0
    raw, blocks = R.inflate_trace(_zwrap(fixed + _stored(b"!", 1), b"abcabcabcabc!"))
    assert raw == b"abcabcabcabc!" and [k["btype"] for k in blocks] == [1, 0, 0]
    assert blocks[0]["tokens"][:3] == [97, 98, 99] and blocks[0]["tokens"][-1][1] == 3 and blocks[2]["tokens"] == [33]


def _bits(fields):
    """(value, width) fields packed from the least significant bit"""
    acc = n = 0
    for v, w in fields:
        acc |= v << n; n += w
    return acc.to_bytes((n + 7) // 8, "little")


def test_inflate_trace_refuses_what_rfc_1951_forbids():
    good = _zwrap(_stored(b"abc", 1), b"abc")
    assert R.inflate_trace(good)[0] == b"abc"
    bad = {
        "LEN != ~NLEN": good[:5] + bytes([good[5] ^ 1]) + good[6:],
        "block type 3": _zwrap(bytes([0b111]), b""),
        "wrong Adler-32": good[:-1] + bytes([good[-1] ^ 1]),
        "bytes behind the last block": _zwrap(_stored(b"abc", 1) + b"\0", b"abc"),
        "ends inside": _zwrap(_stored(b"abc", 0), b"abc"),
        "bad zlib header": b"\x78\x02" + good[2:],
        # fixed block, BFINAL: the literal 'a' (0x61 + 0x30 = 10010001, sent from its most significant bit), then length 3 (symbol 257: 0000001),
        # distance symbol 1 (00001 -> 10000 reversed) = distance 2 with one byte of output
        "beyond the output": _zwrap(_bits([(1, 1), (1, 2), (0b10001001, 8), (0b1000000, 7), (0b10000, 5), (0, 7)]), b"aaaa"),
        # dynamic block whose code-length code has three codes of one bit
        "over-subscribed": _zwrap(_bits([(1, 1), (2, 2), (0, 5), (0, 5), (0, 4), (1, 3), (1, 3), (1, 3), (0, 3)]) + bytes(8), b""),
        # ... and one with a single code of one bit
        "incomplete": _zwrap(_bits([(1, 1), (2, 2), (0, 5), (0, 5), (0, 4), (1, 3), (0, 3), (0, 3), (0, 3)]) + bytes(8), b""),
    }
    for what, z in bad.items():
        with pytest.raises(R.PngError, match=re.escape(what)):
            R.inflate_trace(z)
        if what not in ("bytes behind the last block",):      # zlib.decompress lets trailing bytes pass; R.inflate does not
            with pytest.raises(zlib.error):
                zlib.decompress(z)


# ---- the serial model: its files are valid, and every case reaches the branch it is named for ----
BRANCH = png_cases.branch_cases()
_ENCODED = {}


def _model(name):
    if name not in _ENCODED:
        _ENCODED[name] = M.encode(BRANCH[name])
    return _ENCODED[name]


@pytest.mark.parametrize("name", sorted(BRANCH))
def test_model_files_decode_and_keep_the_stream_promises(name):
    data, info = _model(name)
    got, types = R.decode(data, want_types=True)
    assert np.array_equal(got, BRANCH[name]) and np.array_equal(types, info["types"])
    assert zlib.decompress(R.zlib_stream(data)) == info["stream"]
    M.check_against_model(data, info)


def test_model_on_the_older_images():
    for img in (png_cases.smooth(65, 37), png_cases.noise(63, 3, 1), png_cases.constant(300, 200, (7, 7, 7, 255)), png_cases.alpha_noise(300, 200, 2)):
        data, info = M.encode(img)
        assert np.array_equal(R.decode(data), img)
        M.check_against_model(data, info)


@pytest.mark.parametrize("name", sorted(png_cases.filter_cases()))
def test_filter_cases_decide_as_named(name):
    img, row, what = png_cases.filter_cases()[name]
    s = M.filter_sums(img)[row].tolist()
    chosen = int(M.filter_image(img)[1][row])
    others = lambda *keep: [s[g] for g in range(5) if g not in keep]
    if what[0] == "strict":
        assert chosen == what[1] and s[what[1]] < min(others(what[1]))
    elif what[0] == "tie":
        a, b = what[1:]
        assert a < b and chosen == a and s[a] == s[b] < min(others(a, b))
    elif what[0] == "all_tie":
        assert chosen == 0 and len(set(s)) == 1
    else:
        f, runner, by = what[1:]
        assert chosen == f and s[runner] - s[f] == by and s[f] == min(s) and s[runner] == min(x for x in s if x > s[f])
    print(name, "row", row, "sums", s, "->", chosen)


def test_filter_cases_hold_the_residuals_they_are_named_for():
    for name, none_res, sub_res in (("filter_res_80", 0x80, 0x7f), ("filter_res_81", 0x81, 0x80), ("filter_res_7f", 0x82, 0x7f)):
        planes = M.residual_planes(png_cases.filter_cases()[name][0])
        assert (planes[0, 0, 1] == none_res).all() and (planes[1, 0, 1] == sub_res).all()
    # the last pixel alone decides: without it the five sums are equal and None would win
    for cols in (255, 256, 257, 513):
        img = png_cases.filter_cases()["filter_last_pixel_%d" % cols][0]
        assert img.shape == (1, cols, 4) and len(set(M.filter_sums(img[:, :-1])[0].tolist())) == 1
        assert M.filter_image(img[:, :-1])[1][0] == 0 and M.filter_image(img)[1][0] == 1
    assert M.filter_image(png_cases.filter_cols1())[1].tolist() == [0, 2, 2, 2, 3, 0]
    assert M.filter_image(png_cases.filter_first_row())[1].tolist() == [1, 2, 2]


def _segment_runs(info):
    """per segment the set of (start, length, class) of its maximal runs"""
    stream = info["stream"]
    return [set(M.runs(M.classes(stream[at:at + M.SEG]))) for at in range(0, len(stream), M.SEG)]


def _tokens_by_position(seg_info):
    out, at = {}, 0
    for t in seg_info["tokens"]:
        out[at] = t
        at += 1 if isinstance(t, int) else t[0]
    assert at == seg_info["n"]
    return out


def _pieces(n):
    return [min(M.PIECE, n - a) for a in range(0, n, M.PIECE)]


@pytest.mark.parametrize("case", ["parse_runs", "parse_chunks", "parse_segment_end"])
def test_parse_cases_hold_the_runs_they_mark(case):
    img, marks = getattr(png_cases, case)()
    data, info = _model(case)
    assert info["types"].tolist() == [1]                     # Sub: the stream is the one the case built
    assert not any(s["stored"] for s in info["segments"])
    runs, toks = _segment_runs(info)[0], _tokens_by_position(info["segments"][0])
    for name, (start, n, cls) in marks.items():
        assert (start, n, cls) in runs, (name, start, n, cls)
        at = start
        for piece in _pieces(n):                             # cut into 258s from the run's start; a piece under 3 is literals
            if piece >= 3:
                assert toks[at] == (piece, cls), (name, at)
            else:
                assert all(isinstance(toks[at + k], int) for k in range(piece)), (name, at)
            at += piece
    if case == "parse_runs":
        assert {marks["run4_%d" % n][1] for n in png_cases.RUN_LENGTHS} == set(png_cases.RUN_LENGTHS)
        assert [marks["run1_%d" % n][1:] for n in (1, 2, 3)] == [(1, 1), (2, 1), (3, 1)]
        start, n, _ = marks["both"]                          # equal to the byte 1 back and the byte 4 back: class 4 takes it
        s = info["stream"]
        assert all(s[j] == s[j - 1] == s[j - 4] for j in range(start, start + n))
    if case == "parse_chunks":
        m = marks
        assert [m[k][0] % 64 for k in ("start_63", "start_64", "start_65")] == [63, 0, 1]
        for k in ("span3_short", "span3_cut"):               # three whole chunks inside, both ends inside a chunk
            a, e = m[k][0], m[k][0] + m[k][1]
            assert a % 64 and e % 64 and e // 64 - (a // 64 + 1) == 3
        assert m["span3_short"][1] < M.PIECE < m["span3_cut"][1]
        assert (m["sep_last_a"][0] + m["sep_last_a"][1]) % 64 == 63 and m["sep_last_b"][0] % 64 == 0
        assert (m["sep_first_a"][0] + m["sep_first_a"][1]) % 64 == 0 and m["sep_first_b"][0] % 64 == 1
        assert (m["change_1_4"][0] + 3) % 64 == 0 and m["change_4"][0] % 64 == 0
        assert m["pair_over_edge"][0] % 64 == 63 and m["pair_over_edge"][1:] == (2, 1)
        assert m["whole_chunk"][0] % 64 == 62 and m["whole_chunk"][1] == 68
    if case == "parse_segment_end":
        start, n, _ = marks["to_last_byte"]
        assert start + n == M.SEG and len(info["segments"]) == 2
        assert M.classes(info["stream"][M.SEG:])[:8].tolist() == [0] * 8


def test_no_class_1_run_is_longer_than_three():
    """the fourth position of a run of equal bytes equals the byte 4 back, which is class 4: lengths above 3 exist at distance 4 only"""
    for name in sorted(BRANCH):
        for runs in _segment_runs(_model(name)[1]):
            assert all(n <= 3 for _, n, cls in runs if cls == 1), name


def test_parse_cases_across_a_segment_boundary():
    for case, head in (("parse_segment_cross", [0, 0, 0, 0]), ("parse_segment_cross_constant", [0, 1, 1, 1])):
        img, marks = getattr(png_cases, case)()
        data, info = _model(case)
        assert info["types"].tolist() == [1] and [s["n"] for s in info["segments"]] == [M.SEG, 4 * img.shape[1] + 1 - M.SEG]
        start, n, _ = marks["across"]
        r0, r1 = _segment_runs(info)
        s = info["stream"]
        assert all(s[j] == s[j - 4] for j in range(start + 4, start + n))       # one run to a reader of the whole stream
        if head[1]:
            assert (start, 3, 1) in r0 and (start + 3, M.SEG - start - 3, 4) in r0
        else:
            assert (start, M.SEG - start, 4) in r0
        # the second segment cannot look back: its first four positions are not class 4, the run resumes at position 4
        assert M.classes(s[M.SEG:])[:4].tolist() == head and (4, start + n - M.SEG - 4, 4) in r1
        t1 = _tokens_by_position(info["segments"][1])
        assert t1[4] == (start + n - M.SEG - 4, 4) and all(not isinstance(t1[k], tuple) or t1[k][1] == 1 for k in range(4) if k in t1)


def test_tail_cases_end_on_1_3_5_bytes():
    for name, (img, tail) in png_cases.tail_cases().items():
        info = _model(name)[1]
        assert [s["n"] for s in info["segments"]] == [M.SEG, tail] and tail % 4 and info["segments"][1]["stored"]
        assert any(info["stream"][M.SEG:])                   # the bytes behind the last whole dword are not zeros


def test_limit_cases_reach_both_length_limits():
    for name, (img, which, depth) in png_cases.limit_cases().items():
        info = _model(name)[1]
        seg = info["segments"][0]
        assert info["types"].tolist() == [1] and len(info["segments"]) == 1 and not seg["stored"]
        assert all(isinstance(t, int) for t in seg["tokens"])            # no match: the histogram is the designed one
        hist, lens, limit = (seg["hist"], seg["lens"], 15) if which == "litlen" else (seg["cl_hist"], seg["cl_lens"], 7)
        assert M.plain_huffman(hist)[0] == depth > limit and max(lens) == limit
        assert seg["limited15"] == (which == "litlen") and seg["limited7"] == (which == "cl")
        assert sum(h * l for h, l in zip(hist, lens)) > M.plain_huffman(hist)[1]          # the fold costs bits: it did change lengths
        if which == "litlen":
            assert sorted(h for h in hist if h)[:6] == [1, 1, 2, 3, 5, 8] and seg["depth_litlen"] == depth
        else:
            want = dict(png_cases.LIMIT7_LENGTH_COUNTS)
            assert {l: seg["lens"].count(l) for l in want} == want and seg["depth_cl"] == depth
            assert 16 not in [s for s, h in enumerate(hist) if h]        # no length went out as a repeat
        print(name, which, "unrestricted depth", depth, "histogram", sorted(h for h in hist if h), "sums", info["sums"][0].tolist())


def test_lengths_repeat_case_sends_full_and_partial_repeats():
    info = _model("lengths_repeat_26x1")[1]
    seg = info["segments"][0]
    assert info["types"].tolist() == [1] and not seg["stored"] and all(isinstance(t, int) for t in seg["tokens"])
    seq = M.run_length_code(seg["lens"] + list(M.DIST_LENS))
    at = seq.index((16, 3))
    assert seq[at - 1:at + 6] == [(5, 0), (16, 3), (16, 3), (16, 3), (5, 0), (5, 0), (4, 0)] and (16, 1) in seq      # 1 + 18 + 2 fives; 1 + 4 fours
    assert seg["lens"].count(5) == 21 and seg["cl_hist"][16] == 4


def test_threshold_cases_straddle_the_stored_rule():
    for name, (img, diff) in png_cases.threshold_cases().items():
        seg = _model(name)[1]["segments"][0]
        assert seg["coded_bytes"] - (seg["n"] + M.OVERHEAD) == diff and seg["stored"] == (diff >= 0)


# ---- the model's segment cache and the 1025-segment image (tests/test_gpu_png.py sends it to the device) ----
def test_segment_cache_changes_nothing():
    """a periodic image of 15 segments: with the cache the model encodes the distinct (segment, last) pairs only, and writes the same file"""
    img = png_cases.many_segments(M.SEG)[:15 * png_cases.MANY_BAND]
    cache = {}
    cached, info = M.encode(img, cache=cache)
    plain, plain_info = M.encode(img)
    assert cached == plain and len(info["segments"]) == len(plain_info["segments"]) == 15
    assert len(cache) == 9 and sorted(last for _, last in cache) == [False] * 8 + [True]       # segment 0, the period's seven, the last
    assert [s["coded_bytes"] for s in info["segments"]] == [s["coded_bytes"] for s in plain_info["segments"]]
    M.check_against_model(cached, info)


def test_many_segments_image_is_what_it_is_named_for():
    img = png_cases.many_segments(M.SEG)
    assert img.shape == (12300, 341, 4) and np.array_equal(img[84:], img[:-84]) and not np.array_equal(img[12:], img[:-12])
    stream, types, _ = M.filter_image(img)
    assert len(stream) == 1025 * M.SEG
    segs = [stream[k * M.SEG:(k + 1) * M.SEG] for k in range(1025)]
    assert all(segs[k] == segs[k + 7] for k in range(1, 1018))                                  # the stream repeats from segment 1 on
    assert len(set(segs[1:8])) == 7
