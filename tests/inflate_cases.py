"""The deflate TIFFs the device inflate kernel is tested on, shared by the model's own tests (test_inflate_model.py), the host-run kernel
(test_tiff_inflate_host.py) and the GPU tier (test_gpu_inflate.py).  cases(synth): name -> Case(file bytes, the RGB(A) image, whether
libtiff must read it, facts about the stream from the writer's own parameters: the branch it is there for).  malformed(): name ->
Bad(file bytes, the strip that is bad, the reason class zlib gives).  Shapes are the smallest at which each branch can be reached."""
import collections
import zlib

import numpy as np

import inflate_model as im
import tiff_cases
from tiff_cases import noise, pillow_tiff, smooth

Case = collections.namedtuple("Case", "file img pillow facts")
Bad = collections.namedtuple("Bad", "file strip reason")

BATCH_TOKENS, BATCH_BYTES = 256, 4096   # kInfTokens, kInfBatchBytes in csrc/kernels_tiff.hip


def _row(payload, spp=3):
    """a one-row image whose samples are `payload`"""
    assert len(payload) % spp == 0
    return np.frombuffer(bytes(payload), np.uint8).reshape(1, -1, spp).copy()


def _one(stream, payload, spp=3):
    img = _row(payload, spp)
    return im.write_tiff(img, None, streams={0: stream}), img


def _lits(n, seed, lo=0, hi=256):
    return [int(v) for v in np.random.RandomState(seed).randint(lo, hi, n)]


def token_cases():
    """name -> (stream, payload the strip holds, facts); every payload is a multiple of 3 bytes"""
    out = {}
    # the 15-bit limit: literal/length lengths 1, 2, ..., 14, 15, 15 over the literals 0..14 and the end-of-block code
    lens = [0] * 257
    for k in range(15):
        lens[k] = k + 1
    lens[256] = 15
    toks = [k % 15 for k in range(300)] + [14] * 30
    s, _ = im.dynamic_stream(toks, lit_lens=lens, dist_lens=[0])
    out["lengths_1_to_15"] = (s, im.expand(toks), dict(max_len=max(lens), kraft=im.kraft(lens), dist_codes=0))
    # a 7-bit code-length code: lengths 1..7, 7 over eight of its symbols
    cl = [0] * 19
    for sym, ln in ((0, 1), (8, 2), (7, 3), (18, 4), (1, 5), (2, 6), (16, 7), (17, 7)):
        cl[sym] = ln
    toks = [k % 200 for k in range(600)]
    lit = im.flat_lengths(set(toks) | {256}, 257)   # lengths 7 and 8, zeros between
    s, seq = im.dynamic_stream(toks, lit_lens=lit, dist_lens=[0], cl_lens=cl)
    out["code_length_code_7_bits"] = (s, im.expand(toks), dict(cl_max=max(cl), cl_kraft=im.kraft(cl), cl_used={q[0]: cl[q[0]] for q in seq}))
    # runs of 16, 17 and 18 that cross from the literal/length lengths into the distance lengths
    toks = [97, 98, 99, 100, (3, 1), (4, 2), (3, 3), (4, 4)] * 12 + [97, 98, 99]
    lit = [0] * 259
    for sym in (97, 98, 99, 100):
        lit[sym] = 4
    lit[256] = lit[257] = lit[258] = 2
    s, seq = im.dynamic_stream(toks, lit_lens=lit, dist_lens=[2, 2, 2, 2])
    out["repeat_16_crosses_hlit"] = (s, im.expand(toks), dict(seq=seq, nlen=259))
    for name, zeros in (("repeat_17_crosses_hlit", 3), ("repeat_18_crosses_hlit", 9)):
        toks = [1, 2, 3, 4] * 4 + [(5, 9), 7, (5, 13), 7] * 10 + [1, 2]
        lit = im.flat_lengths({1, 2, 3, 4, 7, 256, 259}, 260 + zeros)   # `zeros` trailing zeros behind symbol 259 ...
        s, seq = im.dynamic_stream(toks, lit_lens=lit, dist_lens=[0] * 6 + [1, 1])   # ... run into the six leading zeros here
        out[name] = (s, im.expand(toks), dict(seq=seq, nlen=len(lit)))
    # matches
    toks = [7, (258, 1), 8, (258, 1), 9] + _lits(42, 3)
    out["length_258_distance_1"] = (im.fixed_stream(toks), im.expand(toks), dict(tokens=toks))
    toks = [1, 2, 3, 4, (10, 2), 5, (11, 3), 6, (13, 4), 9, 9]
    toks += _lits(-len(im.expand(toks)) % 3, 4)
    out["distance_below_length_2_3_4"] = (im.fixed_stream(toks), im.expand(toks), dict(tokens=toks))
    toks = [65, 66, 67, (3, 3), (3, 3), (3, 3), 68, 69, 70]
    out["chain_three_deep"] = (im.fixed_stream(toks), im.expand(toks), dict(tokens=toks))
    toks = _lits(150, 5, 0, 60)
    s, _ = im.dynamic_stream(toks, dist_lens=[0])
    out["no_distance_code"] = (s, im.expand(toks), dict(dist_lens=[0]))
    toks = [33, (5, 1), 34, (7, 1), 35] * 6
    s, _ = im.dynamic_stream(toks, dist_lens=[1])
    out["single_one_bit_distance_code"] = (s, im.expand(toks), dict(dist_lens=[1], kraft=im.kraft([1])))
    # a token that straddles two turns: by the token count (a match as token 256) and by the bytes (a match across byte 4096 of a turn)
    toks = _lits(255, 6) + [(100, 200), (90, 7)] + _lits(300, 7) + [(258, 1)] * 16 + _lits(3, 8)
    toks += _lits(-len(im.expand(toks)) % 3, 9)
    s, _ = im.dynamic_stream(toks)
    out["token_straddles_turns"] = (s, im.expand(toks), dict(tokens=toks))
    # ends
    toks = _lits(60, 10) + [(30, 60)]
    out["over_long_stream"] = (im.fixed_stream(toks + [(40, 5)] + _lits(10, 11)), im.expand(toks), dict(stream_bytes=len(im.expand(toks)) + 50))
    out["ends_exactly_full"] = (im.fixed_stream(toks), im.expand(toks), dict(stream_bytes=len(im.expand(toks))))
    out["trailer_cut_by_one"] = (im.fixed_stream(toks)[:-1], im.expand(toks), dict(cut=1))
    out["bytes_after_trailer"] = (im.fixed_stream(toks) + b"\xa5" * 4, im.expand(toks), dict(extra=4))
    # a match that straddles the strip's end (bytes 84..94 of a 90-byte strip): zlib fills the strip, keeps the rest of the pair pending
    # and reads nothing behind it -- neither the end-of-block and the trailer, which is the longer payload's, nor an invalid symbol
    toks = _lits(84, 12) + [(10, 5)]
    facts = dict(tokens=toks, expect=90)
    out["clipped_match_then_end_fixed"] = (im.fixed_stream(toks), im.expand(toks)[:90], facts)
    out["clipped_match_then_end_dynamic"] = (im.dynamic_stream(toks)[0], im.expand(toks)[:90], facts)
    w = im.BitWriter()
    im.fixed_block(w, toks + [("lit", 286)], True)
    out["clipped_match_then_invalid_symbol"] = (im.zstream(w.getvalue(), im.expand(toks)), im.expand(toks)[:90], facts)
    w = im.BitWriter()
    im.stored_block(w, bytes(_lits(100, 13)), True)
    out["clipped_stored_block"] = (im.zstream(w.getvalue(), bytes(_lits(100, 13))), bytes(_lits(100, 13))[:90], dict(stored=100, expect=90))
    return out


def clip_tokens():
    """96 bytes in which matches end at many positions: a strip of any smaller size cuts a literal, a match or the end"""
    return [1, 2, 3, 4, 5, 6] + [(7, 3), 9, (10, 6), 8, (3, 1)] * 4 + [10, 11]


def every_clip(stream, payload):
    """{strip size: a one-strip file holding `stream`, whose payload is longer than or equal to the strip}, every multiple of 3"""
    return {n: im.write_tiff(_row(payload[:n]), None, streams={0: stream}) for n in range(3, len(payload) + 1, 3)}


def sync_flush_stream(raw):
    c = zlib.compressobj(6)
    return c.compress(raw[:len(raw) // 2]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(raw[len(raw) // 2:]) + c.flush()


def far_match_stream(raw):
    """32,768 literals, then a length 3 at distance 32768 (distance symbol 29, extra 8191), then the rest as literals"""
    raw = bytes(raw)
    assert raw[32768:32771] == raw[0:3]
    return im.fixed_stream(list(raw[:32768]) + [(3, 32768)] + list(raw[32771:]))


def cases(synth):
    out = {}
    rgba = smooth(37, 65, 4, 3)
    out["pillow_65x37"] = Case(pillow_tiff(rgba, "tiff_adobe_deflate"), rgba, True, {})
    out["pillow_65x37_pred2"] = Case(pillow_tiff(rgba, "tiff_adobe_deflate", predictor=2), rgba, True, {})
    st = tiff_cases.stitch_image(synth)
    out["pillow_stitch_480x320"] = Case(pillow_tiff(st, "tiff_adobe_deflate", 1), st, True, {})
    out["pillow_stitch_480x320_pred2"] = Case(pillow_tiff(st, "tiff_adobe_deflate", 1, 2), st, True, {})
    wide = np.concatenate([noise(4, 3000, 4, 21), smooth(4, 6000, 4, 22)], axis=1)   # 9000 x 4: strips of 36,000 bytes
    out["pillow_9000x4"] = Case(pillow_tiff(wide, "tiff_adobe_deflate", 1), wide, True, {})
    # geometry: RGB and RGBA, both byte orders, both compression tags, every strip alignment, a predictor, several rows per strip
    for k, (spp, be, comp, pred, rps) in enumerate(((3, False, 8, 1, 1), (4, True, 32946, 2, 2), (3, True, 8, 2, 5), (4, False, 32946, 1, None))):
        img = smooth(5, 65, spp, k) if k % 2 else noise(5, 65, spp, k)
        out["geom_s%d_%s_c%d_p%d_a%d" % (spp, "be" if be else "le", comp, pred, k)] = Case(
            im.write_tiff(img, zlib.compress, rps, pred, comp, be, k), img, True, {})
    # zlib's own strategies on a 36,000-byte strip; level 0 also on a strip over 65,535 bytes (several stored blocks)
    row = wide[:1].copy()
    row[0, 8192] = row[0, 0]   # bytes 32768..32771 repeat bytes 0..3 (far_match below)
    for name, kw in (("stored", dict(level=0)), ("fixed", dict(strategy=zlib.Z_FIXED)), ("rle", dict(strategy=zlib.Z_RLE)),
                     ("huffman_only", dict(strategy=zlib.Z_HUFFMAN_ONLY)), ("level9", dict(level=9))):
        src = smooth(1, 9000, 4, 23) & 0x1f if name in ("rle", "huffman_only") else row   # (zlib stores what Huffman codes alone do not shrink)
        f = im.write_tiff(src, lambda raw, kw=kw: im.compressobj_stream(raw, **kw))
        out["zlib_" + name] = Case(f, src, True, dict(first_byte=im.strips(f)[0][0][2]))
    two = wide[:2].copy()
    out["zlib_stored_72000"] = Case(im.write_tiff(two, lambda raw: im.compressobj_stream(raw, level=0), rows_per_strip=2), two, True, {})
    out["sync_flush"] = Case(im.write_tiff(row, sync_flush_stream), row, True, {})
    out["far_match_32768"] = Case(im.write_tiff(row, far_match_stream), row, True, dict(distance=32768, symbol=im.distance_symbol(32768)))
    for name, (stream, payload, facts) in token_cases().items():
        f, img = _one(stream, payload)
        whole = name not in ("over_long_stream", "trailer_cut_by_one") and not name.startswith("clipped_")   # (libtiff wants a whole stream of the strip's size)
        out["tok_" + name] = Case(f, img, whole, facts)
    return out


# ---------------------------------------------------------------------------------------------------------------- malformed
BAD_IMG = smooth(2, 20, 3, 1)   # strips of 60 bytes at one row per strip


def _good(raw):
    return zlib.compress(raw, 9)


def _dyn(lit_lens, dist_lens, tokens=(), **kw):
    w = im.BitWriter()
    im.dynamic_block(w, None if tokens is None else list(tokens), lit_lens, dist_lens, True, **kw)
    return im.zstream(w.getvalue(), b"")


def bad_streams():
    """name -> (stream for a 60-byte strip, reason class)"""
    raw = im.strip_raws(BAD_IMG, 1, 1)[0]
    good = im.fixed_stream(list(raw))
    lit60 = im.flat_lengths(set(raw) | {256}, 257)
    out = {}
    out["header_fcheck"] = (bytes([0x78, 0x9d]) + good[2:], im.REASON_ZLIB_HEADER)
    out["header_method"] = (im.zstream(good[2:-4], raw, cmf=0x77), im.REASON_ZLIB_HEADER)
    out["header_window"] = (im.zstream(good[2:-4], raw, cmf=0x88), im.REASON_ZLIB_HEADER)
    out["header_fdict"] = (im.zstream(good[2:-4], raw, flg=0x20 + 31 - (0x7820 % 31)), im.REASON_ZLIB_HEADER)
    w = im.BitWriter(); w.bits(1, 1); w.bits(3, 2)
    out["block_type_3"] = (im.zstream(w.getvalue() + raw, raw), im.REASON_BLOCK_HEADER)
    w = im.BitWriter(); im.stored_block(w, raw, True, nlen=0x1234)
    out["stored_lengths"] = (im.zstream(w.getvalue(), raw), im.REASON_BLOCK_HEADER)
    out["too_many_lengths"] = (_dyn(lit60, [0], hlit=30), im.REASON_CODE_LENGTHS)
    out["too_many_distances"] = (_dyn(lit60, [0], hdist=30), im.REASON_CODE_LENGTHS)
    cl = im.flat_lengths({0, 8, 16}, 19)
    out["repeat_with_nothing_before"] = (_dyn(lit60, [0], None, cl_lens=cl, cl_seq=[(16, 0)]), im.REASON_CODE_LENGTHS)
    out["repeat_past_the_end"] = (_dyn([0] * 257, [0], None, cl_lens=cl, cl_seq=[(8, 0)] * 250 + [(16, 3)] * 2), im.REASON_CODE_LENGTHS)
    over = [0] * 19; over[0] = over[8] = over[9] = 1
    out["code_length_code_over_subscribed"] = (_dyn(lit60, [0], None, cl_lens=over, cl_seq=[]), im.REASON_CODE_LENGTHS)
    short = [0] * 19; short[0] = 1; short[8] = 2
    out["code_length_code_incomplete"] = (_dyn(lit60, [0], None, cl_lens=short, cl_seq=[]), im.REASON_CODE_LENGTHS)
    lit = [0] * 257; lit[0] = lit[1] = lit[256] = 1
    out["lengths_over_subscribed"] = (_dyn(lit, [0], None), im.REASON_CODE_LENGTHS)
    lit = [0] * 257
    for sym in (0, 1, 2, 3, 4, 5, 256):   # seven of the eight 3-bit codes
        lit[sym] = 3
    out["lengths_one_code_short"] = (_dyn(lit, [0], None), im.REASON_CODE_LENGTHS)
    out["distances_2_2"] = (_dyn(lit60, [2, 2], None), im.REASON_CODE_LENGTHS)
    out["distances_over_subscribed"] = (_dyn(lit60, [1, 1, 1], None), im.REASON_CODE_LENGTHS)
    lit = im.flat_lengths(range(4), 257)
    out["no_end_of_block_code"] = (_dyn(lit, [0], None), im.REASON_CODE_LENGTHS)
    w = im.BitWriter(); im.fixed_block(w, list(raw[:30]) + [("lit", 286)], True)
    out["symbol_286"] = (im.zstream(w.getvalue(), raw), im.REASON_INVALID_SYMBOL)
    w = im.BitWriter(); im.fixed_block(w, list(raw[:30]) + [("dist", 5, 30)], True)
    out["distance_symbol_30"] = (im.zstream(w.getvalue(), raw), im.REASON_INVALID_SYMBOL)
    w = im.BitWriter(); im.fixed_block(w, list(raw[:30]) + [(5, 31)] + list(raw[35:]), True)
    out["distance_too_far_back"] = (im.zstream(w.getvalue(), raw), im.REASON_FAR_BACK)
    out["trailer_bit_flipped"] = (good[:-1] + bytes([good[-1] ^ 0x10]), im.REASON_DATA_CHECK)
    out["ten_bytes_short"] = (im.fixed_stream(list(raw[:50])), im.REASON_OK)
    return out


def _bad_file(stream, strip):
    return im.write_tiff(BAD_IMG, _good, streams={strip: stream})


def malformed():
    out = {name: Bad(_bad_file(s, k % 2), k % 2, reason) for k, (name, (s, reason)) in enumerate(sorted(bad_streams().items()))}
    return out


def flip_streams():
    """(the 90 bytes, a dynamic stream, a fixed stream of them), each stream of at most 160 bytes"""
    toks = [int(v) for v in smooth(1, 30, 3, 5).tobytes()[:40]] + [(12, 30), (5, 1)] + [int(v) for v in smooth(1, 11, 3, 6).tobytes()]
    dyn, _ = im.dynamic_stream(toks)
    return im.expand(toks), dyn, im.fixed_stream(toks)


def every_flip(stream, expect=90):
    """one file: strip s holds `stream` with bit s flipped"""
    n = 8 * len(stream)
    img = np.zeros((n, expect // 3, 3), np.uint8)
    blobs = {}
    for s in range(n):
        b = bytearray(stream)
        b[s >> 3] ^= 1 << (s & 7)
        blobs[s] = bytes(b)
    return im.write_tiff(img, None, streams=blobs)


def every_truncation(stream, expect=90):
    """one file: strip s holds the first s bytes of `stream`"""
    img = np.zeros((len(stream), expect // 3, 3), np.uint8)
    return im.write_tiff(img, None, streams={s: stream[:s] for s in range(len(stream))})


def random_strips(n=200):
    """n strips of random bytes behind a valid zlib header"""
    rnd = np.random.RandomState(2025)
    img = np.zeros((n, 20, 3), np.uint8)
    return im.write_tiff(img, None, streams={s: b"\x78\x9c" + rnd.randint(0, 256, 40 + s % 7).astype(np.uint8).tobytes() for s in range(n)})
