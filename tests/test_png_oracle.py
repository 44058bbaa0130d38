"""Pins oracle/png_oracle.py before tests/test_gpu_png_tokens.py trusts it as
the device PNG encoder's checker, and proves on the CPU that every crafted
input of oracle/png_cases.py reaches the edge its GPU test is about (a GPU test
must not pass because its input missed the edge): the inflate against zlib's on
stored, fixed and dynamic blocks; hand-corrupted streams rejected; the greedy
reference against a quadratic restatement of its definition; the preconditions
of the length sweep, the two code-depth limits, the distance sweep, the far
threshold, the mixed file and the stored pieces."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

from oracle import png_cases as C
from oracle import png_oracle as P


def _data(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "text":
        words = [b"render", b"frame", b"tile", b"band", b"the", b"of", b"a", b"png", b"deflate", b"\n"]
        return b" ".join(words[i] for i in rng.integers(0, len(words), n // 4))[:n]
    return bytes(n)


def _streams(data):
    for level in (0, 1, 6, 9):
        yield f"level{level}", zlib.compress(data, level)
    for name, strategy in (("fixed", zlib.Z_FIXED), ("huffman", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)):
        c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, strategy)
        yield name, c.compress(data) + c.flush()


# ------------------------------------------------------ the inflate ------
def test_inflate_equals_zlib_on_every_block_type():
    types = set()
    for kind, (name, stream) in ((k, s) for k in ("noise", "text", "zero") for s in _streams(_data(k, 70000))):
        data = _data(kind, 70000)
        blocks = P.inflate_blocks(stream, strict=False)  # zlib may leave a one-code distance alphabet incomplete
        assert b"".join(b["data"] for b in blocks) == zlib.decompress(stream) == data, name
        out = bytearray()
        for b in blocks:
            out += P.expand(b["tokens"], bytes(out)) if b["btype"] else b["data"]
            types.add(b["btype"])
            assert b["start_bit"] < b["end_bit"]
        assert bytes(out) == data, name
        assert [b["bfinal"] for b in blocks] == [0] * (len(blocks) - 1) + [1]
    assert types == {0, 1, 2}


def test_checksums_equal_zlibs():
    for n in (0, 1, 5000, 70000):
        d = _data("noise", n, 3)
        assert P.crc32(d) == zlib.crc32(d) and P.adler32(d) == zlib.adler32(d)


def _png(f, W, H, level=6):
    def chunk(kind, body):
        return len(body).to_bytes(4, "big") + kind + body + zlib.crc32(kind + body).to_bytes(4, "big")
    ihdr = W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([8, 6, 0, 0, 0])
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(f.tobytes(), level))
            + chunk(b"IEND", b""))


def test_parse_png_and_sub_filter_agree_with_an_independent_decoder():
    rng = np.random.default_rng(4)
    W, H = 23, 7
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    f = P.sub_filter(img)
    assert f.shape == (H, 4 * W + 1) and (f[:, 0] == 1).all()
    data = _png(f, W, H)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGBA")), img)
    w, h, stream = P.parse_png(data)
    assert (w, h) == (W, H) and zlib.decompress(stream) == f.tobytes()
    assert np.array_equal(P.image_from_filtered(f, W, H), img)
    g = rng.integers(0, 256, (H, 4 * W + 1), dtype=np.uint8)
    g[:, 0] = 1
    assert np.array_equal(P.sub_filter(P.image_from_filtered(g, W, H)), g)
    bad = bytearray(data)
    bad[-20] ^= 1  # inside the IDAT body
    with pytest.raises(P.PngError, match="CRC"):
        P.parse_png(bytes(bad))
    with pytest.raises(P.PngError, match="signature"):
        P.parse_png(b"\x88" + data[1:])


# ------------------------------------------- corrupted streams ------
def _bits(stream):
    return np.unpackbits(np.frombuffer(stream, np.uint8), bitorder="little")


def _with_bits(stream, at, value, n):
    b = _bits(stream).copy()
    b[at:at + n] = [(value >> k) & 1 for k in range(n)]
    return np.packbits(b, bitorder="little").tobytes()


def _dynamic_stream():
    stream = zlib.compress(_data("text", 6000, 1), 6)
    blk = P.inflate_blocks(stream, strict=False)[0]
    assert blk["btype"] == 2
    return stream, blk


def _cl_entry(blk, want):
    """(bit offset, symbol) of a 3-bit code-length entry whose value is want."""
    for k in range(blk["hclen"]):
        if blk["cl_lens"][P.CL_ORDER[k]] == want:
            return blk["start_bit"] + 17 + 3 * k, P.CL_ORDER[k]
    raise AssertionError(f"no code-length entry of {want}")


def test_over_subscribed_and_incomplete_codes_are_rejected():
    stream, blk = _dynamic_stream()
    longest = max(blk["cl_lens"])
    at, _ = _cl_entry(blk, longest)
    with pytest.raises(P.PngError, match="over-subscribed"):
        P.inflate_blocks(_with_bits(stream, at, longest - 1, 3), strict=False)
    at, _ = _cl_entry(blk, 0)
    with pytest.raises(P.PngError, match="over-subscribed"):
        P.inflate_blocks(_with_bits(stream, at, 1, 3), strict=False)
    at, _ = _cl_entry(blk, longest)
    with pytest.raises(P.PngError, match="incomplete"):
        P.inflate_blocks(_with_bits(stream, at, 0, 3), strict=False)
    assert zlib.decompress(stream)  # the unchanged stream is sound
    for broken in (_with_bits(stream, at, 0, 3), _with_bits(stream, at, longest - 1, 3)):
        with pytest.raises(zlib.error):
            zlib.decompress(broken)


def test_strict_mode_rejects_a_distance_alphabet_of_less_than_two_codes():
    """RFC 1951 lets a distance alphabet with one code (or none) stay incomplete,
    and some zlib builds write that; the device encoder never does."""
    for lens in ([1] + [0] * 29, [0] * 30):
        table, _ = P._decode_table(lens, "distance", strict=False)
        assert -1 in table
        with pytest.raises(P.PngError, match="incomplete"):
            P._decode_table(lens, "distance", strict=True)
        with pytest.raises(P.PngError, match="incomplete"):
            P._decode_table(lens, "literal/length", strict=False)
    with pytest.raises(P.PngError, match="incomplete"):
        P._decode_table([1, 2] + [0] * 28, "distance", strict=False)


def test_stored_block_with_flipped_nlen_is_rejected():
    data = _data("noise", 1000, 5)
    stream = bytearray(zlib.compress(data, 0))
    assert P.inflate_blocks(bytes(stream))[0]["btype"] == 0
    stream[5] ^= 0x10  # 78 01 | 00 | LEN lo hi | NLEN lo hi
    with pytest.raises(P.PngError, match="NLEN"):
        P.inflate_blocks(bytes(stream))


def test_wrong_adler_and_early_distance_are_rejected():
    data = _data("text", 3000, 6)
    stream = bytearray(zlib.compress(data, 6))
    stream[-1] ^= 1
    with pytest.raises(P.PngError, match="Adler"):
        P.inflate_blocks(bytes(stream), strict=False)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, data[:1500])
    raw = c.compress(data[1500:]) + c.flush()  # reaches into a dictionary the stream does not carry
    body = b"\x78\x01" + raw + zlib.adler32(data[1500:]).to_bytes(4, "big")
    with pytest.raises(P.PngError, match="before the start"):
        P.inflate_blocks(body, strict=False)


def _two_bands(cross):
    """A zlib stream of two 16-row bands at W = 25 (stride 101), each a dynamic
    block behind a sync flush; with cross the second piece was compressed with
    the first band as its dictionary, so its matches reach back into it."""
    W, stride = 25, 101
    a, b = _data("text", 16 * stride, 7), _data("text", 16 * stride, 7)[::-1]
    if cross:
        b = a[:800] + b[800:]
    c1 = zlib.compressobj(6, zlib.DEFLATED, -15)
    p1 = c1.compress(a) + c1.flush(zlib.Z_SYNC_FLUSH)
    c2 = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, a) if cross else \
        zlib.compressobj(6, zlib.DEFLATED, -15)
    p2 = c2.compress(b) + c2.flush()
    return W, 32, b"\x78\x01" + p1 + p2 + zlib.adler32(a + b).to_bytes(4, "big"), a + b


def test_bands_groups_blocks_and_rejects_a_band_crossing_match():
    W, H, stream, data = _two_bands(cross=False)
    blocks = P.inflate_blocks(stream, strict=False)
    assert [b["btype"] for b in blocks] == [2, 0, 2]
    got = P.bands(blocks, W, H)
    assert [b["mode"] for b in got] == ["dynamic", "dynamic"] and b"".join(b["data"] for b in got) == data
    assert got[0]["end_bit"] % 8 == 0 and got[0]["nbytes"] * 8 == got[0]["end_bit"] - 16
    W, H, stream, data = _two_bands(cross=True)
    blocks = P.inflate_blocks(stream, strict=False)  # one stream: the inflate itself has no objection
    assert [b["btype"] for b in blocks] == [2, 0, 2] and b"".join(b["data"] for b in blocks) == data
    with pytest.raises(P.PngError, match="before its band"):
        P.bands(blocks, W, H)
    with pytest.raises(P.PngError):  # band sizes that do not fit the blocks
        P.bands(blocks, W + 1, H)


def test_bands_checks_stored_pieces_and_bfinal():
    W, H = 1092, 16  # 69,904 bytes = 65,535 + 4,369
    data = _data("noise", (4 * W + 1) * H, 8)
    stream = b"\x78\x01"
    for at, final in ((0, 0), (65535, 1)):
        piece = data[at:at + 65535]
        stream += bytes([final]) + len(piece).to_bytes(2, "little") + (len(piece) ^ 0xFFFF).to_bytes(2, "little") + piece
    stream += zlib.adler32(data).to_bytes(4, "big")
    assert zlib.decompress(stream) == data
    blocks = P.inflate_blocks(stream)
    got = P.bands(blocks, W, H)
    assert got[0]["mode"] == "stored" and [len(b["data"]) for b in got[0]["blocks"]] == [65535, 4369]
    assert got[0]["nbytes"] == P.stored_bytes(len(data)) == len(data) + 10
    blocks[0]["bfinal"] = 1
    with pytest.raises(P.PngError, match="BFINAL"):
        P.bands(blocks, W, H)


# --------------------------------------------- the reference parse ------
def _greedy_by_definition(b, stride):
    """The definition read off directly, a run counted byte by byte."""
    n, toks, i = len(b), [], 0
    while i < n:
        best = (0, 0)
        for d in (1, 4, stride):
            if d > i or (d == stride and stride > 32768):
                continue
            run = 0
            while run < 258 and i + run < n and b[i + run] == b[i + run - d]:
                run += 1
            if run >= (4 if d == stride and stride > 4096 else 3) and run > best[0]:
                best = (run, d)
        if best[0]:
            toks.append(best)
            i += best[0]
        else:
            toks.append(b[i])
            i += 1
    return toks


def _zlib_tokens(data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, 15)
    return [t for b in P.inflate_blocks(c.compress(data) + c.flush(), strict=False) for t in b["tokens"]]


def test_greedy_tokens_equal_the_definition_on_two_symbol_streams():
    rng = np.random.default_rng(9)
    for stride in (5, 9, 13, 37, 101, 301):
        data = bytes(rng.integers(0, 2, 600, dtype=np.uint8) * 7)
        toks = P.greedy_tokens(data, stride)
        assert toks == _greedy_by_definition(data, stride)
        assert P.expand(toks) == data
        assert {t[1] for t in toks if isinstance(t, tuple)} <= {1, 4, stride}
    ztoks = _zlib_tokens(data, 1)
    assert P.expand(ztoks) == data and ztoks != toks  # another valid parse: the comparison tells them apart
    long = bytes(700)
    assert P.greedy_tokens(long, 5) == [0, (258, 1), (258, 1), (183, 1)] == _greedy_by_definition(long, 5)
    for stride, taken in ((4093, True), (4097, False)):  # a 3-byte match at the stride, on both sides of 4096
        x = bytes(rng.integers(0, 256, stride, dtype=np.uint8))
        x = x + x[:3] + bytes([x[3] ^ 1])
        assert ((3, stride) in P.greedy_tokens(x, stride)) == taken and P.greedy_tokens(x, stride) == \
            _greedy_by_definition(x, stride)


def test_symbol_tables_cover_every_length_and_distance():
    for ln in range(3, 259):
        s, nb, x = P.len_symbol(ln)
        assert 257 <= s <= 285 and 0 <= x < 1 << nb and P.LEN_BASE[s - 257] + x == ln and nb == P.LEN_EXTRA[s - 257]
        assert s == 285 or ln < P.LEN_BASE[s - 256]
    assert P.len_symbol(258) == (285, 0, 0) and P.len_symbol(257) == (284, 5, 30) and P.len_symbol(227) == (284, 5, 0)
    for d in range(1, 32769):
        s, nb, x = P.dist_symbol(d)
        assert 0 <= x < 1 << nb and P.DIST_BASE[s] + x == d and nb == P.DIST_EXTRA[s]
    assert P.dist_symbol(32765) == (29, 13, 8188) and P.dist_symbol(5) == (4, 1, 0) and P.dist_symbol(4) == (3, 0, 0)
    # the tables against an independent encoder: zlib's own symbols decode back to the same lengths and distances
    data = _data("text", 40000, 10)
    for t in _zlib_tokens(data, 9):
        if isinstance(t, tuple):
            assert 3 <= t[0] <= 258 and 1 <= t[1] <= 32768
    assert P.expand(_zlib_tokens(data, 9)) == data


def test_huffman_cost_and_depth():
    assert (P.optimal_cost([0, 0]), P.unlimited_depth([0, 0])) == (0, 0)
    assert (P.optimal_cost([0, 7]), P.unlimited_depth([0, 7])) == (7, 1)
    assert (P.optimal_cost([1, 1, 2, 4]), P.unlimited_depth([1, 1, 2, 4])) == (3 + 3 + 4 + 4, 3)
    fib = [1, 1, 2, 3, 5, 8, 13, 21, 34]
    assert P.unlimited_depth(fib) == 8 and P.unlimited_depth([1] * 16) == 4
    rng = np.random.default_rng(11)
    for _ in range(20):  # Kraft-complete, and no dearer than zlib's code for the same counts
        f = rng.integers(0, 50, 40).tolist()
        lens = P.huffman_lengths(f)
        assert sum(2.0 ** -l for l in lens if l) == 1.0 and all((l > 0) == (c > 0) for l, c in zip(lens, f))
        assert sum(c * l for c, l in zip(f, lens)) == P.optimal_cost(f)
    data = _data("text", 30000, 12)
    c = zlib.compressobj(9, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
    blk = P.inflate_blocks(c.compress(data) + c.flush(), strict=False)
    assert len(blk) == 1 and blk[0]["btype"] == 2
    ll, _, _ = P.token_histograms(blk[0]["tokens"])
    assert sum(f * l for f, l in zip(ll, blk[0]["ll_lens"])) == P.optimal_cost(ll)  # zlib's is optimal here too
    assert P.stored_bytes(1) == 6 and P.stored_bytes(65535) == 65540 and P.stored_bytes(65536) == 65546
    toks = [(s, x) for s, x in blk[0]["cl_tokens"]]
    lens = [l for l in blk[0]["ll_lens"][:blk[0]["hlit"]]] + blk[0]["d_lens"][:blk[0]["hdist"]]
    back = []
    for s, x in P.code_length_tokens(lens, []):
        back += [s] if s < 16 else [back[-1]] * (3 + x) if s == 16 else [0] * ((3 if s == 17 else 11) + x)
    assert back == lens and len(toks) > 0


# ------------------------------- preconditions of the crafted inputs ------
def _band_tokens(f):
    """Reference tokens per band of a filtered stream."""
    s = f.shape[1]
    return [P.greedy_tokens(f[r:r + P.BAND_ROWS].tobytes(), s) for r in range(0, f.shape[0], P.BAND_ROWS)]


def _matches(toks):
    return [t for t in toks if isinstance(t, tuple)]


def test_every_crafted_stream_is_a_sub_filtered_image():
    for f in (C.length_sweep(), C.ll_limit(), C.cl_limit(), C.far_threshold(1023), C.dist_sweep(48), C.band_rows(33)):
        img = C.image_of(f)
        assert img.dtype == np.uint8 and img.shape == (f.shape[0], (f.shape[1] - 1) // 4, 4)
        assert np.array_equal(P.sub_filter(img), f)


def test_length_sweep_precondition():
    f = C.length_sweep()
    W, H = C.LENGTH_SWEEP_SHAPE
    stride = 4 * W + 1
    assert f.shape == (H, stride) and stride <= P.FAR_STRIDE
    per_band = _band_tokens(f)
    have = {t for toks in per_band for t in _matches(toks)}
    for d in (1, 4, stride):
        assert [ln for ln in range(3, 259) if (ln, d) not in have] == []
    offsets = set()
    for toks in per_band:
        n = stride * P.BAND_ROWS
        assert n > 64 * 512 and n > 16384  # more than 64 parse segments, more than one tile
        pos, seg = 0, 0
        for t in toks:
            while pos >= 512 * seg:  # the first token at or behind a segment's start is where the parse enters it
                offsets.add(pos - 512 * seg)
                seg += 1
            pos += t[0] if isinstance(t, tuple) else 1
    # no single band has 128 segments at a stride <= 4096 (65,488 bytes, 127.9 segments): counted over the three bands
    assert len(offsets) >= 128 and max(offsets) >= 250 and max(offsets) <= 257


def _ref_lengths(toks):
    ll, dd, _ = P.token_histograms(toks)
    ll, dd = P.at_least_two_codes(ll), P.at_least_two_codes(dd)
    return ll, dd, P.huffman_lengths(ll), P.huffman_lengths(dd)


def test_literal_length_limit_precondition():
    f = C.ll_limit()
    assert f.shape[0] == 16
    (toks,) = _band_tokens(f)
    ll, dd, _, _ = _ref_lengths(toks)
    assert P.unlimited_depth(ll) > 15
    assert P.dynamic_lower_bound_bits(toks) < 4 * P.stored_bytes(f.size)  # far from the stored form: a dynamic band


def test_code_length_limit_precondition():
    f = C.cl_limit()
    assert f.shape == (16, 1201)
    (toks,) = _band_tokens(f)
    ll, dd, ll_lens, d_lens = _ref_lengths(toks)
    assert max(ll_lens) <= 15 and max(d_lens) <= 15  # the limit of 15 does not bind: the lengths are what is emitted
    cl = P.symbol_counts([s for s, _ in P.code_length_tokens(ll_lens, d_lens)], 19)
    assert P.unlimited_depth(cl) > 7
    assert P.dynamic_lower_bound_bits(toks) < 6 * P.stored_bytes(f.size)


def test_distance_sweep_precondition():
    assert len(C.DIST_SWEEP_WIDTHS) == 48 and C.DIST_SWEEP_WIDTHS[-1] == 8191
    hit = set()
    for W, H in [(W, 3) for W in C.DIST_SWEEP_WIDTHS] + C.DIST_SWEEP_TALL:
        f = C.dist_sweep(W, H)
        stride = 4 * W + 1
        (toks,) = _band_tokens(f)
        far = [t for t in _matches(toks) if t[1] == stride]
        assert far and sum(t[0] for t in far) >= stride, W  # the rows below the first are matches at the stride
        hit.add(P.dist_symbol(stride)[0])
    assert P.dist_symbol(4 * 8191 + 1) == (29, 13, 8188)
    # symbol 5 is the distances 7 and 8: no stride 4W + 1 is either
    assert hit == set(range(4, 30)) - {5}
    f = C.dist_sweep(C.DIST_SWEEP_BEYOND)
    (toks,) = _band_tokens(f)
    assert 4 * C.DIST_SWEEP_BEYOND + 1 > P.WINDOW and {t[1] for t in _matches(toks)} <= {1, 4}


def test_far_threshold_precondition():
    for W, taken in ((1023, True), (1024, False)):
        f = C.far_threshold(W)
        stride = 4 * W + 1
        (toks,) = _band_tokens(f)
        flat = f.reshape(-1)
        spots = [r * stride + c for r in range(1, f.shape[0]) for c in range(8, stride - 40, 40)]
        assert len(spots) > 100
        for p in spots:  # exactly 3 bytes of the row above, not extendable, and no match at 1 or 4
            assert (flat[p:p + 3] == flat[p - stride:p - stride + 3]).all()
            assert flat[p - 1] != flat[p - 1 - stride] and flat[p + 3] != flat[p + 3 - stride]
            assert not (flat[p:p + 3] == flat[p - 1:p + 2]).all() and not (flat[p:p + 3] == flat[p - 4:p - 1]).all()
        starts, pos = {}, 0
        for t in toks:
            starts[pos] = t
            pos += t[0] if isinstance(t, tuple) else 1
        far = [t for t in _matches(toks) if t[1] == stride]
        if taken:
            assert stride == 4093 and all(starts.get(p) == (3, stride) for p in spots)
        else:  # literals where the 3-byte matches were; longer row matches stay
            assert stride == 4097 and all(starts.get(p) == int(flat[p]) for p in spots)
            assert far and min(t[0] for t in far) >= 4
        assert P.dynamic_lower_bound_bits(toks) < 4 * P.stored_bytes(f.size)  # compressible: a dynamic band


def test_mixed_and_stored_piece_preconditions():
    img = C.mixed()
    f = P.sub_filter(img)
    want = []
    for toks, r in zip(_band_tokens(f), range(0, 53, 16)):
        n = f[r:r + 16].size
        want.append(P.dynamic_lower_bound_bits(toks) >= 8 * P.stored_bytes(n))
    assert want == [True, False, True, False]  # noise must be stored; flat and gradient are far below
    for H, pieces in ((15, 1), (16, 2)):
        f = P.sub_filter(C.kind_image("noise4", 1092, H, 1))
        assert (f.size == 65535) == (H == 15) and P.stored_bytes(f.size) == f.size + 5 * pieces
        (toks,) = _band_tokens(f)
        assert P.dynamic_lower_bound_bits(toks) >= 8 * P.stored_bytes(f.size)


def test_band_rows_make_a_match_into_the_previous_band_attractive():
    f = C.band_rows(33)
    stride = f.shape[1]
    whole = P.greedy_tokens(f.tobytes(), stride)  # parsed as one piece, the rows below 16 and 32 match upwards
    pos, crossing = 0, 0
    for t in whole:
        if isinstance(t, tuple):
            crossing += (pos // stride) % 16 == 0 and t[1] == stride
            pos += t[0]
        else:
            pos += 1
    assert crossing >= 2
    for toks in _band_tokens(f):
        assert any(t[1] == stride for t in _matches(toks)) or len(toks) <= stride
