"""The device PNG encoder (png.hip, deflate.hip) against oracle/png_oracle.py, token for
token and code for code. For every band of every case: the file passes the
strict inflate and the container checks (complete codes, no match before its
band, byte-aligned bands, BFINAL last only); a dynamic band's tokens equal the
serial greedy reference of that band's filtered bytes exactly, a stored band's
bytes equal them; the emitted Huffman lengths keep their limits (15 / 15 / 7),
never give a rarer symbol the shorter code and cost what an optimal code costs
whenever the limit does not bind; no band is larger than its stored form, a
dynamic one is smaller, and a band no dynamic block could shrink is stored.
tests/test_png_oracle.py proves on the CPU that each crafted input reaches the
edge it is here for."""
import numpy as np
import pytest

from oracle import png_cases as C
from oracle import png_oracle as P

pytestmark = pytest.mark.gpu

LIMITS = (15, 15, 7)  # literal/length, distance, code-length alphabet


def _emitted_codes(blk):
    """(counts of what the block's stream uses, emitted lengths) per alphabet."""
    ll, dd, _ = P.token_histograms(blk["tokens"])
    cl = P.symbol_counts([s for s, _ in blk["cl_tokens"]], 19)
    return [(ll, blk["ll_lens"]), (dd, blk["d_lens"]), (cl, blk["cl_lens"])]


def _check_codes(blk):
    depths = []
    for (freq, lens), limit in zip(_emitted_codes(blk), LIMITS):
        assert max(lens) <= limit
        assert all(l > 0 for f, l in zip(freq, lens) if f)
        used = sorted((f, l) for f, l in zip(freq, lens) if f)
        longest = {}
        for f, l in used:
            longest[f] = max(longest.get(f, 0), l)
        fs = sorted(longest)
        for a, b in zip(fs, fs[1:]):  # a < b: every symbol seen a times has a code no shorter than any seen b times
            assert min(l for f, l in used if f == a) >= longest[b], "a more frequent symbol has the longer code"
        cost = sum(f * l for f, l in zip(freq, lens))
        depth = P.unlimited_depth(freq)
        assert cost >= P.optimal_cost(freq)
        if depth <= limit:
            assert cost == P.optimal_cost(freq)
        depths.append(depth)
    return depths


def _check(ctx, img):
    """Encodes img on the device and checks every band; returns (bands, file bytes)."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape[:2]
    data = ctx.png_device(img)
    w, h, stream = P.parse_png(data)
    assert (w, h) == (W, H)
    got = P.bands(P.inflate_blocks(stream), W, H)
    f = P.sub_filter(img)
    assert np.array_equal(P.image_from_filtered(np.frombuffer(b"".join(b["data"] for b in got), np.uint8), W, H), img)
    for b in got:
        ref = f[b["row0"]:b["row0"] + b["rows"]].tobytes()
        assert b["data"] == ref
        want = P.greedy_tokens(ref, 4 * W + 1)
        sto = P.stored_bytes(b["n"])
        if b["mode"] == "dynamic":
            if b["tokens"] != want:
                k = next(i for i, (x, y) in enumerate(zip(b["tokens"], want)) if x != y)
                raise AssertionError(f"band at row {b['row0']}: token {k} is {b['tokens'][k]}, reference {want[k]}")
            b["depths"] = _check_codes(b["blocks"][0])
            assert b["nbytes"] < sto
            assert P.dynamic_lower_bound_bits(want) < 8 * sto  # else it had to be stored
        else:
            assert b["nbytes"] == sto
            assert all(len(p["data"]) == P.PIECE for p in b["blocks"][:-1])
    return got, data


SMALL = [("noise", 1, 1), ("noise", 8, 8), ("noise", 17, 9), ("flat", 64, 48), ("flat", 1, 300),
         ("gradient", 333, 257), ("sparse", 320, 200)]


@pytest.mark.parametrize("kind,w,h", SMALL)
def test_small_shapes_token_for_token(ctx, kind, w, h):
    got, _ = _check(ctx, C.kind_image(kind, w, h, seed=w * 7 + h))
    assert len(got) == (h + 15) // 16
    if kind != "noise":
        assert all(b["mode"] == "dynamic" for b in got if b["n"] > 200)


@pytest.mark.parametrize("h", [1, 15, 16, 17, 31, 32, 33])
def test_band_row_edges(ctx, h):
    """Rows that repeat the row above: the first row of a band still may not match into the band before."""
    f = C.band_rows(h)
    got, _ = _check(ctx, C.image_of(f))
    assert [b["rows"] for b in got] == [16] * (h // 16) + ([h % 16] if h % 16 else [])
    assert any(b["mode"] == "dynamic" for b in got) or h == 1


def test_length_sweep(ctx):
    """Every length 3..258 at the distances 1, 4 and the stride; most parse segments entered inside a match."""
    f = C.length_sweep()
    got, _ = _check(ctx, C.image_of(f))
    assert all(b["mode"] == "dynamic" for b in got)
    have = {t for b in got for t in b["tokens"] if isinstance(t, tuple)}
    assert all((ln, d) in have for ln in range(3, 259) for d in (1, 4, f.shape[1]))


@pytest.mark.parametrize("w,h", [(w, 3) for w in C.DIST_SWEEP_WIDTHS + [C.DIST_SWEEP_BEYOND]] + C.DIST_SWEEP_TALL)
def test_distance_sweep(ctx, w, h):
    """Identical noise rows: matches at the stride 4W + 1, up to distance 32765 and not beyond the window.
    Three rows of 1 to 3 pixels are too short to pay for a dynamic block's header, so those widths come
    again 16 rows high, where the band is dynamic and the distance code is written."""
    (band,), _ = _check(ctx, C.image_of(C.dist_sweep(w, h)))
    stride = 4 * w + 1
    far = [t for t in band["tokens"] if isinstance(t, tuple) and t[1] == stride] if band["mode"] == "dynamic" else []
    if w == C.DIST_SWEEP_BEYOND:
        assert far == [] and band["mode"] == "stored"
    elif w > 3 or h > 3:
        assert band["mode"] == "dynamic" and sum(t[0] for t in far) >= stride


@pytest.mark.parametrize("w", [1023, 1024])
def test_far_threshold(ctx, w):
    """3-byte matches at the row above are taken at the stride 4093 and not at 4097."""
    (band,), _ = _check(ctx, C.image_of(C.far_threshold(w)))
    assert band["mode"] == "dynamic"
    far3 = sum(1 for t in band["tokens"] if t == (3, 4 * w + 1))
    assert far3 > 100 if w == 1023 else far3 == 0
    assert any(isinstance(t, tuple) and t[1] == 4 * w + 1 and t[0] >= 4 for t in band["tokens"])


def test_literal_length_limit(ctx):
    """A band whose literal/length counts want a code of more than 15 bits."""
    (band,), _ = _check(ctx, C.image_of(C.ll_limit()))
    assert band["mode"] == "dynamic"
    assert band["depths"][0] > 15  # from the decoded tokens: else the input is wrong
    assert max(band["blocks"][0]["ll_lens"]) == 15


def test_code_length_limit(ctx):
    """A band whose code lengths' own counts want a code of more than 7 bits."""
    (band,), _ = _check(ctx, C.image_of(C.cl_limit()))
    assert band["mode"] == "dynamic"
    print("code-length token counts", _emitted_codes(band["blocks"][0])[2][0], "depth", band["depths"][2])
    assert band["depths"][2] > 7  # from the emitted code-length tokens: else the input is wrong
    assert max(band["blocks"][0]["cl_lens"]) == 7


def test_mixed_stored_and_dynamic_bands(ctx):
    img = C.mixed()
    got, data = _check(ctx, img)
    assert [b["mode"] for b in got] == ["stored", "dynamic", "stored", "dynamic"]
    assert [b["n"] for b in got] == [1201 * 16] * 3 + [1201 * 5]
    assert ctx.png_device(img) == data


@pytest.mark.parametrize("h,pieces", [(15, [65535]), (16, [65535, 4369])])
def test_stored_pieces(ctx, h, pieces):
    (band,), _ = _check(ctx, C.kind_image("noise4", 1092, h, seed=1))
    assert band["mode"] == "stored" and [len(p["data"]) for p in band["blocks"]] == pieces
