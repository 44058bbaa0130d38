"""The JPEG forward transform restated in float64, the rule a file's quantised
coefficients are held to, and the inputs of tests/test_jpeg_format.py and
tests/test_gpu_jpeg_coeffs.py. No test functions; nothing here reads csrc/.

The restatement (expected_transform / expected_coeffs): coordinates clamp to the
last column and row; Y Cb Cr from Kr = 0.299, Kb = 0.114 (JFIF 1.02), no offset
on the chroma, 128 off the luma; chroma the mean of the four clamped pixels of a
2x2 cell; BW files take color_modes.grey8 as their one component; the
orthonormal 8x8 DCT-II; the quotient by the file's own quantiser, unrounded.

The rule (check_coeffs), derived and not measured: with x the float64 quotient
and d its distance to the nearest half-integer, the file holds rint(x) wherever
d > 2^-7 and one of the two neighbouring integers elsewhere. The coders work in
float32: three products a pixel, two 8-term passes over terms of at most 64 and
512 in magnitude, float32 table entries and a multiply by a float32 1 / q; that
stays below about 3e-3 before the division by q >= 1, and 2^-7 doubles it.
Exact ties exist (at quality 100 the DC, (0,4), (4,0) and (4,4) terms are
multiples of 1/8). An input may have at most 5 % of its coefficients in the
band (BAND_CAP), or it proves too little.
"""
import functools
import io

import numpy as np

import color_modes as M
import jpeg_reader as R

BAND = 2.0 ** -7
BAND_CAP = 0.05
BLOCK_MAX_BYTES = 216  # kJpegBlockMaxBytes of csrc/device.hpp, the bound the device buffers are sized by
TABLE_QUALITIES = (1, 2, 10, 25, 49, 50, 51, 75, 90, 95, 99, 100)


# ---------------------------------------------------------- the restatement --
def _clamped(rgba, m):
    h, w = rgba.shape[:2]
    ys = np.minimum(np.arange(-(-h // m) * m), h - 1)
    xs = np.minimum(np.arange(-(-w // m) * m), w - 1)
    return np.asarray(rgba)[ys][:, xs]


def _fdct(plane):
    """(8a, 8b) float64 -> (a, b, 64) DCT-II coefficients, natural order."""
    c = R.dct_matrix()
    a, b = plane.shape[0] // 8, plane.shape[1] // 8
    blk = plane.reshape(a, 8, b, 8).transpose(0, 2, 1, 3)
    return np.einsum("vy,abyx,ux->abvu", c, blk, c).reshape(a, b, 64)


def expected_transform(rgba, grey):
    """The unquantised float64 coefficients per component, (blocks_y, blocks_x, 64)."""
    if grey:
        return [_fdct(M.grey8(_clamped(rgba, 8)).astype(np.float64) - 128.0)]
    p = _clamped(rgba, 16)[..., :3].astype(np.float64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    kr, kb = 0.299, 0.114
    y = kr * r + (1.0 - kr - kb) * g + kb * b
    cb, cr = (b - y) / (2.0 - 2.0 * kb), (r - y) / (2.0 - 2.0 * kr)
    h, w = y.shape
    mean4 = lambda c: c.reshape(h // 2, 2, w // 2, 2).mean(axis=(1, 3))  # noqa: E731
    return [_fdct(y - 128.0), _fdct(mean4(cb)), _fdct(mean4(cr))]


@functools.lru_cache(maxsize=None)
def pil_file(quality, grey, optimize=False):
    """A small file PIL (libjpeg) writes at `quality`: where the independent tables come from."""
    from PIL import Image
    a = np.arange(16 * 16 * 3, dtype=np.uint32).reshape(16, 16, 3) * 2654435761 >> 24
    im = Image.fromarray(a.astype(np.uint8), "RGB")
    b = io.BytesIO()
    if grey:
        im.convert("L").save(b, "JPEG", quality=quality, optimize=optimize)
    else:
        im.save(b, "JPEG", quality=quality, subsampling=2, optimize=optimize)
    return b.getvalue()


def expected_coeffs(rgba, quality, grey, jpeg=None):
    """x per component: expected_transform over the quantisers `jpeg`'s own DQT
    names (a jpeg_reader.Jpeg), or, without a file, over libjpeg's at `quality`."""
    j = jpeg if jpeg is not None else R.read_jpeg(pil_file(quality, grey))
    return [f / j.quantiser(ci).astype(np.float64) for ci, f in enumerate(expected_transform(rgba, grey))]


def in_band(x):
    return np.abs(np.abs(x - np.floor(x)) - 0.5) <= BAND


def band_share(xs):
    return sum(int(in_band(x).sum()) for x in xs) / sum(x.size for x in xs)


def check_coeffs(jpeg, xs, what=""):
    """The rule. Raises AssertionError naming the first coefficients that break it."""
    bad = []
    for ci, x in enumerate(xs):
        got = jpeg.coeffs[ci]
        assert got.shape == x.shape, (what, ci, got.shape, x.shape)
        lo = np.floor(x)
        ok = np.where(in_band(x), (got == lo) | (got == lo + 1), got == np.rint(x))
        for by, bx, k in np.argwhere(~ok)[:8]:
            bad.append(f"component {ci} block ({by}, {bx}) coefficient ({k // 8}, {k % 8}): "
                       f"file {got[by, bx, k]}, float64 {x[by, bx, k]:.6f}")
    assert not bad, f"{what}: " + "; ".join(bad)


# ------------------------------------------------- what a file's symbols reach --
def coverage(jpeg):
    """Per component: DC and AC categories, zero runs before a non-zero coefficient
    (ZRLs folded in), the longest ZRL chain, blocks without EOB / of EOB only;
    plus the largest coded block in bits and, per 32-bit word of an interval,
    the most blocks that start in it and whether a block of more than 32 bits
    starts off a word boundary."""
    out = {"max_block_bits": max(int(b.max()) for b in jpeg.block_bits), "comp": []}
    for ci, rows in enumerate(jpeg.symbols):
        c = {"dc": set(), "ac": set(), "runs": set(), "zrl_chain": 0, "no_eob": 0, "eob_only": 0, "neg_bits": set()}
        for by, row in enumerate(rows):
            for bx, syms in enumerate(row):
                c["dc"].add(syms[0][1])
                ac = syms[1:]
                chain = 0
                for r, s in ac:
                    if (r, s) == (15, 0):
                        chain += 1
                    elif s:
                        c["ac"].add(s)
                        c["runs"].add(16 * chain + r)
                        c["zrl_chain"] = max(c["zrl_chain"], chain)
                        chain = 0
                c["no_eob"] += (0, 0) not in ac
                c["eob_only"] += ac == [(0, 0)]
        v = jpeg.coeffs[ci][..., 1:]
        neg = -v[v < 0]
        c["neg_bits"] = {int(n).bit_length() for n in np.unique(neg)}
        out["comp"].append(c)
    starts, mid = 0, False
    for order in jpeg.block_order:
        at, per_word = 0, {}
        for ci, by, bx in order:
            n = int(jpeg.block_bits[ci][by, bx])
            per_word[at >> 5] = per_word.get(at >> 5, 0) + 1
            mid |= n > 32 and at % 32 != 0
            at += n
        starts = max(starts, max(per_word.values()))
    out["blocks_in_a_word"], out["long_block_mid_word"] = starts, mid
    return out


# ------------------------------------------------------------------ inputs ---
def _hash8(h, w, seed):
    """(h, w, 3) uint8 from an integer hash of (x, y, channel, seed)."""
    y, x, c = np.meshgrid(np.arange(h, dtype=np.uint64), np.arange(w, dtype=np.uint64),
                          np.arange(3, dtype=np.uint64), indexing="ij")
    m = np.uint64(0xFFFFFFFF)
    v = (x * np.uint64(0x9E3779B1) ^ y * np.uint64(0x85EBCA77) ^ c * np.uint64(0xC2B2AE3D) ^ np.uint64(seed)) & m
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(0x2C1B3C6D)) & m
    v ^= v >> np.uint64(12)
    v = (v * np.uint64(0x297A2D39)) & m
    v ^= v >> np.uint64(15)
    return (v >> np.uint64(8) & np.uint64(255)).astype(np.uint8)


def _rgba(rgb):
    a = np.empty(rgb.shape[:2] + (4,), np.uint8)
    a[..., :3] = rgb
    a[..., 3] = 255
    a.setflags(write=False)
    return a


def distinct_image(w, h, seed=7):
    """Every pixel differs from its eight neighbours by at least 33 codes in each
    channel: 64 * ((x + 2 y + channel) mod 4) plus 5 hashed bits."""
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    v = 64 * ((x + 2 * y + c) % 4) + (_hash8(h, w, seed) >> 3)
    return _rgba(v.astype(np.uint8))


def noise_image(w, h, seed):
    return _rgba(_hash8(h, w, seed))


def smooth_hash_image(w, h, seed):
    """A few coded symbols a block: a step every 8 columns and every row, 3 hashed bits on top."""
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    v = (37 * (x // 8) + 11 * y + 50 * c) % 200 + 20 + (_hash8(h, w, seed) >> 5)
    return _rgba(v.astype(np.uint8))


# Synthesised blocks: quantised coefficients by zigzag position (DC 4 in all of
# them, so a block of zeros codes as DC difference 0 + EOB: 6 bits of luma).
_RUNS = (14, 15, 16, 17, 31, 32, 33, 47, 48, 49, 62)  # zeros before the one non-zero coefficient
_TINY = {}
_LONG = [
    {1: -1, 2: -2, 3: -5, 4: -11, 5: -21, 6: 1, 7: 3, 8: 6, 9: -3, 10: 2},  # negative magnitudes of 1 .. 5 bits
    {1: 3, 18: -1, 51: 1},            # runs of 16 and 32 after a coefficient
    {2: -2, 35: 1, 63: -1},           # runs of 32 and 27, coefficient 63: no EOB
    {1: 2, 2: 2, 3: 2, 4: 2, 5: 2, 6: 1, 7: 1, 8: 1, 9: 1, 10: 1, 11: 1, 12: 1, 13: 1, 14: 1},
]
_LONG_CHROMA = [  # the chroma quantisers are 99 from zigzag position 10 on: smaller magnitudes
    {1: -1, 2: -2, 3: -3, 4: 2, 5: -1, 6: 1},
    {1: 3, 18: -1, 51: 1},
    {2: -2, 35: 1, 63: -1},
]
_SINGLE = [{r + 1: (1 if i % 2 else -1)} for i, r in enumerate(_RUNS)]
SYNTH_BLOCKS = _SINGLE + _LONG


def _synth_sequence(blocks=None):
    seq = []
    for i, b in enumerate(blocks or SYNTH_BLOCKS):
        seq += [b] + [_TINY] * (4 + i % 2)
    return seq


def _block_samples(zz, q):
    """Dequantise zigzag coefficients {k: v} (DC 4) with quantiser q (64, natural), float64 IDCT."""
    f = np.zeros(64)
    f[0] = 4
    for k, v in zz.items():
        f[R.ZIGZAG[k]] = v
    c = R.dct_matrix()
    return c.T @ (f * q).reshape(8, 8) @ c


@functools.lru_cache(maxsize=None)
def synth_luma(quality=50):
    """Two block rows of the sequence (the lower one rotated by three blocks),
    R = G = B, so the BW file and the Y of the three-component file carry it."""
    codes = np.arange(256, dtype=np.uint8)
    assert np.array_equal(M.grey8(np.stack([codes] * 3, -1)), codes)  # grey8(v, v, v) == v
    q = R.read_jpeg(pil_file(quality, True)).quantiser(0)
    seq = _synth_sequence()
    rows = [seq, seq[3:] + seq[:3]]
    img = np.concatenate([np.concatenate([_block_samples(b, q) for b in row], axis=1) for row in rows], axis=0)
    v = np.clip(np.rint(img + 128.0), 0, 255).astype(np.uint8)
    return _rgba(np.stack([v] * 3, -1)), [[dict(b) for b in row] for row in rows]


@functools.lru_cache(maxsize=None)
def synth_chroma(quality=50):
    """One MCU row: Y 128, Cb the sequence, Cr the sequence reversed, each chroma
    sample replicated over its 2x2 cell, through the inverse JFIF matrix."""
    q = R.read_jpeg(pil_file(quality, False)).quantiser(1)
    seq = _synth_sequence(_SINGLE + _LONG_CHROMA)
    up = lambda row: np.kron(np.concatenate([_block_samples(b, q) for b in row], axis=1), np.ones((2, 2)))  # noqa: E731
    cb, cr = up(seq), up(seq[::-1])
    kr, kb = 0.299, 0.114
    r = 128.0 + (2.0 - 2.0 * kr) * cr
    b = 128.0 + (2.0 - 2.0 * kb) * cb
    g = (128.0 - kr * r - kb * b) / (1.0 - kr - kb)
    rgb = np.stack([r, g, b], -1)
    assert rgb.min() >= 0 and rgb.max() <= 255
    return _rgba(np.rint(rgb).astype(np.uint8)), [seq, seq[::-1]]


def synth_expected(rows, shape):
    """The chosen quantised coefficients as (blocks_y, blocks_x, 64), natural order."""
    out = np.zeros(shape + (64,), np.int64)
    out[..., 0] = 4
    for by, row in enumerate(rows):
        for bx, b in enumerate(row):
            for k, v in b.items():
                out[by, bx, R.ZIGZAG[k]] = v
    return out


@functools.lru_cache(maxsize=None)
def full_swing():
    """16-pixel-high tiles side by side, 0 / 255 only: stripes and checkers of
    1, 2, 4 and 8 pixels, all-0 / all-255 blocks of 8 and 16, red / blue and
    green / magenta alternations, binary noise."""
    yy, xx = np.mgrid[0:16, 0:16]
    tiles = []
    grey = lambda m: np.stack([m] * 3, -1)  # noqa: E731
    for p in (1, 2, 4, 8):
        tiles += [grey((xx // p) % 2), grey((yy // p) % 2), grey((xx // p + yy // p) % 2)]
    tiles += [grey(np.zeros((16, 16), int)), grey(np.ones((16, 16), int))] * 2
    red, blue, green, magenta = (1, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 1)
    solid = lambda c: np.broadcast_to(np.array(c), (16, 16, 3))  # noqa: E731
    two = lambda m, a, b: np.where(m[..., None] == 0, np.array(a), np.array(b))  # noqa: E731
    tiles += [solid(red), solid(blue), solid(red), solid(green), solid(magenta), solid(green)]
    tiles += [two((xx // 8) % 2, red, blue), two((yy // 8) % 2, green, magenta), two((xx // 2 + yy // 2) % 2, red, blue),
              two((xx // 4) % 2, green, magenta), two((xx // 8 + yy // 8) % 2, blue, red)]
    h = _hash8(16, 64, 11)
    tiles += [grey(h[:, :32, 0] >> 7), h[:, 32:] >> 7]
    return _rgba((np.concatenate(tiles, axis=1) * 255).astype(np.uint8))


RAGGED = (1, 7, 8, 9, 15, 16, 17, 33)
QUALITIES = (1, 49, 50, 51, 100)
# (w, h, seed) of noise_image: found by a search over seeds with the host coder at quality 90, the
# first whose file has an interval ending in a padded 0xFF (BW: interval 2, RGB: interval 1)
PADFF = {"BW": (24, 24, 4), "RGB": (24, 24, 7)}


def padff_image(mode):
    w, h, seed = PADFF[mode]
    return noise_image(w, h, seed)


def padded_ff_intervals(data, jpeg):
    """Intervals whose last byte carries padding and is 0xFF, stuffed in front of
    the RSTn / EOI: FF 00 FF Dn in the file's bytes."""
    hits = [i for i, iv in enumerate(jpeg.intervals) if iv["pad_bits"] > 0 and iv["last_byte"] == 0xFF]
    n = sum(data[k:k + 3] == b"\xff\x00\xff" and 0xD0 <= data[k + 3] <= 0xD9 for k in range(len(data) - 3))
    return hits, n


# (id, mode, quality, image builder): every input of both test files but the
# synthesised, full-swing and padded-0xFF ones, which carry coverage conditions.
def plain_cases():
    out = []
    for q in QUALITIES:
        for mode in ("BW", "RGB"):
            out.append((f"quality{q}-{mode}", mode, q, functools.partial(noise_image, 37, 29, 100 + q)))
    for w in RAGGED:
        for h in RAGGED:
            for mode in ("BW", "RGB"):
                out.append((f"ragged{w}x{h}-{mode}", mode, 90, functools.partial(distinct_image, w, h)))
    out.append(("rows257-BW", "BW", 90, functools.partial(distinct_image, 8, 2056)))
    out.append(("rows257-RGB", "RGB", 90, functools.partial(distinct_image, 16, 4112)))
    # row 257 is the first whose sum over the earlier rows takes a thread round the stride a second time
    out.append(("rows258-BW", "BW", 90, functools.partial(distinct_image, 8, 2064)))
    out.append(("rows258-RGB", "RGB", 90, functools.partial(distinct_image, 16, 4128)))
    for h in (1, 9):
        for mode in ("BW", "RGB"):
            out.append((f"wide65535x{h}-{mode}", mode, 50, functools.partial(smooth_hash_image, 65535, h, 5)))
    return out


def expected_header(jpeg, w, h, grey):
    """The header fields of a file of ours."""
    assert (jpeg.width, jpeg.height, jpeg.precision) == (w, h, 8)
    assert jpeg.jfif == (1, 1, 0, 1, 1)
    if grey:
        assert jpeg.components == [(1, 1, 1, 0)] and jpeg.scan == [(1, 0, 0)]
        assert jpeg.dri == (w + 7) // 8 and len(jpeg.intervals) == (h + 7) // 8
    else:
        assert jpeg.components == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
        assert jpeg.scan == [(1, 0, 0), (2, 1, 1), (3, 1, 1)]
        assert jpeg.dri == (w + 15) // 16 and len(jpeg.intervals) == (h + 15) // 16


# ------------------------------------------- the checks both test files make --
def verify(data, rgba, quality, mode, what):
    """The reader accepts `data`; header fields; the band cap on the input; the
    rule; the block bound. -> (Jpeg, coverage, band share)."""
    grey = mode == "BW"
    j = R.read_jpeg(data)
    h, w = rgba.shape[:2]
    expected_header(j, w, h, grey)
    xs = expected_coeffs(rgba, quality, grey, j)
    share = band_share(xs)
    assert share <= BAND_CAP, f"{what}: {share:.2%} of the coefficients within 2^-7 of a tie: the input proves too little"
    check_coeffs(j, xs, what)
    cov = coverage(j)
    assert cov["max_block_bits"] <= 8 * BLOCK_MAX_BYTES, (what, cov["max_block_bits"])
    print(f"{what}: {len(data)} bytes, band share {share:.3%}, largest block {(cov['max_block_bits'] + 7) // 8} bytes")
    return j, cov, share


def check_synth_luma(j, cov, rows, what):
    """The luma of the file is the chosen coefficients exactly, and the symbol
    stream holds what the blocks were built for."""
    assert np.array_equal(j.coeffs[0], synth_expected(rows, j.coeffs[0].shape[:2])), what
    c = cov["comp"][0]
    assert set(_RUNS) <= c["runs"], (what, sorted(c["runs"]))
    assert c["zrl_chain"] == 3 and c["no_eob"] >= 2 and c["eob_only"] >= 3 * len(SYNTH_BLOCKS), (what, c)
    assert {1, 2, 3, 4, 5} <= c["neg_bits"], (what, c["neg_bits"])
    assert cov["blocks_in_a_word"] >= 3 and cov["long_block_mid_word"], (what, cov)
    for ci in range(1, len(j.coeffs)):  # R = G = B: no chroma
        assert not j.coeffs[ci].any(), (what, ci)


def check_synth_chroma(j, cov, rows, what):
    for ci in (1, 2):
        assert np.array_equal(j.coeffs[ci], synth_expected([rows[ci - 1]], j.coeffs[ci].shape[:2])), (what, ci)
        c = cov["comp"][ci]
        assert c["zrl_chain"] >= 2 and set(_RUNS) <= c["runs"], (what, ci, c)  # the chroma AC table's ZRL chains
        assert c["no_eob"] >= 2 and {1, 2} <= c["neg_bits"], (what, ci, c)
    assert cov["blocks_in_a_word"] >= 3 and cov["long_block_mid_word"], (what, cov)


def check_full_swing(cov, what):
    for c in cov["comp"]:
        assert 11 in c["dc"] and 10 in c["ac"], (what, sorted(c["dc"]), sorted(c["ac"]))


def check_padded_ff(data, j, what):
    hits, n = padded_ff_intervals(data, j)
    assert hits and n >= len(hits), (what, hits, n, j.intervals)
    for i in hits:
        assert j.intervals[i]["stuffed"] >= 1
