"""The images of the rr_set_exr_codec tests (test code only): float RGBA means
whose OPEN_EXR words code, go raw, or alternate, and the words a file of them
holds (color_modes.expected_exr: A = 1, as rr_debug_encode_device writes it)."""
import numpy as np

import color_modes as CM
import exr_codecs as E
import exr_reader as X

# W: no run possible or barely (1, 2, 3); the packet caps inside a flat row's byte halves (127, 128,
# 129); the packer's 256-element step and its 3-back / 4-forward window (255, 256, 257, 259); 300.
WIDTHS = [1, 2, 3, 127, 128, 129, 255, 256, 257, 259, 300]
# H: PXR24's band edges and a short last band; 17 rows are enough for the per-row coders.
HEIGHTS = [1, 15, 16, 17, 33]
# every W at H = 17, every H at W = 300, and the smallest
SIZES = [(w, 17) for w in WIDTHS] + [(300, h) for h in HEIGHTS if h != 17] + [(1, 1)]


def noise(w, h, full, seed=0):
    """Means whose words are as good as random. HALF: every half bit pattern but
    NaN and infinity; FLOAT: random float bits with exponents 64 .. 191 (the luma
    of three stays finite)."""
    rng = np.random.default_rng(1000 + seed)
    if not full:
        b = rng.integers(0, 1 << 16, (h, w, 4), dtype=np.uint16)
        b = np.where((b & 0x7C00) == 0x7C00, b & np.uint16(0xBFFF), b).astype(np.uint16)
        return np.ascontiguousarray(b.view(np.float16).astype(np.float32))
    b = rng.integers(0, 1 << 32, (h, w, 4), dtype=np.uint64).astype(np.uint32)
    e = (b >> np.uint32(23)) & np.uint32(0x7F)
    b = (b & np.uint32(0x807FFFFF)) | ((e + np.uint32(64)) << np.uint32(23))
    return np.ascontiguousarray(b.view(np.float32))


def float_edges(w, h, seed=0):
    """FLOAT means that exercise the 24-bit rounding (low bytes 0x7f, 0x80, 0x81, a
    mantissa of all ones, the largest finite float), infinities and a NaN, among flat pixels."""
    vals = np.array([0x3F80007F, 0x3F800080, 0x3F800081, 0x3F7FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000,
                     0x7FC00000, 0x00000001, 0x00800000, 0x3E99997F, 0x00000000, 0x80000000], np.uint32).view(np.float32)
    rng = np.random.default_rng(2000 + seed)
    a = np.full((h, w, 4), 0.25, np.float32)
    pick = rng.random((h, w, 4)) < 0.2
    a[pick] = vals[rng.integers(0, len(vals), int(pick.sum()))]
    return a


def flat(w, h, full):
    """One colour. FLOAT: black, whose words are zero bytes: after the reorder a flat row of
    floats alternates a sample's bytes 0 and 2 (1 and 3), so a colour whose bytes differ
    has no run of three and RLE stores it raw."""
    a = X.make_image("flat", w, h)
    if full:
        a[..., :3] = 0.0
    return a


def image(kind, w, h, full, seed=0):
    """(H, W, 4) float32 means."""
    if kind == "noise":
        return noise(w, h, full, seed)
    if kind == "flat":
        return flat(w, h, full)
    if kind == "alternate":  # even rows flat, odd rows noise
        a = flat(w, h, full)
        a[1::2] = noise(w, h, full, seed)[1::2]
        return a
    if kind == "float_edges":
        return float_edges(w, h, seed)
    return X.make_image(kind, w, h, seed)


def words(kind, w, h, c, full, seed=0):
    with np.errstate(all="ignore"):
        return CM.expected_exr(image(kind, w, h, full, seed), c, full)


def run_row_image():
    """A HALF image of one row whose B, G and R samples are exr_codecs.run_row_words: in
    colour mode BW the luma is not those halfs, so the row is for RGB files, whose three
    planes repeat it."""
    half = E.run_row_words()[0, :, 0]
    v = half.view(np.float16).astype(np.float32)
    a = np.ones((1, len(v), 4), np.float32)
    a[0, :, :3] = v[:, None]
    return a
