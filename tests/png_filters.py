"""PNG's adaptive row filter (rr_set_png_compression) restated for the tests,
from the PNG specification (second edition, section 9) and the selection rule
include/rr.h states. No test functions.

 - rule: the filter type of every row of raw scanlines, in numpy;
 - filter_rows / unfilter_rows: the five filter types, both ways;
 - read_png: a strict reader for colour types 0 / 2 / 6 at 8 and 16 bits that
   accepts all five filter types and returns each row's filter byte and the
   unfiltered scanlines (the chunk and zlib checks are tests/png16_reader.py's);
 - image: the generator the filter tests share;
 - stored_only: whether a zlib stream holds stored blocks only;
 - libpng_filters: the filter bytes of libpng's own file, through ctypes.
"""
import ctypes
import ctypes.util
import struct
import zlib

import numpy as np

import png16_reader as P

NAMES = ["None", "Sub", "Up", "Average", "Paeth"]


class FormatError(ValueError):
    pass


# ---------------------------------------------------------------- the rule --
def _neighbours(raw, bpp):
    """x, a, b, c of every byte of (H, n) raw scanlines, int32."""
    x = np.asarray(raw, np.uint8).astype(np.int32)
    h, n = x.shape
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :n - bpp] if n > bpp else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :n - bpp] if n > bpp else 0
    return x, a, b, c


def paeth(a, b, c):
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def residuals(raw, bpp):
    """(5, H, n) residuals mod 256 of the five types."""
    x, a, b, c = _neighbours(raw, bpp)
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth(a, b, c)]) & 255


def rule(raw, bpp):
    """The type every row takes: the smallest sum of r < 128 ? r : 256 - r, the
    types tried in the order 0 .. 4, a later one only when strictly smaller.
    libpng leaves out the types whose neighbours an image of one row (Up,
    Average, Paeth) or of one pixel's width (Sub, Average, Paeth) lacks; of
    those only Average could have won."""
    r = residuals(raw, bpp)
    score = np.where(r < 128, r, 256 - r).sum(axis=2, dtype=np.int64)  # (5, H)
    best = np.zeros(score.shape[1], np.int64)
    thin = r.shape[1] == 1 or r.shape[2] <= bpp  # one row, or one pixel wide: libpng tries no Average
    for t in range(1, 5):
        if thin and t == 3:
            continue
        best = np.where(score[t] < score[best, np.arange(score.shape[1])], t, best)
    return best.astype(np.uint8)


def filter_rows(raw, bpp, types):
    """The filtered bytes, filter byte in front of every row: (H, n + 1) uint8."""
    r = residuals(raw, bpp)
    types = np.asarray(types, np.int64)
    body = r[types, np.arange(len(types))].astype(np.uint8)
    return np.concatenate([types.astype(np.uint8)[:, None], body], axis=1)


def unfilter_rows(rows, bpp):
    """(H, n + 1) filtered bytes -> ((H, n) raw scanlines, (H,) filter types)."""
    rows = np.asarray(rows, np.uint8)
    types = rows[:, 0]
    if types.max(initial=0) > 4:
        raise FormatError(f"filter type {int(types.max())}")
    h, n = rows.shape[0], rows.shape[1] - 1
    if n % bpp:
        raise FormatError("row is no whole number of pixels")
    res = rows[:, 1:].reshape(h, n // bpp, bpp).astype(np.int32)
    out = np.zeros_like(res)
    zero = np.zeros_like(res[0])
    for y in range(h):
        t, r, up = int(types[y]), res[y], (out[y - 1] if y else zero)
        if t == 0:
            out[y] = r
        elif t == 1:
            out[y] = np.cumsum(r, axis=0) & 255
        elif t == 2:
            out[y] = (r + up) & 255
        else:
            left = np.zeros(bpp, np.int32)
            upleft = np.zeros(bpp, np.int32)
            for x in range(r.shape[0]):
                pred = (left + up[x]) >> 1 if t == 3 else paeth(left, up[x], upleft)
                left = (r[x] + pred) & 255
                out[y, x] = left
                upleft = up[x]
    return out.astype(np.uint8).reshape(h, n), types.copy()


# ------------------------------------------------------------------ reader --
def _idat_stream(data, one_idat):
    try:
        ch = P._chunks(bytes(data))
    except P.Png16Error as e:
        raise FormatError(str(e)) from None
    names = [t for t, _ in ch]
    if one_idat and names != [b"IHDR", b"IDAT", b"IEND"]:
        raise FormatError(f"chunks {names}")
    if names[0] != b"IHDR" or len(ch[0][1]) != 13 or len(ch[-1][1]) != 0:
        raise FormatError("IHDR / IEND")
    return ch[0][1], b"".join(body for t, body in ch if t == b"IDAT")


def read_png(data, one_idat=True):
    """-> (samples (H, W, C) uint8 / uint16, info). Signature, IHDR, one IDAT,
    IEND (one_idat False: any chunks, the IDATs joined: libpng's own files);
    colour types 0 / 2 / 6 at 8 or 16 bits, no interlace; one complete zlib
    stream of exactly the image's filtered bytes; filter types 0 .. 4.
    info: "filters" the rows' filter bytes, "raw" the unfiltered scanlines
    (H, bpp W) uint8, "filtered" the inflated bytes, "zlib" the stream."""
    ihdr, z = _idat_stream(data, one_idat)
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", ihdr)
    if w == 0 or h == 0 or depth not in (8, 16) or colour not in (0, 2, 6) or (comp, filt, lace) != (0, 0, 0):
        raise FormatError(f"IHDR {(w, h, depth, colour, comp, filt, lace)}")
    c = {0: 1, 2: 3, 6: 4}[colour]
    if len(z) < 6 or (z[0] & 0x0F) != 8 or (z[0] >> 4) > 7 or ((z[0] << 8) | z[1]) % 31 or (z[1] & 0x20):
        raise FormatError("zlib header")
    d = zlib.decompressobj()
    try:
        filtered = d.decompress(z)
    except zlib.error as e:
        raise FormatError(f"zlib: {e}") from None
    if not d.eof or d.unused_data:
        raise FormatError("not exactly one complete zlib stream")
    bpp = c * depth // 8
    if len(filtered) != (bpp * w + 1) * h:
        raise FormatError(f"IDAT inflates to {len(filtered)} bytes, expected {(bpp * w + 1) * h}")
    raw, types = unfilter_rows(np.frombuffer(filtered, np.uint8).reshape(h, bpp * w + 1), bpp)
    if depth == 8:
        px = raw.reshape(h, w, c)
    else:
        b = raw.reshape(h, w, c, 2).astype(np.uint16)
        px = (b[..., 0] << 8) | b[..., 1]
    return px, {"width": w, "height": h, "depth": depth, "colour_type": colour, "channels": c, "bpp": bpp,
                "filters": types, "raw": raw, "filtered": filtered, "zlib": z}


def scanlines(samples, depth):
    """(H, W, C) samples -> (H, bpp W) raw scanline bytes (16 bits: big-endian)."""
    s = np.asarray(samples)
    h = s.shape[0]
    if depth == 16:
        s = np.stack([s >> 8, s & 255], axis=-1)
    return s.astype(np.uint8).reshape(h, -1)


def stored_only(z):
    """Whether the deflate data of zlib stream z consists of stored blocks only."""
    at = 2  # stored blocks are byte-aligned: a stream of them only has every header on a byte
    while True:
        if at >= len(z) - 4:
            return False
        head = z[at]
        if head & 0x06:  # BTYPE != 0 (or bits of a compressed block)
            return False
        if at + 5 > len(z):
            return False
        n, nn = struct.unpack_from("<HH", z, at + 1)
        if n ^ nn != 0xFFFF:
            return False
        at += 5 + n
        if head & 1:
            return at == len(z) - 4


# --------------------------------------------------------------- generator --
KINDS = ["noise", "ramp", "ramp+noise", "step"]


def image(w, h, c, seed=0):
    """(H, W, 4) uint8 whose rows mix four contents in stripes (stripe k of
    max(1, H // 8) rows has content (k + seed) mod 4): uniform noise; the ramp
    3x + 5y + 7k of channel k; the ramp plus noise in 0 .. 5; a two-level step.
    Alpha 255. c: the channels of the file the image is meant for (the
    contents are per channel, so every c sees them)."""
    rng = np.random.default_rng(1000 * seed + 10 * w + h + c)
    yy, xx, kk = np.mgrid[0:h, 0:w, 0:4]
    ramp = 3 * xx + 5 * yy + 7 * kk
    contents = [rng.integers(0, 256, (h, w, 4)), ramp, ramp + rng.integers(0, 6, (h, w, 4)),
                np.where((xx // 5 + yy // 3) % 2 == 0, 40 + 20 * kk, 200 - 10 * kk)]
    stripe = np.arange(h) // max(1, h // 8)
    pick = (stripe + seed) % 4
    img = np.zeros((h, w, 4), np.int64)
    for k in range(4):
        img[pick == k] = contents[k][pick == k]
    img = (img & 255).astype(np.uint8)
    img[..., 3] = 255
    return img


def float_image(w, h, seed=0):
    """(H, W, 4) float32 means in [0, 1] with the same mix of contents, for the
    16-bit path (codes of the generator's bytes with a fine ramp added, so both
    bytes of a sample vary)."""
    b = image(w, h, 4, seed).astype(np.float32)
    yy, xx = np.mgrid[0:h, 0:w]
    fine = ((7 * xx + 3 * yy) % 64).astype(np.float32)[..., None] / np.float32(64 * 255)
    out = (b / np.float32(255.0)) * np.float32(0.9) + fine
    out[..., 3] = 1.0
    return out.astype(np.float32)


# ------------------------------------------------------------------ libpng --
class _PngImage(ctypes.Structure):
    _fields_ = [("opaque", ctypes.c_void_p), ("version", ctypes.c_uint32), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("format", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("colormap_entries", ctypes.c_uint32), ("warning_or_error", ctypes.c_uint32),
                ("message", ctypes.c_char * 64)]


_LIBPNG_FORMAT = {1: 0, 3: 2, 4: 3}  # PNG_FORMAT_GRAY, _RGB, _RGBA
_libpng = None


def libpng():
    """libpng16 through ctypes, or None where it does not load."""
    global _libpng
    if _libpng is None:
        name = ctypes.util.find_library("png16")
        try:
            L = ctypes.CDLL(name) if name else False
            if L:
                L.png_image_write_to_memory.restype = ctypes.c_int
                L.png_image_write_to_memory.argtypes = [ctypes.POINTER(_PngImage), ctypes.c_void_p,
                                                        ctypes.POINTER(ctypes.c_size_t), ctypes.c_int, ctypes.c_void_p,
                                                        ctypes.c_int32, ctypes.c_void_p]
        except (OSError, AttributeError):
            L = False
        _libpng = L
    return _libpng or None


def libpng_file(samples):
    """The PNG libpng's simplified API writes of (H, W, C) uint8 samples, default filters."""
    L = libpng()
    s = np.ascontiguousarray(samples, np.uint8)
    h, w, c = s.shape
    im = _PngImage()
    im.version, im.width, im.height, im.format = 1, w, h, _LIBPNG_FORMAT[c]
    buf = ctypes.create_string_buffer(2 * s.size + 65536)
    n = ctypes.c_size_t(len(buf))
    ok = L.png_image_write_to_memory(ctypes.byref(im), buf, ctypes.byref(n), 0, s.ctypes.data_as(ctypes.c_void_p), 0, None)
    if not ok:
        raise RuntimeError(f"libpng: {im.message.decode(errors='replace')}")
    return buf.raw[:n.value]
