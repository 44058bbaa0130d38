"""A strict reader of the 16-bit RGBA PNG files the renderer writes, written
from the format (PNG specification, second edition; RFC 1950 for the zlib
stream), a reference writer, and a numpy float32 restatement of the device
front end (csrc/png16.hip): what tests/test_png16_format.py and
tests/test_gpu_png16.py compare the device encoder with.

The reader accepts exactly one layout: signature, IHDR (bit depth 16, colour
type 6, no interlace), one IDAT holding one complete zlib stream of
(8 W + 1) H filtered bytes, IEND, nothing else; every chunk CRC is checked;
all five filter types are undone. Anything else raises Png16Error."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"

# the device encoder's case lists (tests/test_gpu_png16.py): the sizes cross
# the 512-position parse segment, the 4096-position chunk and the 16-row band,
# and 4096 x 17 puts the row above beyond the 32 KB window
SIZES = [(1, 1), (2, 1), (3, 17), (31, 16), (64, 15), (333, 33), (511, 17), (513, 16), (4096, 17)]
KINDS = ["flat", "gradient", "grey", "noise", "ramp"]


class Png16Error(ValueError):
    pass


# ------------------------------------------------------------------ reader --
def _chunks(data):
    if data[:8] != SIGNATURE:
        raise Png16Error("signature")
    at, out = 8, []
    while True:
        if at + 12 > len(data):
            raise Png16Error(f"truncated in the chunk at {at}")
        n, = struct.unpack_from(">I", data, at)
        typ = data[at + 4:at + 8]
        if at + 12 + n > len(data):
            raise Png16Error(f"truncated in chunk {typ!r}")
        body = data[at + 8:at + 8 + n]
        crc, = struct.unpack_from(">I", data, at + 8 + n)
        if crc != (zlib.crc32(typ + body) & 0xFFFFFFFF):
            raise Png16Error(f"CRC of chunk {typ!r}")
        out.append((typ, body))
        at += 12 + n
        if typ == b"IEND":
            break
    if at != len(data):
        raise Png16Error(f"{len(data) - at} bytes after IEND")
    return out


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def unfilter(raw, w, h):
    """(8 w + 1) h filtered bytes -> (h, 8 w) image bytes; pixel size 8."""
    rows = np.frombuffer(raw, np.uint8).reshape(h, 8 * w + 1)
    types = rows[:, 0]
    if types.max(initial=0) > 4:
        raise Png16Error(f"filter type {int(types.max())}")
    res = rows[:, 1:].reshape(h, w, 8)
    if np.all(types == 1):  # what the device writes: one cumulative sum per byte lane
        return np.cumsum(res, axis=1, dtype=np.uint8).reshape(h, 8 * w), types
    out = np.zeros((h, w, 8), np.int32)
    zero = np.zeros((w, 8), np.int32)
    for y in range(h):
        t, r = int(types[y]), res[y].astype(np.int32)
        up = out[y - 1] if y else zero
        if t == 0:
            out[y] = r
        elif t == 1:
            out[y] = np.cumsum(r, axis=0) & 255
        elif t == 2:
            out[y] = (r + up) & 255
        else:
            left = np.zeros(8, np.int32)
            upleft = np.zeros(8, np.int32)
            for x in range(w):
                pred = (left + up[x]) >> 1 if t == 3 else _paeth(left, up[x], upleft)
                left = (r[x] + pred) & 255
                out[y, x] = left
                upleft = up[x]
    return out.astype(np.uint8).reshape(h, 8 * w), types


def read_png16(data):
    """-> (pixels (H, W, 4) uint16, info dict). Raises Png16Error on any deviation."""
    ch = _chunks(bytes(data))
    if [t for t, _ in ch] != [b"IHDR", b"IDAT", b"IEND"]:
        raise Png16Error(f"chunks {[t for t, _ in ch]}")
    if len(ch[0][1]) != 13 or len(ch[2][1]) != 0:
        raise Png16Error("IHDR / IEND length")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", ch[0][1])
    if w == 0 or h == 0 or (depth, colour, comp, filt, lace) != (16, 6, 0, 0, 0):
        raise Png16Error(f"IHDR {(w, h, depth, colour, comp, filt, lace)}")
    z = ch[1][1]
    if len(z) < 6 or (z[0] & 0x0F) != 8 or (z[0] >> 4) > 7 or ((z[0] << 8) | z[1]) % 31 or (z[1] & 0x20):
        raise Png16Error("zlib header")
    d = zlib.decompressobj()
    try:
        raw = d.decompress(z)
    except zlib.error as e:  # damaged deflate data, or a wrong Adler-32
        raise Png16Error(f"zlib: {e}") from None
    if not d.eof:
        raise Png16Error("zlib stream truncated")
    if d.unused_data:
        raise Png16Error(f"{len(d.unused_data)} bytes after the zlib stream")
    if len(raw) != (8 * w + 1) * h:
        raise Png16Error(f"IDAT inflates to {len(raw)} bytes, expected {(8 * w + 1) * h}")
    img, types = unfilter(raw, w, h)
    px = img.reshape(h, w, 4, 2).astype(np.uint16)
    return (px[..., 0] << 8) | px[..., 1], {"width": w, "height": h, "filters": types, "zlib_bytes": len(z),
                                            "raw": raw}


# ------------------------------------------------------------------ writer --
def image_bytes(px):
    px = np.ascontiguousarray(px, np.uint16)
    h, w = px.shape[:2]
    return np.stack([px >> 8, px & 255], axis=-1).astype(np.uint8).reshape(h, 8 * w)


def filtered_bytes(px, types=None):
    """The filtered scanlines of an (H, W, 4) uint16 image: Sub everywhere (what
    the device writes), or the given filter type per row."""
    b = image_bytes(px).astype(np.int32)
    h, w8 = b.shape
    zero = np.zeros(w8, np.int32)
    rows = []
    for y in range(h):
        t = 1 if types is None else int(types[y])
        cur, up = b[y], (b[y - 1] if y else zero)
        left = np.concatenate([np.zeros(8, np.int32), cur[:-8]])
        upleft = np.concatenate([np.zeros(8, np.int32), up[:-8]])
        pred = [zero, left, up, (left + up) >> 1, _paeth(left, up, upleft)][t]
        rows.append(bytes([t]) + ((cur - pred) & 255).astype(np.uint8).tobytes())
    return b"".join(rows)


def _chunk(typ, body):
    return struct.pack(">I", len(body)) + typ + body + struct.pack(">I", zlib.crc32(typ + body) & 0xFFFFFFFF)


def wrap(w, h, zstream):
    return SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 6, 0, 0, 0)) + _chunk(b"IDAT", zstream) + \
        _chunk(b"IEND", b"")


def write_png16(px, level=1, types=None):
    """Reference writer: Sub filter (or `types`), zlib.compress(..., level)."""
    h, w = np.asarray(px).shape[:2]
    return wrap(w, h, zlib.compress(filtered_bytes(px, types), level))


# ------------------------------------------------- front end, restated --
F32 = np.float32


def quantize16(v):
    """rr_device.h quantize16: 0 for v <= 0, 65535 for v >= 1, else (uint16)(v * 65535 + 0.5), each step in float32."""
    v = np.asarray(v, F32)
    s = v * F32(65535.0)
    q = (s + F32(0.5)).astype(np.int64)
    return np.where(v <= 0, 0, np.where(v >= 1, 65535, q)).astype(np.uint16)


def srgb_oetf16(x, table):
    """rr_device.h srgb_oetf16 over the table rr_debug_srgb16_table returns
    (intervals + 1 floats; the read at x = 1 touches a repeat of the last)."""
    x = np.asarray(x, F32)
    t = np.concatenate([np.asarray(table, F32), np.asarray(table[-1:], F32)])
    n = len(table) - 1
    f = x * F32(n)
    i = f.astype(np.int32)
    fr = f - i.astype(F32)
    d = t[i + 1] - t[i]
    m = d * fr
    return np.where(x <= F32(0.0031308), x * F32(12.92), t[i] + m).astype(F32)


def front_end(rgba, view, exposure_scale=1.0, table=None, inv_spp=1.0):
    """The 16-bit samples k_png16_front forms from film sums `rgba` (H, W, >= 3):
    view 0 Standard (needs `table`), 1 Raw. A = 65535."""
    c = (np.asarray(rgba, F32)[..., :3] * F32(inv_spp)) * F32(exposure_scale)
    v = np.minimum(np.maximum(c, F32(0)), F32(1))
    if view == 0:
        v = srgb_oetf16(v, table)
    elif view != 1:
        raise ValueError("Standard and Raw only: Filmic has no numpy restatement")
    q = quantize16(v)
    return np.concatenate([q, np.full(q.shape[:2] + (1,), 65535, np.uint16)], axis=-1)


def make_image(kind, w, h, seed=0):
    """Float film means (H, W, 4); alpha carries junk the encoder must ignore."""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, 4), F32)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "flat":
        img[..., :3] = (0.25, 0.5, 0.0625)
    elif kind == "gradient":  # from below 0 to above 1 across the image
        img[..., 0] = (xx / max(w - 1, 1)) * 1.2 - 0.1
        img[..., 1] = (yy / max(h - 1, 1)) * 1.2 - 0.1
        img[..., 2] = ((xx + yy) % 64) / 63.0
    elif kind == "grey":
        img[..., :3] = rng.random((h, w, 1), F32) ** 2
    elif kind == "noise":  # around the sRGB knee and out of range too
        img[..., :3] = rng.random((h, w, 3), F32) * 1.1 - 0.05
        img[::2, ::3, :3] *= 0.01
    elif kind == "ramp":  # code (3 pixel + channel) mod 65536 of the Raw view
        k = ((yy * w + xx)[..., None] * 3 + np.arange(3)) % 65536
        img[..., :3] = (k / 65535.0).astype(F32)
    else:
        raise ValueError(kind)
    img[..., 3] = rng.random((h, w), F32) * 2.0 - 0.5
    return img
