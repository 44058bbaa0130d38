"""Colour modes (rr_set_color_mode: BW, RGB, RGBA) restated for the tests, from
the byte layouts (PNG specification, second edition; OpenEXR file layout) and
the grey rule of include/rr.h. No test functions.

 - grey8 / luma: the Rec.709 rule in numpy float32, one rounded operation a
   step, left to right, as csrc/grey.h computes it;
 - expected_png8 / expected_png16 / expected_exr: the samples each front end
   forms for C in {1, 3, 4} channels;
 - read_png: a strict PNG reader for colour types 0 / 2 / 6 at 8 and 16 bits;
 - read_exr: a strict EXR reader for the channel lists Y, B G R, A B G R, HALF
   and FLOAT.
"""
import struct
import zlib

import numpy as np

import exr_reader as X
import png16_reader as P

F32 = np.float32
BW, RGB, RGBA = 1, 3, 4  # RR_COLOR_*: the channels of the file
MODES = {"BW": BW, "RGB": RGB, "RGBA": RGBA}
COLOUR_TYPE = {1: 0, 3: 2, 4: 6}
EXR_CHANNELS = {1: ["Y"], 3: ["B", "G", "R"], 4: ["A", "B", "G", "R"]}


class FormatError(ValueError):
    pass


# ------------------------------------------------------------ the grey rule --
def luma(r, g, b):
    """0.2126 r + 0.7152 g + 0.0722 b in float32, products first, summed left to right."""
    r, g, b = (np.asarray(v, F32) for v in (r, g, b))
    pr, pg, pb = F32(0.2126) * r, F32(0.7152) * g, F32(0.0722) * b
    return ((pr + pg).astype(F32) + pb).astype(F32)


def grey8(rgba8):
    """(..., >= 3) uint8 -> uint8 grey codes: c * (1/255)f, luma, 0 for l <= 0,
    255 for l > 1 - 0.5/255, else (uint8)(255 l + 0.5)."""
    k = F32(1.0) / F32(255.0)
    c = np.asarray(rgba8)[..., :3].astype(F32) * k
    l = luma(c[..., 0], c[..., 1], c[..., 2])
    top = F32(1.0) - F32(0.5) / F32(255.0)
    q = (F32(255.0) * l + F32(0.5)).astype(F32).astype(np.int64)
    return np.where(l <= 0, 0, np.where(l > top, 255, q)).astype(np.uint8)


def expected_png8(rgba8, c):
    """(H, W, 4) uint8 -> (H, W, c) uint8 as the 8-bit PNG of c channels holds it."""
    rgba8 = np.asarray(rgba8, np.uint8)
    if c == 1:
        return grey8(rgba8)[..., None]
    return rgba8[..., :c].copy()


def display16(rgba, view, exposure_scale=1.0, table=None):
    """The display-referred floats of the 16-bit path: exposure, clamp, view
    transform (0 Standard with `table`, 1 Raw)."""
    v = np.asarray(rgba, F32)[..., :3] * F32(1.0) * F32(exposure_scale)
    v = np.minimum(np.maximum(v, F32(0)), F32(1))
    if view == 0:
        v = P.srgb_oetf16(v, table)
    elif view != 1:
        raise ValueError("Standard and Raw only")
    return v.astype(F32)


def expected_png16(rgba, c, view, exposure_scale=1.0, table=None):
    """(H, W, 4) float means -> (H, W, c) uint16 samples of the 16-bit PNG."""
    d = display16(rgba, view, exposure_scale, table)
    if c == 1:
        return P.quantize16(luma(d[..., 0], d[..., 1], d[..., 2]))[..., None]
    q = P.quantize16(d)
    if c == 3:
        return q
    return np.concatenate([q, np.full(q.shape[:2] + (1,), 65535, np.uint16)], axis=-1)


def exr_means(rgba, c):
    """(H, W, 4) float means -> (H, W, c) float32 in the file's channel order
    (Y; B, G, R; A, B, G, R with A = 1)."""
    a = np.asarray(rgba, F32)
    if c == 1:
        return luma(a[..., 0], a[..., 1], a[..., 2])[..., None]
    if c == 3:
        return a[..., [2, 1, 0]].copy()
    out = a[..., [3, 2, 1, 0]].copy()
    out[..., 0] = 1.0
    return out


def expected_exr(rgba, c, full):
    """The words of the file: uint32 float bits (FLOAT) or uint16 half bits (HALF)."""
    m = exr_means(rgba, c)
    if full:
        return np.ascontiguousarray(m).view(np.uint32)
    with np.errstate(over="ignore"):
        return X.expected_halfs(m)


# ------------------------------------------------------------- PNG reader ---
def read_png(data):
    """-> (samples (H, W, C) uint8 / uint16, info). Signature, IHDR, one IDAT,
    IEND; colour types 0 / 2 / 6 at 8 or 16 bits; one complete zlib stream of
    exactly the image's filtered bytes; filter types 0 and 1 only."""
    try:
        ch = P._chunks(bytes(data))
    except P.Png16Error as e:
        raise FormatError(str(e)) from None
    if [t for t, _ in ch] != [b"IHDR", b"IDAT", b"IEND"]:
        raise FormatError(f"chunks {[t for t, _ in ch]}")
    if len(ch[0][1]) != 13 or len(ch[2][1]) != 0:
        raise FormatError("IHDR / IEND length")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", ch[0][1])
    if w == 0 or h == 0 or depth not in (8, 16) or colour not in (0, 2, 6) or (comp, filt, lace) != (0, 0, 0):
        raise FormatError(f"IHDR {(w, h, depth, colour, comp, filt, lace)}")
    c = {0: 1, 2: 3, 6: 4}[colour]
    z = ch[1][1]
    if len(z) < 6 or (z[0] & 0x0F) != 8 or (z[0] >> 4) > 7 or ((z[0] << 8) | z[1]) % 31 or (z[1] & 0x20):
        raise FormatError("zlib header")
    d = zlib.decompressobj()
    try:
        raw = d.decompress(z)
    except zlib.error as e:
        raise FormatError(f"zlib: {e}") from None
    if not d.eof or d.unused_data:
        raise FormatError("not exactly one complete zlib stream")
    bpp = c * depth // 8
    if len(raw) != (bpp * w + 1) * h:
        raise FormatError(f"IDAT inflates to {len(raw)} bytes, expected {(bpp * w + 1) * h}")
    rows = np.frombuffer(raw, np.uint8).reshape(h, bpp * w + 1)
    types = rows[:, 0]
    if types.max(initial=0) > 1:
        raise FormatError(f"filter type {int(types.max())}")
    res = rows[:, 1:].reshape(h, w, bpp)
    img = np.where((types == 1)[:, None, None], np.cumsum(res, axis=1, dtype=np.uint8), res)
    if depth == 8:
        px = img.reshape(h, w, c)
    else:
        b = img.reshape(h, w, c, 2).astype(np.uint16)
        px = (b[..., 0] << 8) | b[..., 1]
    return px, {"width": w, "height": h, "depth": depth, "colour_type": colour, "channels": c, "filters": types,
                "raw": raw, "zlib_bytes": len(z)}


def png_front_bytes(samples, depth):
    """The Sub-filtered bytes (what the device's front end forms) of (H, W, C) samples."""
    s = np.asarray(samples)
    h, w, c = s.shape
    if depth == 16:
        s = np.stack([s >> 8, s & 255], axis=-1)
    b = s.astype(np.uint8).reshape(h, w, -1).astype(np.int32)
    left = np.concatenate([np.zeros((h, 1, b.shape[2]), np.int32), b[:, :-1]], axis=1)
    body = ((b - left) & 255).astype(np.uint8).reshape(h, -1)
    return np.concatenate([np.ones((h, 1), np.uint8), body], axis=1).tobytes()


# ------------------------------------------------------------- EXR reader ---
def read_exr(data):
    """-> (words (H, W, C) uint16 (HALF) or uint32 (FLOAT) in the file's channel
    order, info). Version 2 single-part scanline file, ZIP, the channel lists Y
    / B G R / A B G R of one pixel type, chunks of 16 scanlines back to back."""
    data = bytes(data)
    if data[:4] != X.MAGIC or data[4:8] != X.VERSION:
        raise FormatError("magic / version")
    header, at = {}, 8
    try:
        while True:
            if at >= len(data):
                raise FormatError("truncated header")
            if data[at] == 0:
                at += 1
                break
            name, at = X._cstr(data, at)
            typ, at = X._cstr(data, at)
            size = struct.unpack_from("<i", data, at)[0]
            at += 4
            if size < 0 or at + size > len(data) or name in header:
                raise FormatError(f"attribute {name!r}")
            header[name] = X._value(typ, data[at:at + size])
            at += size
    except (X.ExrError, struct.error) as e:
        raise FormatError(str(e)) from None
    want = {"channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio",
            "screenWindowCenter", "screenWindowWidth"}
    if set(header) != want:
        raise FormatError(f"attributes {sorted(header)}")
    names = [c["name"] for c in header["channels"]]
    if names not in EXR_CHANNELS.values():
        raise FormatError(f"channels {names}")
    c = len(names)
    ptype = header["channels"][0]["pixelType"]
    if ptype not in (1, 2):
        raise FormatError(f"pixel type {ptype}")
    for e in header["channels"]:
        if (e["pixelType"], e["pLinear"], e["reserved"], e["xSampling"], e["ySampling"]) != (ptype, 0, (0, 0, 0), 1, 1):
            raise FormatError(f"channel {e}")
    if header["compression"] != 3 or header["lineOrder"] != 0:
        raise FormatError("not ZIP / increasing y")
    x0, y0, x1, y1 = header["dataWindow"]
    if (x0, y0) != (0, 0) or x1 < 0 or y1 < 0 or header["displayWindow"] != header["dataWindow"]:
        raise FormatError("windows")
    if (header["pixelAspectRatio"], header["screenWindowCenter"], header["screenWindowWidth"]) != (1.0, (0.0, 0.0), 1.0):
        raise FormatError("screen window / aspect")
    w, h = x1 + 1, y1 + 1
    word = 2 if ptype == 1 else 4
    dt = "<u2" if ptype == 1 else "<u4"
    nchunks = (h + X.ROWS - 1) // X.ROWS
    if at + 8 * nchunks > len(data):
        raise FormatError("truncated offset table")
    offsets = struct.unpack_from(f"<{nchunks}Q", data, at)
    at += 8 * nchunks
    px = np.zeros((h, w, c), np.uint16 if ptype == 1 else np.uint32)
    modes, sizes, ref = [], [], 0
    for k in range(nchunks):
        if offsets[k] != at or at + 8 > len(data):
            raise FormatError(f"chunk {k}: offset {offsets[k]}, at {at}")
        y, size = struct.unpack_from("<ii", data, at)
        at += 8
        rows = min(X.ROWS, h - k * X.ROWS)
        n = word * c * w * rows
        if y != k * X.ROWS or size <= 0 or size > n or at + size > len(data):
            raise FormatError(f"chunk {k}: scanline {y}, {size} bytes of {n}")
        body = data[at:at + size]
        at += size
        if size == n:
            raw, mode = body, "raw"
        else:
            d = zlib.decompressobj()
            try:
                pre = d.decompress(body) + d.flush()
            except zlib.error as e:
                raise FormatError(f"chunk {k}: {e}") from None
            if not d.eof or d.unused_data or len(pre) != n:
                raise FormatError(f"chunk {k}: not one complete zlib stream of {n} bytes")
            raw, mode = X.unprocess(pre), "zip"
        px[y:y + rows] = np.frombuffer(raw, dt).reshape(rows, c, w).transpose(0, 2, 1)
        modes.append(mode)
        sizes.append(size)
        ref += min(n, len(zlib.compress(X.preprocess(raw), 1)))  # what a zlib level 1 writer stores
    if at != len(data):
        raise FormatError(f"{len(data) - at} bytes after the last chunk")
    return px, {"width": w, "height": h, "channels": names, "pixel_type": ptype, "modes": modes,
                "sizes": sizes, "zlib1_file_bytes": len(data) - sum(sizes) + ref}


# ------------------------------------------------------------ test images ---
KINDS = ["flat", "grey", "gradient", "noise"]


def float_image(kind, w, h, seed=0):
    """(H, W, 4) float32 means; values below 0 and above 1 included, alpha junk."""
    return P.make_image(kind, w, h, seed)


def rgba8_image(kind, w, h, seed=0):
    """(H, W, 4) uint8; alpha carries junk the coders must ignore or pass on."""
    rng = np.random.default_rng(seed + 1)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.zeros((h, w, 4), np.uint8)
    if kind == "flat":
        img[..., :3] = (200, 64, 13)
    elif kind == "grey":
        img[..., :3] = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    elif kind == "gradient":
        img[..., 0] = (xx * 255) // max(w - 1, 1)
        img[..., 1] = (yy * 255) // max(h - 1, 1)
        img[..., 2] = (xx + yy) % 256
    elif kind == "noise":
        img[..., :3] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    else:
        raise ValueError(kind)
    img[..., 3] = 255
    return img


def smooth_image(w, h):
    """A smooth colour image with some texture, (H, W, 4) uint8."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros((h, w, 4), np.uint8)
    img[..., 0] = 127 + 100 * np.sin(xx / 9.0) * np.cos(yy / 13.0)
    img[..., 1] = (xx * 255 / max(w - 1, 1)) * 0.6 + (yy * 255 / max(h - 1, 1)) * 0.4
    img[..., 2] = 127 + 90 * np.cos((xx + yy) / 17.0)
    img[..., 3] = 255
    return img


def png_zlib1_file_bytes(data, info):
    """Size of the same PNG with its front-end bytes deflated by zlib level 1."""
    return len(data) - info["zlib_bytes"] + len(zlib.compress(info["raw"], 1))


def psnr(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    m = float(np.mean(d * d))
    return 99.0 if m == 0 else 10.0 * np.log10(255.0 ** 2 / m)
