"""A strict reader of the OpenEXR files the renderer writes, and a reference
writer of the same rules, in numpy + zlib (test code only).

The subset: single-part scanline file, version 2, four HALF channels A, B, G,
R, ZIP compression (zlib over chunks of 16 scanlines), increasing line order.
Layout, all little-endian:
  76 2f 31 01 | 02 00 00 00 | attributes (name\\0 type\\0 size:int32 value) | \\0
  offset table: ceil(H / 16) uint64 absolute offsets
  chunks: y:int32 size:int32 data
A chunk's n = 8 * W * rows bytes go scanline by scanline, within a scanline
channel by channel (A, B, G, R), W halfs each. ZIP: even-indexed bytes to the
first n / 2 positions, odd-indexed bytes behind them; t[i] = t[i] - t[i-1] +
128 (mod 256) for i >= 1; one zlib stream. A chunk whose stream is not smaller
than n carries the n bytes as they are (size == n).

The reader accepts nothing else: any deviation raises ExrError.
"""
import struct
import zlib

import numpy as np

ROWS = 16
MAGIC = bytes([0x76, 0x2F, 0x31, 0x01])
VERSION = bytes([2, 0, 0, 0])
CHANNELS = ("A", "B", "G", "R")


class ExrError(ValueError):
    pass


# ------------------------------------------------------------- the rules ---
def chunk_bytes(px: np.ndarray) -> bytes:
    """(rows, W, 4) uint16 RGBA -> the chunk's uncompressed bytes."""
    planes = px[:, :, [3, 2, 1, 0]].transpose(0, 2, 1)  # rows, (A B G R), W
    return np.ascontiguousarray(planes).astype("<u2").tobytes()


def preprocess(raw: bytes) -> bytes:
    b = np.frombuffer(raw, np.uint8)
    t = np.concatenate([b[0::2], b[1::2]]).astype(np.int32)
    out = t.copy()
    out[1:] = (t[1:] - t[:-1] + 128) & 0xFF
    return out.astype(np.uint8).tobytes()


def unprocess(pre: bytes) -> bytes:
    t = np.frombuffer(pre, np.uint8).astype(np.int64)
    d = t.copy()
    d[1:] -= 128
    t = (np.cumsum(d) & 0xFF).astype(np.uint8)
    half = (len(t) + 1) // 2
    out = np.empty(len(t), np.uint8)
    out[0::2] = t[:half]
    out[1::2] = t[half:]
    return out.tobytes()


def _attr(name: str, typ: str, value: bytes) -> bytes:
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(value)) + value


def header_bytes(w: int, h: int) -> bytes:
    chl = b"".join(c.encode() + b"\0" + struct.pack("<iB3xii", 1, 0, 1, 1) for c in CHANNELS) + b"\0"
    box = struct.pack("<4i", 0, 0, w - 1, h - 1)
    return (MAGIC + VERSION + _attr("channels", "chlist", chl) + _attr("compression", "compression", b"\x03")
            + _attr("dataWindow", "box2i", box) + _attr("displayWindow", "box2i", box)
            + _attr("lineOrder", "lineOrder", b"\x00") + _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
            + _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
            + _attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")


def write_exr(px: np.ndarray, level: int = 1) -> bytes:
    """Reference writer: (H, W, 4) uint16 half bit patterns, RGBA -> file bytes."""
    px = np.asarray(px, np.uint16)
    h, w = px.shape[:2]
    chunks = []
    for y in range(0, h, ROWS):
        raw = chunk_bytes(px[y:y + ROWS])
        z = zlib.compress(preprocess(raw), level)
        chunks.append((y, z if len(z) < len(raw) else raw))
    head = header_bytes(w, h)
    at = len(head) + 8 * len(chunks)
    table = b""
    for _, c in chunks:
        table += struct.pack("<Q", at)
        at += 8 + len(c)
    return head + table + b"".join(struct.pack("<ii", y, len(c)) + c for y, c in chunks)


# ------------------------------------------------------------ the reader ---
def _cstr(data: bytes, at: int):
    end = data.find(b"\0", at)
    if end < 0 or end - at > 255:
        raise ExrError("unterminated string in the header")
    return data[at:end].decode("ascii"), end + 1


def _value(typ: str, v: bytes):
    if typ == "chlist":
        out, at = [], 0
        while True:
            if at >= len(v):
                raise ExrError("channel list without its closing byte")
            if v[at] == 0:
                if at + 1 != len(v):
                    raise ExrError("bytes after the channel list")
                return out
            name, at = _cstr(v, at)
            if at + 16 > len(v):
                raise ExrError("truncated channel entry")
            ptype, plin, r0, r1, r2, xs, ys = struct.unpack_from("<iB3Bii", v, at)
            out.append({"name": name, "pixelType": ptype, "pLinear": plin, "reserved": (r0, r1, r2),
                        "xSampling": xs, "ySampling": ys})
            at += 16
    sizes = {"compression": 1, "lineOrder": 1, "box2i": 16, "float": 4, "v2f": 8}
    if typ not in sizes:
        raise ExrError(f"attribute type {typ!r} is not part of the subset")
    if len(v) != sizes[typ]:
        raise ExrError(f"{typ} of {len(v)} bytes")
    if typ in ("compression", "lineOrder"):
        return v[0]
    if typ == "box2i":
        return struct.unpack("<4i", v)
    if typ == "float":
        return struct.unpack("<f", v)[0]
    return struct.unpack("<2f", v)


def read_exr(data: bytes):
    """-> (pixels (H, W, 4) uint16 half bit patterns in R, G, B, A order,
    header dict, chunk sizes, chunk modes 'zip' / 'raw')."""
    data = bytes(data)
    if data[:4] != MAGIC:
        raise ExrError("bad magic")
    if data[4:8] != VERSION:
        raise ExrError("not a version 2 single-part scanline file")
    header, at = {}, 8
    while True:
        if at >= len(data):
            raise ExrError("truncated header")
        if data[at] == 0:
            at += 1
            break
        name, at = _cstr(data, at)
        typ, at = _cstr(data, at)
        if at + 4 > len(data):
            raise ExrError("truncated header")
        size = struct.unpack_from("<i", data, at)[0]
        at += 4
        if size < 0 or at + size > len(data):
            raise ExrError("truncated header")
        if name in header:
            raise ExrError(f"attribute {name!r} twice")
        header[name] = _value(typ, data[at:at + size])
        at += size
    want = {"channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio",
            "screenWindowCenter", "screenWindowWidth"}
    if set(header) != want:
        raise ExrError(f"attributes {sorted(header)}")
    ch = header["channels"]
    if [c["name"] for c in ch] != list(CHANNELS):
        raise ExrError("channels are not A, B, G, R")
    for c in ch:
        if (c["pixelType"], c["pLinear"], c["reserved"], c["xSampling"], c["ySampling"]) != (1, 0, (0, 0, 0), 1, 1):
            raise ExrError(f"channel {c}")
    if header["compression"] != 3 or header["lineOrder"] != 0:
        raise ExrError("not ZIP / increasing y")
    x0, y0, x1, y1 = header["dataWindow"]
    if (x0, y0) != (0, 0) or x1 < 0 or y1 < 0 or header["displayWindow"] != header["dataWindow"]:
        raise ExrError("windows")
    if (header["pixelAspectRatio"], header["screenWindowCenter"], header["screenWindowWidth"]) != (1.0, (0.0, 0.0),
                                                                                                  1.0):
        raise ExrError("screen window / aspect")
    w, h = x1 + 1, y1 + 1
    nchunks = (h + ROWS - 1) // ROWS
    if at + 8 * nchunks > len(data):
        raise ExrError("truncated offset table")
    offsets = struct.unpack_from(f"<{nchunks}Q", data, at)
    at += 8 * nchunks
    px = np.zeros((h, w, 4), np.uint16)
    sizes, modes = [], []
    for k in range(nchunks):
        if offsets[k] != at:
            raise ExrError(f"offset table entry {k} is {offsets[k]}, the chunk is at {at}")
        if at + 8 > len(data):
            raise ExrError("truncated chunk header")
        y, size = struct.unpack_from("<ii", data, at)
        at += 8
        if y != k * ROWS:
            raise ExrError(f"chunk {k} starts at scanline {y}")
        rows = min(ROWS, h - y)
        n = 8 * w * rows
        if size <= 0 or size > n:
            raise ExrError(f"chunk {k} of {size} bytes, {n} uncompressed")
        if at + size > len(data):
            raise ExrError("truncated chunk")
        body = data[at:at + size]
        at += size
        if size == n:
            raw, mode = body, "raw"
        else:
            d = zlib.decompressobj()
            try:
                pre = d.decompress(body) + d.flush()
            except zlib.error as e:  # a wrong Adler-32 included
                raise ExrError(f"chunk {k}: {e}") from e
            if not d.eof or d.unused_data:
                raise ExrError(f"chunk {k}: not exactly one complete zlib stream")
            if len(pre) != n:
                raise ExrError(f"chunk {k} inflates to {len(pre)} bytes, not {n}")
            raw, mode = unprocess(pre), "zip"
        planes = np.frombuffer(raw, "<u2").reshape(rows, 4, w)
        px[y:y + rows] = planes.transpose(0, 2, 1)[:, :, [3, 2, 1, 0]]
        sizes.append(size)
        modes.append(mode)
    if at != len(data):
        raise ExrError(f"{len(data) - at} bytes after the last chunk")
    return px, header, sizes, modes


# ------------------------------------------------- shared test images ------
# W x H of the device encoder's cases: a last band of one row (5x33); n = 4096,
# one Adler / emit chunk exactly (32x16); one parse tile of 16384 positions and
# just over (128x16, 129x16); 4W = 32768, the window's edge, and the row above
# out of the window (8192x3, 8193x3).
SIZES = [(1, 1), (1, 17), (3, 16), (5, 33), (32, 16), (128, 16), (129, 16), (333, 257), (8192, 3), (8193, 3),
         (4100, 16)]
KINDS = ["flat", "gradient", "grey", "values", "bits"]

VALUES = np.array([
    0.0, -0.0, 1.0, -1.0, 0.1, 1.0 / 3.0, 0.18, 3.14159274,
    1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 1.0 + 2.0 ** -11 - 2.0 ** -20,  # ties at 1
    2049.0, 2051.0, 2049.001, 2050.999, -2049.0, -2051.0,                                                # ties at 2048
    1e-6, 6e-8, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 * 1.0000001, 2.9e-8, 1e-10, 1e-40,   # subnormals
    2.0 ** -14, 2.0 ** -14 - 2.0 ** -26, 2.0 ** -14 - 2.0 ** -25, 6.1e-5, -6.1e-5, 5 * 2.0 ** -25,     # around 2^-14
    65504.0, 65519.9, 65520.0, 65536.0, 1e9, -65504.0, -65519.9, -65520.0, -1e9, 65503.9, 65488.0,    # the clamp
], dtype=np.float32)


def make_image(kind: str, w: int, h: int, seed: int = 0) -> np.ndarray:
    """(H, W, 4) float32 RGBA."""
    rng = np.random.default_rng(seed)
    if kind == "flat":
        a = np.empty((h, w, 4), np.float32)
        a[...] = (0.8, 0.25, 0.05, 1.0)
    elif kind == "gradient":
        y, x = np.mgrid[0:h, 0:w].astype(np.float32)
        a = np.stack([x / max(w - 1, 1), y / max(h - 1, 1), (x + y) * 0.01, np.ones_like(x)], -1)
    elif kind == "grey":
        g = rng.random((h, w), np.float32)
        a = np.stack([g, g, g, np.ones_like(g)], -1)
    elif kind == "noise":  # independent channels (the size comparison of grey)
        a = rng.random((h, w, 4), np.float32)
        a[..., 3] = 1.0
    elif kind == "values":
        a = VALUES[rng.integers(0, len(VALUES), (h, w, 4))]
        flat = a.reshape(-1)
        k = min(len(VALUES), flat.size)
        flat[:k] = VALUES[:k]  # every value at least once where the image has room
    elif kind == "bits":  # every half bit pattern but NaN and infinity
        b = rng.integers(0, 1 << 16, (h, w, 4), dtype=np.uint16)
        b = np.where((b & 0x7C00) == 0x7C00, b & np.uint16(0xBFFF), b).astype(np.uint16)
        a = b.view(np.float16).astype(np.float32)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(a, np.float32)


def expected_halfs(img: np.ndarray) -> np.ndarray:
    return np.clip(img, -65504, 65504).astype(np.float16).view(np.uint16)
