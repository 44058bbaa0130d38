"""A strict reader of the OpenEXR files with FLOAT channels the renderer writes
(rr_set_exr_depth 32), and a reference writer of the same rules, in numpy +
zlib (test code only).

The file is exr_reader's but for the channel type: single-part scanline file,
version 2, four FLOAT channels A, B, G, R (pixelType 2), ZIP compression (zlib
over chunks of 16 scanlines), increasing line order, the same eight
attributes. A chunk's n = 16 * W * rows bytes go scanline by scanline, within
a scanline channel by channel (A, B, G, R), W little-endian 32-bit floats
each. ZIP is type-agnostic (exr_reader.preprocess / unprocess): even-indexed
bytes first, odd-indexed behind them, then differences + 128; for floats the
first half alternates bytes 0 and 2 of consecutive samples, the second half
bytes 1 and 3. A chunk whose stream is not smaller than n carries the n bytes
as they are.

The reader accepts nothing else: any deviation raises ExrError. Pixels are
uint32 bit patterns throughout, so NaN payloads, signed zeros and subnormals
compare exactly.
"""
import struct
import zlib

import numpy as np

from exr_reader import (CHANNELS, MAGIC, ROWS, VALUES, VERSION, ExrError, _attr, _cstr, _value, make_image as _make16,
                        preprocess, unprocess)

FLOAT = 2
SIZES = [(1, 1), (1, 17), (3, 16), (5, 33), (16, 16), (64, 16), (65, 16), (333, 257), (4096, 3), (4097, 3),
         (16384, 2), (16385, 2), (1025, 16)]
KINDS = ["flat", "gradient", "grey", "values", "bits", "bits32", "values32"]

_F32 = np.finfo(np.float32)
VALUES32 = np.concatenate([VALUES, np.array([
    _F32.smallest_subnormal, -_F32.smallest_subnormal, 2.0 ** -130, -(2.0 ** -140), _F32.tiny, -_F32.tiny,
    float(np.nextafter(_F32.tiny, np.float32(0), dtype=np.float32)),  # the largest subnormal
    _F32.max, -_F32.max, np.inf, -np.inf,
    65505.0, 65536.0, 70000.0, -70000.0, 131071.0, 1e6, 16777217.0, 3.0e38,  # HALF clamps these to 65504
], dtype=np.float32)])


def make_image(kind: str, w: int, h: int, seed: int = 0) -> np.ndarray:
    """(H, W, 4) float32 RGBA: exr_reader's kinds and two of 32-bit patterns."""
    rng = np.random.default_rng(seed)
    if kind == "bits32":  # uniform 32-bit patterns but NaN; infinities and subnormals stay
        b = rng.integers(0, 1 << 32, (h, w, 4), dtype=np.uint64).astype(np.uint32)
        nan = ((b & 0x7F800000) == 0x7F800000) & ((b & 0x007FFFFF) != 0)
        b = np.where(nan, b & np.uint32(0xBFFFFFFF), b).astype(np.uint32)  # exponent 0x7F
        return np.ascontiguousarray(b.view(np.float32))
    if kind == "values32":
        a = VALUES32[rng.integers(0, len(VALUES32), (h, w, 4))]
        flat = a.reshape(-1)
        k = min(len(VALUES32), flat.size)
        flat[:k] = VALUES32[len(VALUES32) - k:]  # the float-only values first where room is short
        return np.ascontiguousarray(a, np.float32)
    return _make16(kind, w, h, seed)


def bits(img: np.ndarray) -> np.ndarray:
    """(H, W, 4) float32 -> its bit patterns."""
    return np.ascontiguousarray(img, np.float32).view(np.uint32)


# ------------------------------------------------------------- the rules ---
def chunk_bytes(px: np.ndarray) -> bytes:
    """(rows, W, 4) uint32 RGBA -> the chunk's uncompressed bytes."""
    planes = px[:, :, [3, 2, 1, 0]].transpose(0, 2, 1)  # rows, (A B G R), W
    return np.ascontiguousarray(planes).astype("<u4").tobytes()


def header_bytes(w: int, h: int) -> bytes:
    chl = b"".join(c.encode() + b"\0" + struct.pack("<iB3xii", FLOAT, 0, 1, 1) for c in CHANNELS) + b"\0"
    box = struct.pack("<4i", 0, 0, w - 1, h - 1)
    return (MAGIC + VERSION + _attr("channels", "chlist", chl) + _attr("compression", "compression", b"\x03")
            + _attr("dataWindow", "box2i", box) + _attr("displayWindow", "box2i", box)
            + _attr("lineOrder", "lineOrder", b"\x00") + _attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
            + _attr("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
            + _attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")


def write_exr32(px: np.ndarray, level: int = 1) -> bytes:
    """Reference writer: (H, W, 4) uint32 float bit patterns, RGBA -> file bytes."""
    px = np.asarray(px, np.uint32)
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
def read_exr32(data: bytes):
    """-> (pixels (H, W, 4) uint32 float bit patterns in R, G, B, A order,
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
        if c["pixelType"] != FLOAT:
            raise ExrError(f"channel {c['name']} has pixelType {c['pixelType']}, not FLOAT")
        if (c["pLinear"], c["reserved"], c["xSampling"], c["ySampling"]) != (0, (0, 0, 0), 1, 1):
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
    px = np.zeros((h, w, 4), np.uint32)
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
        n = 16 * w * rows
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
        planes = np.frombuffer(raw, "<u4").reshape(rows, 4, w)
        px[y:y + rows] = planes.transpose(0, 2, 1)[:, :, [3, 2, 1, 0]]
        sizes.append(size)
        modes.append(mode)
    if at != len(data):
        raise ExrError(f"{len(data) - at} bytes after the last chunk")
    return px, header, sizes, modes
