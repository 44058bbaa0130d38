"""The OpenEXR files of rr_set_exr_codec NONE, RLE and PXR24: a restatement of
the writer's rules and a strict reader, in numpy + zlib (test code only).

The files are exr_reader's subset (single-part scanline, version 2, increasing
line order) with the channel lists Y / B, G, R / A, B, G, R of one pixel type
(1 HALF, 2 FLOAT) and the compression attribute 0 (NONE), 1 (RLE) or 5
(PXR24). Samples are handled as words: (H, W, C) uint16 half bits or uint32
float bits in the file's channel order (color_modes.expected_exr).

NONE: a chunk per scanline, the planes' words little-endian, n = word C W bytes.
RLE: a chunk per scanline; the n bytes through exr_reader.preprocess, then the
  packets of csrc/exr_rle_rule.h (rle_packets); a scanline whose packets are
  not shorter than n is stored raw. The decoder is OpenEXR's: a negative count
  copies -count bytes, otherwise count + 1 copies of the next byte.
PXR24: chunks of 16 scanlines; per scanline and channel one run of W pixels,
  the differences of the 16-bit (HALF) or 24-bit (FLOAT, float24) values to the
  pixel before as 2 or 3 planes of W bytes, most significant first; one zlib
  stream; a chunk whose stream is not smaller than the raw words is stored raw.

The reader accepts nothing else: any deviation raises ExrError.
"""
import struct
import zlib

import numpy as np

import exr_reader as X
from exr_reader import ExrError

NONE, RLE, PXR24 = 0, 1, 5
CODEC_NAME = {NONE: "NONE", RLE: "RLE", PXR24: "PXR24"}
CHANNELS = {1: ["Y"], 3: ["B", "G", "R"], 4: ["A", "B", "G", "R"]}
MIN_RUN, RUN_PACKET, LIT_PACKET = 3, 128, 127


# ------------------------------------------------------------- the rules ---
def float24(bits) -> np.ndarray:
    """uint32 float bits -> their 24-bit form (csrc/pxr24_rule.h)."""
    b = np.asarray(bits, np.uint32).astype(np.uint64)
    s, e, m = b & 0x80000000, b & 0x7F800000, b & 0x007FFFFF
    fin = ((e | m) + (m & 0x80)) >> 8
    fin = np.where(fin >= 0x7F8000, (e | m) >> 8, fin)
    mm = m >> 8
    nan = (e >> 8) | mm | (mm == 0)
    i = np.where(e == 0x7F800000, np.where(m != 0, nan, e >> 8), fin)
    return ((s >> 8) | i).astype(np.uint32)


def rle_packets(data: bytes) -> bytes:
    """The packets of csrc/exr_rle_rule.h for the bytes of one scanline: maximal
    runs of at least 3 equal bytes are run stretches, what lies between them
    literal stretches; a stretch is cut into packets of 128 (run) or 127
    (literal) bytes and a remainder."""
    b = np.frombuffer(bytes(data), np.uint8)
    n = len(b)
    edges = np.flatnonzero(np.concatenate([[True], b[1:] != b[:-1], [True]]))
    out = bytearray()

    def stretch(lo, hi, run):
        cap = RUN_PACKET if run else LIT_PACKET
        for at in range(lo, hi, cap):
            count = min(cap, hi - at)
            if run:
                out.append(count - 1)
                out.append(int(b[at]))
            else:
                out.append(256 - count)
                out.extend(b[at:at + count].tobytes())

    lit = 0
    for lo, hi in zip(edges[:-1], edges[1:]):
        if hi - lo >= MIN_RUN:
            if lit < lo:
                stretch(lit, lo, False)
            stretch(lo, hi, True)
            lit = hi
    if lit < n:
        stretch(lit, n, False)
    return bytes(out)


def rle_unpack(packets: bytes, n: int) -> bytes:
    """OpenEXR's decoder: exactly n bytes and no byte left over, else ExrError."""
    out = bytearray()
    at = 0
    while at < len(packets):
        c = packets[at] - 256 if packets[at] >= 128 else packets[at]
        at += 1
        if c < 0:
            if at - c > len(packets):
                raise ExrError("literal packet beyond the chunk")
            out += packets[at:at - c]
            at -= c
        else:
            if at >= len(packets):
                raise ExrError("run packet without its value")
            out += bytes([packets[at]]) * (c + 1)
            at += 1
        if len(out) > n:
            raise ExrError(f"packets decode to more than {n} bytes")
    if len(out) != n:
        raise ExrError(f"packets decode to {len(out)} bytes, not {n}")
    return bytes(out)


def raw_rows(words: np.ndarray) -> bytes:
    """(rows, W, C) words -> the scanlines' raw bytes: per row the planes."""
    dt = "<u2" if words.dtype == np.uint16 else "<u4"
    return np.ascontiguousarray(words.transpose(0, 2, 1)).astype(dt).tobytes()


def pxr24_front(words: np.ndarray) -> bytes:
    """(rows, W, C) words -> the bytes the chunk's zlib stream holds."""
    full = words.dtype == np.uint32
    v = (float24(words) if full else words.astype(np.uint32)).astype(np.uint32)
    v = v.transpose(0, 2, 1)  # rows, C, W
    d = v.copy()
    d[..., 1:] = v[..., 1:] - v[..., :-1]
    shifts = (16, 8, 0) if full else (8, 0)
    planes = np.stack([(d >> s) & 0xFF for s in shifts], axis=2)  # rows, C, S, W
    return planes.astype(np.uint8).tobytes()


def pxr24_back(front: bytes, rows: int, w: int, c: int, full: bool) -> np.ndarray:
    """The inverse of pxr24_front: (rows, W, C) words as a reader returns them
    (FLOAT: the 24 bits << 8)."""
    s = 3 if full else 2
    p = np.frombuffer(front, np.uint8).reshape(rows, c, s, w).astype(np.uint32)
    d = np.zeros((rows, c, w), np.uint32)
    for k in range(s):
        d |= p[:, :, k, :] << np.uint32(8 * (s - 1 - k))
    v = np.cumsum(d.astype(np.uint64), axis=-1).astype(np.uint32)
    if full:
        return ((v & 0xFFFFFF) << np.uint32(8)).transpose(0, 2, 1).astype(np.uint32)
    return (v & 0xFFFF).astype(np.uint16).transpose(0, 2, 1)


# ------------------------------------------------------------ the writer ---
def header_bytes(w: int, h: int, c: int, full: bool, codec: int) -> bytes:
    chl = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", 2 if full else 1, 0, 1, 1) for n in CHANNELS[c]) + b"\0"
    box = struct.pack("<4i", 0, 0, w - 1, h - 1)
    a = X._attr
    return (X.MAGIC + X.VERSION + a("channels", "chlist", chl) + a("compression", "compression", bytes([codec]))
            + a("dataWindow", "box2i", box) + a("displayWindow", "box2i", box)
            + a("lineOrder", "lineOrder", b"\x00") + a("pixelAspectRatio", "float", struct.pack("<f", 1.0))
            + a("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0))
            + a("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")


def chunk_rows(codec: int) -> int:
    return X.ROWS if codec == PXR24 else 1


def chunk_payload(words: np.ndarray, codec: int):
    """One chunk's (payload, mode) by the writer's rules; mode 'raw' or the codec's name in lower case."""
    raw = raw_rows(words)
    if codec == NONE:
        return raw, "raw"
    if codec == RLE:
        packed = rle_packets(X.preprocess(raw))
        return (packed, "rle") if len(packed) < len(raw) else (raw, "raw")
    z = zlib.compress(pxr24_front(words), 1)
    return (z, "pxr24") if len(z) < len(raw) else (raw, "raw")


def assemble(w, h, c, full, codec, chunks) -> bytes:
    """The file around chunks [(y, payload)]."""
    head = header_bytes(w, h, c, full, codec)
    at = len(head) + 8 * len(chunks)
    table = b""
    for _, p in chunks:
        table += struct.pack("<Q", at)
        at += 8 + len(p)
    return head + table + b"".join(struct.pack("<ii", y, len(p)) + p for y, p in chunks)


def write_exr(words: np.ndarray, codec: int):
    """Reference writer: (H, W, C) uint16 / uint32 words -> (file bytes, chunk modes)."""
    words = np.ascontiguousarray(words)
    assert words.dtype in (np.uint16, np.uint32) and words.ndim == 3 and words.shape[2] in CHANNELS
    h, w, c = words.shape
    step = chunk_rows(codec)
    chunks, modes = [], []
    for y in range(0, h, step):
        p, mode = chunk_payload(words[y:y + step], codec)
        chunks.append((y, p))
        modes.append(mode)
    return assemble(w, h, c, words.dtype == np.uint32, codec, chunks), modes


# ------------------------------------------------------------ the reader ---
def read_exr(data: bytes, codec: int):
    """-> (words (H, W, C) as a reader returns them, chunk modes, chunks
    [(y, mode, the chunk's content: raw bytes, or what a coded chunk's stream
    holds: the preprocessed bytes (RLE) or the byte planes (PXR24))])."""
    data = bytes(data)
    if data[:4] != X.MAGIC or data[4:8] != X.VERSION:
        raise ExrError("magic / version")
    header, at = {}, 8
    while True:
        if at >= len(data):
            raise ExrError("truncated header")
        if data[at] == 0:
            at += 1
            break
        name, at = X._cstr(data, at)
        typ, at = X._cstr(data, at)
        if at + 4 > len(data):
            raise ExrError("truncated header")
        size = struct.unpack_from("<i", data, at)[0]
        at += 4
        if size < 0 or at + size > len(data) or name in header:
            raise ExrError(f"attribute {name!r}")
        header[name] = X._value(typ, data[at:at + size])
        at += size
    want = {"channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio",
            "screenWindowCenter", "screenWindowWidth"}
    if set(header) != want:
        raise ExrError(f"attributes {sorted(header)}")
    names = [e["name"] for e in header["channels"]]
    if names not in CHANNELS.values():
        raise ExrError(f"channels {names}")
    c = len(names)
    ptype = header["channels"][0]["pixelType"]
    if ptype not in (1, 2):
        raise ExrError(f"pixel type {ptype}")
    for e in header["channels"]:
        if (e["pixelType"], e["pLinear"], e["reserved"], e["xSampling"], e["ySampling"]) != (ptype, 0, (0, 0, 0), 1, 1):
            raise ExrError(f"channel {e}")
    if header["compression"] != codec:
        raise ExrError(f"compression attribute {header['compression']}, not {codec}")
    if header["lineOrder"] != 0:
        raise ExrError("not increasing y")
    x0, y0, x1, y1 = header["dataWindow"]
    if (x0, y0) != (0, 0) or x1 < 0 or y1 < 0 or header["displayWindow"] != header["dataWindow"]:
        raise ExrError("windows")
    if (header["pixelAspectRatio"], header["screenWindowCenter"], header["screenWindowWidth"]) != (1.0, (0.0, 0.0), 1.0):
        raise ExrError("screen window / aspect")
    w, h = x1 + 1, y1 + 1
    full = ptype == 2
    word, dt = (4, "<u4") if full else (2, "<u2")
    step = chunk_rows(codec)
    nchunks = (h + step - 1) // step
    if at + 8 * nchunks > len(data):
        raise ExrError("truncated offset table")
    offsets = struct.unpack_from(f"<{nchunks}Q", data, at)
    at += 8 * nchunks
    px = np.zeros((h, w, c), np.uint32 if full else np.uint16)
    modes, chunks = [], []
    for k in range(nchunks):
        if offsets[k] != at:
            raise ExrError(f"offset table entry {k} is {offsets[k]}, the chunk is at {at}")
        if at + 8 > len(data):
            raise ExrError("truncated chunk header")
        y, size = struct.unpack_from("<ii", data, at)
        at += 8
        if y != k * step:
            raise ExrError(f"chunk {k} starts at scanline {y}")
        rows = min(step, h - y)
        n = word * c * w * rows
        if size <= 0 or size > n:
            raise ExrError(f"chunk {k} of {size} bytes, {n} uncompressed")
        if at + size > len(data):
            raise ExrError("truncated chunk")
        body = data[at:at + size]
        at += size
        if size == n:
            mode, content = "raw", body
            got = np.frombuffer(body, dt).reshape(rows, c, w).transpose(0, 2, 1)
        elif codec == NONE:
            raise ExrError(f"chunk {k} of {size} bytes in an uncompressed file")
        elif codec == RLE:
            mode, content = "rle", rle_unpack(body, n)
            got = np.frombuffer(X.unprocess(content), dt).reshape(rows, c, w).transpose(0, 2, 1)
        else:
            d = zlib.decompressobj()
            try:
                content = d.decompress(body) + d.flush()
            except zlib.error as e:  # a wrong Adler-32 included
                raise ExrError(f"chunk {k}: {e}") from e
            if not d.eof or d.unused_data:
                raise ExrError(f"chunk {k}: not exactly one complete zlib stream")
            front = (3 if full else 2) * c * w * rows
            if len(content) != front:
                raise ExrError(f"chunk {k} inflates to {len(content)} bytes, not {front}")
            mode, got = "pxr24", pxr24_back(content, rows, w, c, full)
        px[y:y + rows] = got
        modes.append(mode)
        chunks.append((y, mode, content))
    if at != len(data):
        raise ExrError(f"{len(data) - at} bytes after the last chunk")
    return px, modes, chunks


def expected_words(words: np.ndarray, codec: int, modes) -> np.ndarray:
    """What a reader returns of a file of `words` with the chunk modes `modes`:
    the words, but float24 << 8 in the coded chunks of a FLOAT PXR24 file."""
    out = np.array(words, copy=True)
    if codec == PXR24 and words.dtype == np.uint32:
        for k, mode in enumerate(modes):
            if mode == "pxr24":
                rows = slice(k * X.ROWS, (k + 1) * X.ROWS)
                out[rows] = float24(words[rows]) << np.uint32(8)
    return out


# ---------------------------------------------------------- test images ---
def run_row_words() -> np.ndarray:
    """One scanline of one HALF channel, (1, W, 1) uint16, whose preprocessed
    bytes hold runs of exactly 2, 3, 128, 129 and 256 equal bytes, separated by
    single other bytes: chosen through the inverse of the preprocessing. The
    runs lie in the low bytes' half; every high byte is 0x30 (finite halfs,
    which a float image can name), a run of its own."""
    low = bytearray()
    v = 1
    for run in (2, 3, 128, 129, 256, 2, 3):
        low += bytes([v]) * run
        v = (v * 7 + 3) & 0xFF
        low += bytes([v ^ 0x55])
        v = (v + 11) & 0xFF
    m = len(low)
    last = (sum(low) - 128 * (m - 1)) & 0xFF  # the last low byte after the predictor is undone
    high = bytes([(0x30 - last + 128) & 0xFF]) + bytes([128]) * (m - 1)
    raw = X.unprocess(bytes(low) + high)
    return np.frombuffer(raw, "<u2").astype(np.uint16).reshape(1, -1, 1)
