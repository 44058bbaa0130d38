"""TARGA files, written down from the format's byte layout and from the packet
rule of the project ("TARGA": run-length coded, "TARGA_RAW": plain): a strict
reader, a restatement of the encoder in numpy, and the test images. Used by
test_tga_format.py (host coder) and test_gpu_tga.py (device coder).

The file: 18 header bytes (id length 0, no colour map, image type 2 true colour
or 3 grey, + 8 run-length coded, colour-map specification 0, origin 0 0, width
and height uint16 little-endian, 8 C bits a pixel, descriptor 8 for C = 4 else
0: bottom-left origin), then the rows bottom first, pixels B, G, R(, A) or the
grey code of color_modes.grey8. No footer.

The packet rule: packets never cross a row. A row's maximal runs of equal
pixels that have at least 2 pixels (C = 3, 4) or 3 (C = 1) are run stretches,
the pixels between them literal stretches; a stretch of n pixels is n // 128
packets of 128 pixels and one of the remainder. Run packet: 0x80 | (count - 1)
and one pixel; literal packet: count - 1 and count pixels."""
import struct

import numpy as np

import color_modes as M

HEADER = 18
PIL_MODE = {1: "L", 3: "RGB", 4: "RGBA"}


class FormatError(ValueError):
    pass


def min_run(c):
    return 3 if c == 1 else 2


def row_bound(w, c):
    """The bytes of an all-literal row: no coded row is longer."""
    return w * c + (w + 127) // 128


def expected(rgba8, c):
    """(H, W, 4) uint8 -> (H, W, c): what a reader returns, rows top first, R, G, B(, A) or grey."""
    return M.expected_png8(rgba8, c)


def file_rows(rgba8, c):
    """(H, W, 4) uint8 -> (H, W, c): the file's rows (bottom first) of pixels in file order."""
    a = np.asarray(rgba8, np.uint8)[::-1]
    if c == 1:
        return np.ascontiguousarray(M.grey8(a)[..., None])
    return np.ascontiguousarray(a[..., [2, 1, 0, 3][:c]])


def header(w, h, c, rle):
    return struct.pack("<BBBHHBHHHHBB", 0, 0, (3 if c == 1 else 2) + (8 if rle else 0), 0, 0, 0, 0, 0, w, h, 8 * c,
                       8 if c == 4 else 0)


def pack_row(row):
    """The packets of one row, (W, c) uint8 in file order."""
    w, c = row.shape
    out = bytearray()

    def stretch(a, b, run):
        for at in range(a, b, 128):
            k = min(128, b - at)
            out.append((0x80 if run else 0) | (k - 1))
            out.extend(row[at:at + (1 if run else k)].tobytes())

    change = np.flatnonzero(np.any(row[1:] != row[:-1], axis=1)) + 1
    starts = np.concatenate([[0], change]).tolist()
    ends = np.concatenate([change, [w]]).tolist()
    lit = 0
    for s, e in zip(starts, ends):
        if e - s >= min_run(c):
            stretch(lit, s, False)
            stretch(s, e, True)
            lit = e
    stretch(lit, w, False)
    return bytes(out)


def encode(rgba8, c, rle):
    """The file the project writes for an (H, W, 4) uint8 image in c channels."""
    rows = file_rows(rgba8, c)
    h, w = rows.shape[:2]
    body = b"".join(pack_row(r) for r in rows) if rle else rows.tobytes()
    return header(w, h, c, rle) + body


def read(data):
    """Strict reader of the files above. Returns (pixels (H, W, c) rows top first
    in R, G, B(, A) / grey order, info). FormatError for a header field that is
    not what the project writes, a packet that crosses or overruns its row, a
    short body, and trailing bytes."""
    if len(data) < HEADER:
        raise FormatError("short header")
    idlen, cmap, typ, cm0, cmn, cmb, x0, y0, w, h, bpp, desc = struct.unpack("<BBBHHBHHHHBB", data[:HEADER])
    if idlen != 0 or cmap != 0 or (cm0, cmn, cmb) != (0, 0, 0):
        raise FormatError("image id or colour map present")
    if typ not in (2, 3, 10, 11):
        raise FormatError(f"image type {typ}")
    if (x0, y0) != (0, 0) or w == 0 or h == 0:
        raise FormatError("origin or size")
    grey = typ in (3, 11)
    if bpp not in ((8,) if grey else (24, 32)):
        raise FormatError(f"{bpp} bits a pixel in image type {typ}")
    c = bpp // 8
    if desc != (8 if c == 4 else 0):
        raise FormatError(f"descriptor {desc:#x}")
    rle = typ >= 10
    pos = HEADER
    packets = []
    if not rle:
        if len(data) != HEADER + w * h * c:
            raise FormatError("body is not W H C bytes")
        rows = np.frombuffer(data, np.uint8, w * h * c, HEADER).reshape(h, w, c)
        pos = len(data)
    else:
        rows = np.zeros((h, w, c), np.uint8)
        for y in range(h):
            x, row_packets = 0, []
            while x < w:
                if pos >= len(data):
                    raise FormatError("short body")
                b = data[pos]
                pos += 1
                k, run = (b & 127) + 1, bool(b & 128)
                if x + k > w:
                    raise FormatError(f"row {y}: a packet of {k} pixels at {x} crosses the row's end at {w}")
                n = c if run else k * c
                if pos + n > len(data):
                    raise FormatError("short body")
                px = np.frombuffer(data, np.uint8, n, pos).reshape(-1, c)
                rows[y, x:x + k] = px  # a run's one pixel is broadcast
                pos += n
                x += k
                row_packets.append((run, k))
            packets.append(row_packets)
        if pos != len(data):
            raise FormatError(f"{len(data) - pos} trailing bytes")
    img = rows[::-1]
    if c >= 3:
        img = img[..., [2, 1, 0, 3][:c]]
    info = {"channels": c, "rle": rle, "width": w, "height": h, "body": len(data) - HEADER, "packets": packets}
    return np.ascontiguousarray(img), info


# ------------------------------------------------------------ the images ----
def _distinct(n, seed=0):
    """n RGBA pixels, neighbours different in every mode: the grey code steps by one."""
    v = ((np.arange(n) + seed) % 256).astype(np.uint8)
    px = np.stack([v, v, v, np.full(n, 255, np.uint8)], axis=1)
    px[:, 3] -= (np.arange(n) % 3).astype(np.uint8)  # alpha varies too
    return px


def _row_of(parts, width=None, seed=0):
    """A row from ('lit', n) and ('run', n) parts, padded with distinct pixels to `width`.
    A run's colour is far from the ramp of the literals around it."""
    out, at = [], seed
    for k, (kind, n) in enumerate(parts):
        if kind == "lit":
            out.append(_distinct(n, at))
            at += n
        else:
            col = np.array([200 - 7 * k, 40 + 5 * k, 90 + 3 * k, 255 - k], np.uint8)
            out.append(np.tile(col, (n, 1)))
    row = np.concatenate(out)
    if width is not None and len(row) < width:
        row = np.concatenate([row, _distinct(width - len(row), at + 64)])
    return row


SIZES = [(w, h) for w in (1, 2, 3, 127, 128, 129, 255, 256, 257, 300) for h in (1, 3)]
RUNS = (1, 2, 3, 127, 128, 129, 256, 257)


def images():
    """name -> (H, W, 4) uint8. The same set serves every mode."""
    rng = np.random.default_rng(7)
    out = {}
    for w, h in SIZES:
        out[f"constant {w}x{h}"] = np.tile(np.array([17, 130, 201, 255], np.uint8), (h, w, 1))
        out[f"distinct {w}x{h}"] = np.stack([_distinct(w, 31 * y) for y in range(h)])
        pal = np.array([[0, 0, 0, 255], [255, 255, 255, 255], [200, 30, 30, 255]], np.uint8)
        out[f"palette {w}x{h}"] = pal[rng.integers(0, 3, (h, w))]
    # runs of exactly n pixels between literals, one row a length
    width = max(RUNS) + 6
    out["runs"] = np.stack([_row_of([("lit", 3), ("run", n), ("lit", 2)], width, seed=5 * n) for n in RUNS])
    # runs back to back (each its own stretch), and pairs only: runs for C = 3, 4, literals for C = 1
    out["runs back to back"] = np.stack([_row_of([("run", n), ("run", 2), ("run", 130), ("run", 3)], width + 135)
                                         for n in RUNS])
    out["pairs"] = np.repeat(_distinct(150, 9), 2, axis=0)[None]
    # literal stretches of 129 and 257 pixels between runs
    out["literals"] = np.stack([_row_of([("run", 5), ("lit", n), ("run", 4)], 270, seed=n) for n in (129, 257)])
    # a row's last pixel(s) equal the next row's first: no packet crosses
    a = np.stack([_distinct(40, 50 * y) for y in range(4)])
    a[1, :1] = a[0, -1]
    a[2, :2] = a[1, -1]
    a[1, -2:] = a[1, -1]
    a[3, :3] = a[2, -1]
    a[2, -3:] = a[2, -1]
    out["row ends"] = a
    # equal in all but one channel
    q = np.array([[10, 20, 30, 255], [10, 20, 31, 255], [10, 21, 31, 255], [11, 21, 31, 255], [11, 21, 31, 254],
                  [11, 21, 31, 254], [11, 21, 31, 255]], np.uint8)
    out["one channel"] = np.tile(q, (2, 9, 1))
    # no top / bottom symmetry
    g = np.zeros((5, 37, 4), np.uint8)
    g[..., 0] = (np.arange(5) * 50)[:, None]
    g[..., 1] = np.arange(37)[None] // 4
    g[..., 3] = 255
    out["rows"] = g
    return out


def device_images(chunk=256):
    """The shapes at which the device packer can go wrong, beyond images(): the
    ballot word, the packet edge, the kernel's row chunk, stretches across chunks."""
    rng = np.random.default_rng(11)
    out = {}
    pal = np.array([[5, 5, 5, 255], [250, 250, 250, 255], [30, 200, 30, 255], [30, 200, 30, 128]], np.uint8)
    widths = sorted({63, 64, 65, 127, 128, 129, 255, 256, 257, chunk - 1, chunk, chunk + 1})
    for w in widths:
        for h in (1, 2, 17):
            out[f"palette {w}x{h}"] = pal[rng.integers(0, 4, (h, w)) * rng.integers(0, 2, (h, w))]
            out[f"distinct {w}x{h}"] = np.stack([_distinct(w, 13 * y) for y in range(h)])
        out[f"constant {w}x2"] = np.tile(np.array([1, 2, 3, 4], np.uint8), (2, w, 1))
    c = chunk
    out["across chunks"] = np.stack([
        _row_of([("lit", c - 56), ("run", 200), ("lit", 200), ("run", 3)], 3 * c + 40),      # each spans two chunks
        _row_of([("lit", 100), ("run", 2 * c + 90), ("lit", 5)], 3 * c + 40),                # a chunk inside a run
        _row_of([("run", 100), ("lit", 2 * c + 90), ("run", 5)], 3 * c + 40),                # and inside a literal stretch
        _row_of([("lit", c - 1), ("run", 2), ("lit", c - 2), ("run", 3), ("lit", 1)], 3 * c + 40),  # runs on the seams
        _row_of([("lit", c - 2), ("run", 3), ("lit", c - 3), ("run", 4)], 3 * c + 40),
        _row_of([("run", c), ("run", c), ("lit", c)], 3 * c + 40),
    ])
    return out
