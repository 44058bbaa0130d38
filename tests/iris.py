"""IRIS files (Silicon Graphics .rgb, run-length coded), written down from the
format's byte layout and from the packet rule of the project: a strict reader,
a restatement of the encoder in numpy and Python, and the test images. Used by
test_iris_format.py (host coder) and test_gpu_iris.py (device coder).

The file, every number big-endian: 512 header bytes (int16 474; byte 1,
run-length coded; byte 1, a byte a channel; uint16 dimension, 2 for one channel
else 3; uint16 W, H, C; int32 pixmin 0; int32 pixmax 255; everything else 0),
the start table and the length table of H C uint32 entries each, then the coded
row-planes. A row-plane is one channel of one row: channels R, G, B(, A), or the
grey code of color_modes.grey8 for one channel. File row 0 is the image's bottom
row. Entry y + z H describes file row y of channel z: the offset from the start
of the file, and the coded bytes with the terminator. The coded row-planes are
contiguous: file row 0 first, within a row channel 0 .. C - 1.

The packet rule: no packet crosses a row-plane. A row-plane's maximal runs of
equal bytes that have at least 3 bytes are run stretches, the bytes between
them (runs of 2 included) literal stretches; a stretch of n bytes is n // 127
packets of 127 bytes and one of the remainder. Run packet: the byte count and
the value; literal packet: 0x80 | count and count bytes. One 0 byte ends the
row-plane."""
import struct

import numpy as np

import color_modes as M

HEADER = 512
PACKET = 127
MIN_RUN = 3
PIL_MODE = {1: "L", 3: "RGB", 4: "RGBA"}


class FormatError(ValueError):
    pass


def plane_bound(w):
    """The bytes of an all-literal row-plane and its terminator: no coded row-plane is longer."""
    return w + (w + PACKET - 1) // PACKET + 1


def body_bound(w, h, c):
    """The tables and every row-plane at its longest."""
    return h * c * (8 + plane_bound(w))


def expected(rgba8, c):
    """(H, W, 4) uint8 -> (H, W, c): what a reader returns, rows top first, R, G, B(, A) or grey."""
    return M.expected_png8(rgba8, c)


def file_planes(rgba8, c):
    """(H, W, 4) uint8 -> (H, c, W): the file's rows (bottom first), each as its c row-planes."""
    return np.ascontiguousarray(expected(rgba8, c)[::-1].transpose(0, 2, 1))


def header(w, h, c):
    return struct.pack(">hBBHHHHii", 474, 1, 1, 2 if c == 1 else 3, w, h, c, 0, 255) + bytes(HEADER - 20)


def pack_plane(p):
    """The packets of one row-plane, (W,) uint8, and its terminator."""
    w = len(p)
    out = bytearray()

    def stretch(a, b, run):
        for at in range(a, b, PACKET):
            k = min(PACKET, b - at)
            out.append(k if run else 0x80 | k)
            out.extend(p[at:at + (1 if run else k)].tobytes())

    change = np.flatnonzero(p[1:] != p[:-1]) + 1
    starts = np.concatenate([[0], change]).tolist()
    ends = np.concatenate([change, [w]]).tolist()
    lit = 0
    for s, e in zip(starts, ends):
        if e - s >= MIN_RUN:
            stretch(lit, s, False)
            stretch(s, e, True)
            lit = e
    stretch(lit, w, False)
    out.append(0)
    return bytes(out)


def encode(rgba8, c):
    """The file the project writes for an (H, W, 4) uint8 image in c channels."""
    planes = file_planes(rgba8, c)
    h, _, w = planes.shape
    n = h * c
    start, length = [0] * n, [0] * n
    coded, at = [], HEADER + 8 * n
    for y in range(h):
        for z in range(c):
            b = pack_plane(planes[y, z])
            start[y + z * h], length[y + z * h] = at, len(b)
            coded.append(b)
            at += len(b)
    return header(w, h, c) + struct.pack(f">{2 * n}I", *start, *length) + b"".join(coded)


def read(data):
    """Strict reader of the files above. Returns (pixels (H, W, c) rows top first
    in R, G, B(, A) / grey order, info). FormatError for: a header field that is
    not what the project writes; a start entry out of the stated order or not
    contiguous; a length entry that is not the bytes its row-plane takes; a
    row-plane that does not expand to exactly W bytes or does not end in its 0
    byte; a count of 0 before the terminator; three or more equal bytes in a
    row that are not a run packet's; packets that could have been one packet of
    at most 127; a short file, and trailing bytes."""
    if len(data) < HEADER:
        raise FormatError("short header")
    magic, storage, bpc, dim, w, h, c, pixmin, pixmax = struct.unpack(">hBBHHHHii", data[:20])
    if magic != 474:
        raise FormatError(f"header: magic {magic}")
    if storage != 1 or bpc != 1:
        raise FormatError(f"header: storage {storage}, {bpc} bytes a channel")
    if c not in (1, 3, 4) or dim != (2 if c == 1 else 3):
        raise FormatError(f"header: dimension {dim} with {c} channels")
    if w == 0 or h == 0:
        raise FormatError("header: size")
    if (pixmin, pixmax) != (0, 255):
        raise FormatError(f"header: pixmin {pixmin}, pixmax {pixmax}")
    if any(data[20:HEADER]):
        raise FormatError("header: dummy, name, colour map or padding not 0")
    n = h * c
    if len(data) < HEADER + 8 * n:
        raise FormatError("short tables")
    tab = struct.unpack(f">{2 * n}I", data[HEADER:HEADER + 8 * n])
    start, length = tab[:n], tab[n:]
    planes = np.zeros((h, c, w), np.uint8)
    packets = []
    pos = HEADER + 8 * n
    for y in range(h):
        row_packets = []
        for z in range(c):
            e = y + z * h
            if start[e] != pos:
                raise FormatError(f"row {y} channel {z}: start entry {start[e]}, the coded rows before it end at {pos}")
            p, x, plane_packets = planes[y, z], 0, []
            while True:
                if pos >= len(data):
                    raise FormatError("short body")
                b = data[pos]
                pos += 1
                k, lit = b & 127, bool(b & 128)
                if k == 0:
                    if lit:
                        raise FormatError(f"row {y} channel {z}: a literal packet of count 0")
                    if x < w:
                        raise FormatError(f"row {y} channel {z}: count 0 after {x} of {w} bytes")
                    break
                if x == w:
                    raise FormatError(f"row {y} channel {z}: no 0 byte after {w} bytes")
                if x + k > w:
                    raise FormatError(f"row {y} channel {z}: a packet of {k} bytes at {x} overruns the row's {w}")
                m = k if lit else 1
                if pos + m > len(data):
                    raise FormatError("short body")
                p[x:x + k] = np.frombuffer(data, np.uint8, m, pos)  # a run's one byte is broadcast
                pos += m
                x += k
                plane_packets.append((not lit, k))
            if length[e] != pos - start[e]:
                raise FormatError(f"row {y} channel {z}: length entry {length[e]}, the row takes {pos - start[e]} bytes")
            # the rule: every byte of a run of three and more is a run packet's ...
            eq = np.zeros(w + 3, bool)  # eq[j + 1]: byte j equals byte j - 1
            eq[2:w + 1] = p[1:] == p[:-1]
            in_run = (eq[:w] & eq[1:w + 1]) | (eq[1:w + 1] & eq[2:w + 2]) | (eq[2:w + 2] & eq[3:w + 3])
            x = 0
            for run, k in plane_packets:
                if not run and in_run[x:x + k].any():
                    raise FormatError(f"row {y} channel {z}: three equal bytes inside the literal packet at {x}")
                if run and not in_run[x:x + k].all():
                    raise FormatError(f"row {y} channel {z}: a run packet of {k} at {x} for a run below three bytes")
                x += k
            # ... and no two packets could have been one
            x = 0
            for (r0, k0), (r1, k1) in zip(plane_packets, plane_packets[1:]):
                x += k0
                if r0 and r1 and p[x - 1] == p[x] and k0 < PACKET:
                    raise FormatError(f"row {y} channel {z}: run packets of {k0} and {k1} at {x - k0} could merge")
                if not r0 and not r1 and k0 < PACKET:
                    raise FormatError(f"row {y} channel {z}: literal packets of {k0} and {k1} at {x - k0} could merge")
            row_packets.append(plane_packets)
        packets.append(row_packets)
    if pos != len(data):
        raise FormatError(f"{len(data) - pos} trailing bytes")
    img = np.ascontiguousarray(planes.transpose(0, 2, 1)[::-1])
    info = {"channels": c, "width": w, "height": h, "body": len(data) - HEADER, "packets": packets,
            "start": start, "length": length}
    return img, info


# ------------------------------------------------------------ the images ----
SIZES = [(1, 1), (2, 3), (3, 2), (63, 2), (64, 2), (65, 3), (126, 2), (127, 2), (128, 2), (129, 1), (254, 2), (255, 2),
         (256, 2), (257, 2), (381, 2), (300, 17), (5, 1100)]
ODD_AT = (63, 64, 127, 128, 255, 256)


def _runs_of(n, w, h, shifted):
    """Runs of exactly n bytes in every channel (neighbouring runs differ by 9 and
    more, so the grey code's do too). shifted: each channel's runs start one byte
    later than the channel's before, so the planes differ; else all four are one."""
    img = np.zeros((h, w, 4), np.uint8)
    x = np.arange(w + 4)
    for y in range(h):
        v = ((x + y) // n * 37 + 11 * y) % 251
        for z in range(4):
            img[y, :, z] = v[z:z + w] if shifted else v[:w]
    return img


def _odd_one_out(w, h, by_channel):
    """Rows that are one run but for a single other byte at one of ODD_AT (where the
    row has that byte). The rows take the places in turn, all channels at the same
    place (so the grey code has one odd byte too); by_channel: row y's channel z
    takes place 3 y + z, so two rows of three channels take all six."""
    img = np.zeros((h, w, 4), np.uint8)
    img[...] = np.array([40, 90, 160, 255], np.uint8)
    odd = np.array([41, 200, 20, 254], np.uint8)
    for y in range(h):
        for z in range(4):
            x = ODD_AT[(3 * y + z if by_channel else y) % len(ODD_AT)]
            if x < w:
                img[y, x, z] = odd[z]
    return img


def images():
    """name -> (H, W, 4) uint8: every size of SIZES in every kind. The same set serves every mode."""
    rng = np.random.default_rng(23)
    out = {}
    two = np.array([[0, 0, 0, 255], [255, 255, 255, 128]], np.uint8)
    for w, h in SIZES:
        s = f"{w}x{h}"
        out[f"random {s}"] = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        out[f"constant {s}"] = np.tile(np.array([17, 130, 201, 255], np.uint8), (h, w, 1))
        # two-valued noise, each channel its own
        out[f"two values {s}"] = np.stack([two[rng.integers(0, 2, (h, w)), z] for z in range(4)], axis=-1)
        out[f"runs of 3 {s}"] = _runs_of(3, w, h, False)
        out[f"runs of 3 shifted {s}"] = _runs_of(3, w, h, True)
        out[f"runs of 2 {s}"] = _runs_of(2, w, h, False)
        out[f"runs of 2 shifted {s}"] = _runs_of(2, w, h, True)
        out[f"odd one out {s}"] = _odd_one_out(w, h, False)
        out[f"odd one out by channel {s}"] = _odd_one_out(w, h, True)
    # the six places in one image in every mode
    out["odd one out 257x6"] = _odd_one_out(257, 6, False)
    return out


def _plane_of(parts, width, seed=0):
    """A row-plane from ('lit', n) and ('run', n) parts, padded with a ramp to `width`."""
    out, at = [], seed
    for k, (kind, n) in enumerate(parts):
        if kind == "lit":
            out.append(((np.arange(n) + at) % 256).astype(np.uint8))
            at += n
        else:
            out.append(np.full(n, (200 - 7 * k) % 256, np.uint8))
    p = np.concatenate(out)
    if len(p) < width:
        p = np.concatenate([p, ((np.arange(width - len(p)) + at + 64) % 256).astype(np.uint8)])
    return p


def device_images(chunk=256):
    """Beyond images(): stretches across the size kernel's steps of `chunk` bytes, runs
    on the seams, packets of 127 that do not line up with the steps, and rows and
    channels enough for several steps of the scan kernel."""
    c = chunk
    w = 3 * c + 40
    rows = [
        [("lit", c - 56), ("run", 200), ("lit", 200), ("run", 3)],       # each spans two steps
        [("lit", 100), ("run", 2 * c + 90), ("lit", 5)],                 # a step inside a run
        [("run", 100), ("lit", 2 * c + 90), ("run", 5)],                 # and inside a literal stretch
        [("lit", c - 1), ("run", 3), ("lit", c - 3), ("run", 4), ("lit", 2)],  # runs on the seams
        [("lit", c - 2), ("run", 3), ("lit", c - 2), ("run", 2), ("lit", 1)],  # a pair on the seam stays literal
        [("run", c), ("run", c), ("lit", c)],
        [("lit", c - 1), ("run", 127), ("run", 128), ("lit", 3)],
    ]
    img = np.zeros((len(rows), w, 4), np.uint8)
    for y, parts in enumerate(rows):
        for z in range(4):  # the channels take the rows in turn, so every plane of a row differs
            img[y, :, z] = _plane_of(rows[(y + z) % len(rows)], w, seed=17 * z + y)
    rng = np.random.default_rng(29)
    tall = rng.integers(0, 4, (700, 9, 4), dtype=np.uint8) * 60  # 700 x 4 row-planes: three steps of the scan
    return {"across steps": img, "tall 9x700": tall}
