"""Radiance RGBE files ("HDR", .hdr), written down from the format's byte layout
and from the project's two rules (csrc/hdr_rule.h): a strict reader, a
restatement of the encoder in two independent parts (the quads through numpy's
frexp in float64, the packer as a walk over the runs), and the test images.
Used by test_hdr_format.py (host coder) and test_gpu_hdr.py (device coder).

The file: the text "#?RADIANCE\\nFORMAT=32-bit_rle_rgbe\\n\\n-Y <H> +X <W>\\n",
then the rows top first. A row of W < 8 or W > 32767 pixels is W quads R, G, B,
E. Every other row is 2, 2, W >> 8, W & 255 and the R, G, B and E planes, W
bytes each in packets: a byte above 128 is a run of (byte - 128) copies of the
next byte, a byte of 1 .. 128 that many literal bytes. Packets never cross a
plane.

The RGBE rule: a channel below 0, -0 or NaN is 0, a channel above 0x1.fep126 is
that; with m the largest channel and m = f 2^e (frexp), the quad is
floor(c 2^(8 - e)) a channel and e + 128; all zero for m < 1e-32f.

The packet rule: a plane's maximal runs of at least 4 equal bytes are run
stretches, the bytes between them literal stretches; a run stretch of n bytes
is n // 127 packets of 127 and one of the remainder, a literal stretch n // 128
packets of 128 and one of the remainder."""
import re

import numpy as np

import color_modes as M

F32 = np.float32
MAXV = F32(float.fromhex("0x1.fep126"))
TINY = F32(1e-32)
MIN_RUN, RUN_PACKET, LIT_PACKET = 4, 127, 128
HEADER_RE = re.compile(rb"#\?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y ([1-9][0-9]*) \+X ([1-9][0-9]*)\n")


class FormatError(ValueError):
    pass


def flat(w):
    return w < 8 or w > 32767


def plane_bound(w):
    """The bytes of an all-literal plane: no coded plane is longer."""
    return w + (w + 127) // 128


def row_bound(w):
    return 4 * w if flat(w) else 4 + 4 * plane_bound(w)


def header(w, h):
    return b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w)


# ------------------------------------------------------------ the RGBE rule --
def clamp(v):
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v) | np.signbit(v), F32(0), np.minimum(v, MAXV)).astype(F32)


def rgbe(rgb):
    """(..., 3) float32 -> (..., 4) uint8 quads."""
    c = clamp(rgb).astype(np.float64)
    m = c.max(axis=-1)
    _, e = np.frexp(m)
    e = e.astype(np.int64)
    mant = np.floor(c * np.ldexp(1.0, 8 - e)[..., None])  # exact: a power of two times a float32
    assert mant.max(initial=0) <= 255
    quad = np.concatenate([mant, (e + 128)[..., None]], axis=-1)
    quad[m < np.float64(TINY)] = 0
    assert quad.min(initial=0) >= 0 and quad.max(initial=0) <= 255
    return quad.astype(np.uint8)


def quads(rgba, c):
    """(H, W, >= 3) float32 means -> (H, W, 4) uint8 quads of the file in c channels (1: luma in all three)."""
    a = np.asarray(rgba, F32)[..., :3]
    if c == 1:
        with np.errstate(all="ignore"):
            y = M.luma(a[..., 0], a[..., 1], a[..., 2])
        a = np.stack([y, y, y], axis=-1)
    return rgbe(a)


def decode(quad):
    """(..., 4) uint8 -> (..., 3) float64: the least value of each channel's bracket, byte 2^(e - 136)."""
    q = np.asarray(quad).astype(np.int64)
    return np.where(q[..., 3:] == 0, 0.0, np.ldexp(q[..., :3].astype(np.float64), q[..., 3:] - 136))


# ---------------------------------------------------------- the packet rule --
def pack_plane(p):
    """The packets of one plane, (W,) uint8."""
    p = np.asarray(p, np.uint8)
    w = len(p)
    out = bytearray()

    def stretch(a, b, run):
        cap = RUN_PACKET if run else LIT_PACKET
        for at in range(a, b, cap):
            k = min(cap, b - at)
            out.append(128 + k if run else k)
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
    return bytes(out)


def pack_rows(quad):
    """(H, W, 4) uint8 quads -> the file's body."""
    h, w = quad.shape[:2]
    if flat(w):
        return np.ascontiguousarray(quad).tobytes()
    out = []
    for row in quad:
        out.append(bytes([2, 2, w >> 8, w & 255]))
        out.extend(pack_plane(row[:, k]) for k in range(4))
    return b"".join(out)


def encode(rgba, c=3):
    """The file the project writes for (H, W, >= 3) float32 means in c channels (3 or 1)."""
    q = quads(rgba, c)
    h, w = q.shape[:2]
    return header(w, h) + pack_rows(q)


# -------------------------------------------------------------- the reader --
def read(data):
    """Strict reader of the files above. Returns (quads (H, W, 4) uint8, info).
    FormatError for a header that is not the project's, a wrong marker or width,
    a packet of count 0, a packet that overruns its plane, a short body and
    trailing bytes."""
    data = bytes(data)
    m = HEADER_RE.match(data)
    if not m:
        raise FormatError("header")
    h, w = int(m.group(1)), int(m.group(2))
    pos = m.end()
    packets = []
    if flat(w):
        if len(data) - pos < 4 * w * h:
            raise FormatError("short body")
        if len(data) - pos > 4 * w * h:
            raise FormatError(f"{len(data) - pos - 4 * w * h} trailing bytes")
        quad = np.frombuffer(data, np.uint8, 4 * w * h, pos).reshape(h, w, 4).copy()
    else:
        quad = np.zeros((h, w, 4), np.uint8)
        for y in range(h):
            if pos + 4 > len(data):
                raise FormatError("short body")
            if data[pos:pos + 4] != bytes([2, 2, w >> 8, w & 255]):
                raise FormatError(f"row {y}: marker {list(data[pos:pos + 4])}")
            pos += 4
            row_packets = []
            for k in range(4):
                x, plane_packets = 0, []
                while x < w:
                    if pos >= len(data):
                        raise FormatError("short body")
                    b = data[pos]
                    pos += 1
                    run, n = b > 128, (b - 128 if b > 128 else b)
                    if b == 0:  # (128 is a literal packet of 128 bytes: a run of count 0 cannot be written)
                        raise FormatError(f"row {y} plane {k}: a packet of count 0 at {x}")
                    if x + n > w:
                        raise FormatError(f"row {y} plane {k}: a packet of {n} bytes at {x} overruns the plane's end at {w}")
                    need = 1 if run else n
                    if pos + need > len(data):
                        raise FormatError("short body")
                    quad[y, x:x + n, k] = np.frombuffer(data, np.uint8, need, pos)  # a run's byte is broadcast
                    pos += need
                    x += n
                    plane_packets.append((run, n))
                row_packets.append(plane_packets)
            packets.append(row_packets)
        if pos != len(data):
            raise FormatError(f"{len(data) - pos} trailing bytes")
    info = {"width": w, "height": h, "flat": flat(w), "body": len(data) - m.end(), "packets": packets}
    return quad, info


# ------------------------------------------------------------ the images ----
def floats_from_rgbe(r, g, b, e):
    """float32 (..., 4) images (alpha 1) whose quads are the given planes: the
    value (byte + 0.5) 2^(e - 136) lies inside its byte's bracket. Some channel
    must be >= 128 at every pixel (the exponent is then the pixel's own) and e in
    32 .. 250 (every value is then normal and below the clamp)."""
    r, g, b, e = (np.asarray(v).astype(np.int64) for v in (r, g, b, e))
    assert np.all(np.maximum(np.maximum(r, g), b) >= 128) and np.all((e >= 32) & (e <= 250))
    img = np.ones(r.shape + (4,), F32)
    for k, v in enumerate((r, g, b)):
        img[..., k] = np.ldexp(v.astype(np.float64) + 0.5, e - 136).astype(F32)
    want = np.stack([r, g, b, e], axis=-1).astype(np.uint8)
    assert np.array_equal(rgbe(img[..., :3]), want), "the restatement does not return the planes"
    return img


def plane_of(parts, width, lo, seed=0):
    """A plane from ('lit', n) and ('run', n) parts, padded with literals to `width`.
    Literal bytes are odd and differ from their neighbours, run values even: a run
    is exactly as long as it says. lo: the least value (128 for R, G, B; 32 for E)."""
    out, at = [], seed
    for k, (kind, n) in enumerate(parts):
        if kind == "lit":
            out.append(lo + 1 + 2 * (((np.arange(n) + at) * 19) % 59))
            at += n
        else:
            out.append(np.full(n, lo + 2 * ((k + seed) % 55)))
    have = sum(len(o) for o in out)
    assert have <= width, (have, width)
    if have < width:
        out.append(lo + 1 + 2 * (((np.arange(width - have) + at + 7) * 19) % 59))
    return np.concatenate(out).astype(np.uint8)


def image_of(rows, width):
    """rows: per row four part lists (R, G, B, E) -> the (H, W, 4) float32 image whose planes they are."""
    planes = [[plane_of(parts, width, 32 if k == 3 else 128, seed=3 * y + k) for k, parts in enumerate(row)]
              for y, row in enumerate(rows)]
    p = np.array(planes)  # H, 4, W
    return floats_from_rgbe(p[:, 0], p[:, 1], p[:, 2], p[:, 3])


WIDTHS = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257)
RUNS = (3, 4, 5, 126, 127, 128, 129, 254, 255)
LITS = (128, 129, 257)
PALETTE = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.8, 0.05, 0.05], [3.5e4, 2.0e-3, 7.0], [0.18, 0.18, 0.18],
                    [-1.0, 0.5, 2.0e-20]], F32)


def shape_image(w, h, seed=0):
    """(H, W, 4) float32: a palette with many repeats (runs in every plane) under smooth noise in some columns."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(PALETTE), (h, w)) * rng.integers(0, 2, (h, w))
    img = np.ones((h, w, 4), F32)
    img[..., :3] = PALETTE[idx]
    noisy = rng.random((h, w)) < 0.3
    img[noisy, :3] = np.exp(rng.normal(0, 3, (int(noisy.sum()), 3))).astype(F32)
    img[..., 3] = rng.random((h, w)).astype(F32)  # alpha is junk the coder ignores
    return img


def images():
    """name -> (H, W, 4) float32. The same set serves every mode."""
    out = {}
    for w in WIDTHS:
        for h in (1, 2, 3):
            out[f"shape {w}x{h}"] = shape_image(w, h, seed=100 * w + h)
    width = 3 + max(RUNS) + 6
    # runs of exactly n bytes between literals: each plane its own lengths (rotated), one row a length
    out["runs"] = image_of([[[("lit", 3), ("run", RUNS[(i + k) % len(RUNS)]), ("lit", 2)] for k in range(4)]
                            for i in range(len(RUNS))], width)
    # a run that ends a plane, a plane that is one run, runs back to back
    out["run ends"] = image_of([[[("lit", 5), ("run", 35)], [("run", 40)], [("run", 4), ("run", 36)],
                                 [("lit", 36), ("run", 4)]],
                                [[("run", 40)], [("lit", 40)], [("lit", 37), ("run", 3)], [("run", 40)]]], 40)
    out["literals"] = image_of([[[("run", 5), ("lit", n), ("run", 4)], [("lit", n), ("run", 7)],
                                 [("run", 4), ("lit", n)], [("lit", 1), ("run", 6), ("lit", n)]] for n in LITS], 270)
    # row 0's last quad equals row 1's first, and R's last byte equals G's first: packets do not cross
    p = np.array([[plane_of([("lit", 40)], 40, 32 if k == 3 else 128, seed=5 * y + k) for k in range(4)]
                  for y in range(3)])
    p[0, 0, -4:] = 200  # R of row 0 ends in a run of four of 200
    p[0, 1, :4] = 200   # and G of row 0 starts with one
    p[1, :, :3] = p[0, :, -1:]  # row 1 starts with three copies of row 0's last quad
    p[0, :, -3:] = p[0, :, -1:]
    p[2, :, 0] = p[1, :, -1]
    out["ends meet"] = floats_from_rgbe(p[:, 0], p[:, 1], p[:, 2], p[:, 3])
    return out


def device_images(chunk=256):
    """The shapes at which the device packer can go wrong, beyond images(): the
    64-lane ballot word, the packet caps, the kernel's step, stretches across steps."""
    c = chunk
    w = 3 * c + 40
    out = {"shape 513x2": shape_image(513, 2, seed=5)}
    lit, run = (lambda n: ("lit", n)), (lambda n: ("run", n))
    out["across words"] = image_of([
        [[lit(60), run(9), lit(50), run(20)], [run(64), run(64), lit(3)], [lit(62), run(4), lit(62), run(4)],
         [lit(61), run(3), run(5), lit(58), run(100)]],
        [[run(63), lit(2), run(63)], [lit(64), run(64), lit(64)], [lit(127), run(127)], [run(1), run(4), lit(59), run(4)]],
    ], c - 1)
    out["across steps"] = image_of([
        [[lit(c - 56), run(200), lit(200), run(3)], [lit(100), run(2 * c + 90), lit(5)],
         [run(100), lit(2 * c + 90), run(5)], [lit(c - 1), run(4), lit(c - 5), run(5), lit(1)]],
        [[lit(c - 2), run(4), lit(c - 3), run(4)], [run(c), run(c), lit(c)], [lit(c - 127), run(127), run(127)],
         [lit(c - 1), run(128), lit(c - 3), run(4)]],
        [[lit(c - 3), run(3), lit(c - 1), run(4)], [lit(c - 4), run(4), run(4)], [run(c + 1), lit(c - 1), run(c)],
         [lit(2 * c - 128), lit(128), run(127), run(1)]],
    ], w)
    return out


def special_row():
    """(1, N, 4) float32: the values at which the RGBE rule branches, one pixel each. More than 7
    and fewer than 32768 pixels: a coded row; the host tests cut it into flat pieces too."""
    inf, nan, big = F32(np.inf), F32(np.nan), np.finfo(F32).max
    up = lambda v: np.nextafter(F32(v), inf)         # noqa: E731
    down = lambda v: np.nextafter(F32(v), -inf)      # noqa: E731
    den = F32(1e-40)
    px = [(0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (-1.0, -1.0, -1.0), (nan, nan, nan), (inf, inf, inf), (-inf, -inf, -inf),
          (big, big, big), (MAXV, MAXV, MAXV), (up(MAXV), 1.0, 0.0), (down(MAXV), 1.0, 0.0),
          (TINY, TINY, TINY), (up(TINY), 0.0, 0.0), (down(TINY), down(TINY), 0.0), (den, 1.0e4, 0.0), (den, den, den),
          (1.0, 1.0, 1.0), (0.5, 0.5, 0.5), (down(1.0), down(1.0), down(1.0)), (1.0, 2.0 ** -20, 2.0 ** 20),
          (2.0 ** -20, 1.0, 0.0), (nan, 1.0, -1.0), (inf, -0.0, 0.25), (-nan, 3.0, big), (0.0, 0.0, up(TINY)),
          (1.0, down(1.0), up(1.0)), (255.5, 256.0, 0.99)]
    img = np.ones((1, len(px), 4), F32)
    img[0, :, :3] = np.array(px, F32)
    return img
