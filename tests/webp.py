"""Lossless WebP files (a RIFF container with one VP8L chunk), written down from
the format's bit layout and from the run rule of the project: a strict reader of
the subset the project writes, a restatement of the encoder in numpy and Python,
and the test images. Used by test_webp_format.py (host coder) and
test_gpu_webp.py (device coder).

The file: "RIFF", uint32 size, "WEBP", "VP8L", uint32 payload size, the payload,
a 0 byte if the payload's size is odd. The payload is an LSB-first bit stream:
byte 0x2F, 14 bits W - 1, 14 bits H - 1, 1 bit alpha hint, 3 bits version 0;
bit 1, 2 bits type 2: subtract-green; bit 1, 2 bits type 0: predictor, 3 bits
block bits - 2, and its sub-image (1 bit colour cache 0, five prefix codes, the
green one's symbol the mode, pixels that take no bits); bit 0; 1 bit colour
cache 0, 1 bit meta prefix 0, five prefix codes (green + lengths 280 symbols,
red, blue, alpha 256, distance 40), the pixels.

The pixels a reader returns: R, G, B, A as they are with four channels; alpha
255 with three; the grey code of color_modes.grey8 in R, G and B with one.

The run rule: the unit is the residual pixel. Within a row a maximal stretch of
pixels whose residual equals their left neighbour's is cut into chunks of 4096
and the remainder; a chunk of at least MIN_RUN pixels is a copy at distance 1,
the pixels of a shorter one are literals. A row's first pixel is a literal."""
import glob
import os
import re
import struct

import numpy as np

import color_modes as M

# the minimum copy length is the rule header's (tools/webp_measure.py imports this file without pytest)
with open(glob.glob(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "*", "csrc",
                                 "webp_rule.h"))[0]) as _f:
    MIN_RUN = int(re.search(r"constexpr uint32_t kWebpMinRun = (\d+);", _f.read()).group(1))
MAX_COPY = 4096
MAX_SIDE = 16384
BLOCK_BITS = 9
SIZES = (280, 256, 256, 256, 40)  # green + lengths, red, blue, alpha, distance
CL_ORDER = (17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
TOKEN_MAX_BITS = 60  # a literal: four codes of 15 bits
HEADER_MAX_BITS = 128 + 5 * 64 + sum(SIZES) * 7
RIFF = 20
PIL_MODE = {1: "RGB", 3: "RGB", 4: "RGBA"}


class FormatError(ValueError):
    pass


def body_bound(w, h):
    """The payload's bytes with every pixel a literal at its longest, plus header: no payload is longer."""
    return (HEADER_MAX_BITS + w * h * TOKEN_MAX_BITS + 7) // 8


def file_bound(w, h):
    return RIFF + body_bound(w, h) + 1


def expected(rgba8, c):
    """(H, W, 4) uint8 -> (H, W, 4) uint8: the RGBA pixels a reader returns in colour mode c."""
    e = M.expected_png8(rgba8, c)
    h, w = e.shape[:2]
    out = np.full((h, w, 4), 255, np.uint8)
    out[..., :3] = e[..., :3] if c >= 3 else e[..., :1]
    if c == 4:
        out[..., 3] = e[..., 3]
    return out


def pil_expected(rgba8, c):
    """What PIL returns: RGBA with the alpha hint, RGB without."""
    return expected(rgba8, c)[..., :len(PIL_MODE[c])]


# ------------------------------------------------------------ transforms ----
def _words(px):
    """(H, W, 4) RGBA -> (H, W, 4) int64 channels after subtract-green, in the order A, R, G, B."""
    p = px.astype(np.int64)
    return np.stack([p[..., 3], (p[..., 0] - p[..., 1]) & 255, p[..., 1], (p[..., 2] - p[..., 1]) & 255], -1)


def residuals(px):
    """(H, W, 4) RGBA -> (H, W) uint32 residual words A << 24 | R << 16 | G << 8 | B."""
    t = _words(px)
    pred = np.empty_like(t)
    pred[:, 1:] = t[:, :-1]
    pred[1:, 0] = t[:-1, 0]
    pred[0, 0] = (255, 0, 0, 0)
    r = (t - pred) & 255
    return (r[..., 0] << 24 | r[..., 1] << 16 | r[..., 2] << 8 | r[..., 3]).astype(np.uint32)


def from_residuals(res):
    """(H, W) uint32 residual words -> (H, W, 4) RGBA: what a decoder makes of them."""
    res = np.asarray(res, np.uint32)
    h, w = res.shape
    r = np.stack([(res >> s) & 255 for s in (24, 16, 8, 0)], -1).astype(np.int64)
    row = np.cumsum(r, axis=1)  # left prediction within a row, from the row's first pixel
    first = np.cumsum(r[:, 0], axis=0) + np.array([255, 0, 0, 0])  # column 0: the pixel above; (0, 0): 0xFF000000
    t = (row - r[:, :1] + first[:, None]) & 255
    g = t[..., 2]
    return np.stack([(t[..., 1] + g) & 255, g, (t[..., 3] + g) & 255, t[..., 0]], -1).astype(np.uint8)


def prefix(v):
    """A length or distance code v >= 1 -> (symbol, extra bits, their value)."""
    if v <= 2:
        return v - 1, 0, 0
    d = v - 1
    h = d.bit_length() - 1
    return 2 * h + ((d >> (h - 1)) & 1), h - 1, d & ((1 << (h - 1)) - 1)


def tokens(row):
    """A row of residual words -> [("lit", word) | ("copy", n)] by the run rule."""
    row = [int(v) for v in row]
    out, x, w = [], 0, len(row)
    while x < w:
        if x == 0 or row[x] != row[x - 1]:
            out.append(("lit", row[x]))
            x += 1
            continue
        e = x
        while e < w and row[e] == row[e - 1]:
            e += 1
        while x < e:
            m = min(MAX_COPY, e - x)
            out.extend([("copy", m)] if m >= MIN_RUN else [("lit", row[x])] * m)
            x += m
    return out


# ----------------------------------------------------------- prefix codes ----
def lengths(freq, maxbits):
    """Code lengths of at most maxbits for counts with at least two nonzero: symbols by (count,
    index), the two-queue Huffman merge (a leaf before an internal node of equal weight),
    depths capped at maxbits, the Kraft sum repaired by moving leaves down, lengths handed
    out by rank. Returns (lengths, the deepest leaf of the unlimited tree)."""
    order = sorted((s for s in range(len(freq)) if freq[s]), key=lambda s: (freq[s], s))
    nu = len(order)
    assert nu >= 2
    iw, lpar, ipar = [], [0] * nu, [0] * nu
    li = ii = 0
    for _ in range(nu - 1):
        w = 0
        for _pick in range(2):
            if li < nu and (ii >= len(iw) or freq[order[li]] <= iw[ii]):
                w += freq[order[li]]
                lpar[li] = len(iw)
                li += 1
            else:
                w += iw[ii]
                ipar[ii] = len(iw)
                ii += 1
        iw.append(w)
    ni = len(iw)
    idepth = [0] * ni
    for k in range(ni - 2, -1, -1):
        idepth[k] = idepth[ipar[k]] + 1
    depth = [idepth[lpar[i]] + 1 for i in range(nu)]
    count = [0] * (maxbits + 2)
    for d in depth:
        count[min(d, maxbits)] += 1
    total = sum(count[i] << (maxbits - i) for i in range(1, maxbits + 1))
    while total > 1 << maxbits:
        count[maxbits] -= 1
        for i in range(maxbits - 1, 0, -1):
            if count[i]:
                count[i] -= 1
                count[i + 1] += 2
                break
        total -= 1
    lens = [0] * len(freq)
    j = nu
    for i in range(1, maxbits + 1):
        for _ in range(count[i]):
            j -= 1
            lens[order[j]] = i
    return lens, max(depth)


def canonical(lens):
    """{symbol: (code, length)}: canonical codes, the code's first bit its highest."""
    code, out = 0, {}
    for length in range(1, 16):
        for s, l in enumerate(lens):
            if l == length:
                out[s] = (code, length)
                code += 1
        code <<= 1
    return out


class Bits:
    def __init__(self):
        self.out, self.acc, self.n, self.bits = bytearray(), 0, 0, 0

    def put(self, v, nb):
        assert 0 <= v < (1 << nb) or nb == 0 and v == 0
        self.acc |= v << self.n
        self.n += nb
        self.bits += nb
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c):  # a prefix code's bits go first bit first
        code, length = c
        for k in range(length - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def simple(self, syms):
        self.put(1, 1)
        self.put(len(syms) - 1, 1)
        self.put(1 if syms[0] > 1 else 0, 1)
        self.put(syms[0], 8 if syms[0] > 1 else 1)
        if len(syms) == 2:
            self.put(syms[1], 8)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def write_code(b, freq, info):
    """One alphabet's code into b; returns {symbol: (code, length)}."""
    used = [s for s in range(len(freq)) if freq[s]]
    if not used or (len(used) <= 2 and used[-1] < 256):
        b.simple(used or [0])
        info.append({"simple": len(used)})
        return {s: (k, len(used) - 1) for k, s in enumerate(used)}
    lens, depth = lengths(freq, 15)
    clfreq = [lens.count(k) for k in range(19)]
    if sum(1 for f in clfreq if f) == 1:
        cllen = [1 if f else 0 for f in clfreq]
        clcode = {s: (0, 0) for s in range(19)}  # its only symbol takes no bits
    else:
        cllen = lengths(clfreq, 7)[0]
        clcode = canonical(cllen)
    info.append({"simple": None, "depth": depth, "cl_used": sum(1 for f in clfreq if f), "max_len": max(lens)})
    b.put(0, 1)
    b.put(19 - 4, 4)
    for k in CL_ORDER:
        b.put(cllen[k], 3)
    b.put(0, 1)
    for l in lens:
        b.code(clcode[l])
    return canonical(lens)


def wrap(payload):
    pad = len(payload) & 1
    return (b"RIFF" + struct.pack("<I", 12 + len(payload) + pad) + b"WEBPVP8L" + struct.pack("<I", len(payload)) +
            payload + b"\0" * pad)


def encode(rgba8, c, info=None):
    """The file of an (H, W, 4) uint8 image in colour mode c. info: a dict that receives the
    rows' tokens, the five codes' forms and the payload's bits."""
    px = expected(rgba8, c)
    h, w = px.shape[:2]
    res = residuals(px)
    toks = [tokens(row) for row in res]
    freq = [[0] * n for n in SIZES]
    for row in toks:
        for kind, v in row:
            if kind == "lit":
                for a, sh in enumerate((8, 16, 0, 24)):
                    freq[a][(v >> sh) & 255] += 1
            else:
                freq[0][256 + prefix(v)[0]] += 1
                freq[4][prefix(2)[0]] += 1
    b = Bits()
    b.put(0x2F, 8)
    b.put(w - 1, 14)
    b.put(h - 1, 14)
    b.put(1 if c == 4 else 0, 1)
    b.put(0, 3)
    b.put(1, 1), b.put(2, 2)
    b.put(1, 1), b.put(0, 2), b.put(BLOCK_BITS - 2, 3)
    b.put(0, 1)
    b.simple([1])
    for _ in range(4):
        b.simple([0])
    b.put(0, 1)
    b.put(0, 1), b.put(0, 1)
    forms = []
    codes = [write_code(b, f, forms) for f in freq]
    header_bits = b.bits
    for row in toks:
        for kind, v in row:
            if kind == "lit":
                for a, sh in enumerate((8, 16, 0, 24)):
                    b.code(codes[a][(v >> sh) & 255])
            else:
                sym, nb, extra = prefix(v)
                b.code(codes[0][256 + sym])
                b.put(extra, nb)
                b.code(codes[4][prefix(2)[0]])
    if info is not None:
        info.update(tokens=toks, codes=forms, bits=b.bits, header_bits=header_bits)
    assert header_bits <= HEADER_MAX_BITS
    return wrap(b.done())


# ----------------------------------------------------------------- reader ----
class _In:
    def __init__(self, data):
        self.d, self.pos = data, 0

    def get(self, nb):
        v = 0
        for k in range(nb):
            i = self.pos + k
            if i >> 3 >= len(self.d):
                raise FormatError("short: the bit stream ends inside the image")
            v |= ((self.d[i >> 3] >> (i & 7)) & 1) << k
        self.pos += nb
        return v


def _decoder(lens, what):
    """lens -> a function reading one symbol; a code with one used symbol takes no bits."""
    used = [s for s, l in enumerate(lens) if l]
    if not used:
        raise FormatError(f"{what}: a code without symbols")
    if len(used) == 1:
        return lambda src: used[0]
    kraft = sum(1 << (15 - l) for l in lens if l)
    if kraft > 1 << 15:
        raise FormatError(f"{what}: over-subscribed code")
    if kraft < 1 << 15:
        raise FormatError(f"{what}: under-subscribed code")
    table = {(code, length): s for s, (code, length) in canonical(lens).items()}

    def read(src):
        code = 0
        for length in range(1, 16):
            code = code << 1 | src.get(1)
            if (code, length) in table:
                return table[(code, length)]
        raise FormatError(f"{what}: no such code")
    return read


def _read_code(src, n, what, forms):
    if src.get(1):  # simple
        k = src.get(1) + 1
        syms = [src.get(8 if src.get(1) else 1)]
        if k == 2:
            syms.append(src.get(8))
            if syms[1] == syms[0]:
                raise FormatError(f"{what}: a simple code's symbols are equal")
        lens = [0] * n
        for s in syms:
            lens[s] = 1
        forms.append({"simple": k, "symbols": syms})
        return _decoder(lens, what)
    num = 4 + src.get(4)
    cllen = [0] * 19
    for k in CL_ORDER[:num]:
        cllen[k] = src.get(3)
    cl = _decoder(cllen, what + " code lengths")
    top = n
    if src.get(1):
        top = 2 + src.get(2 + 2 * src.get(3))
        if top > n:
            raise FormatError(f"{what}: max_symbol above the alphabet")
    lens, prev = [], 8
    while len(lens) < n and top > 0:
        top -= 1
        s = cl(src)
        if s < 16:
            lens.append(s)
            prev = s or prev
        else:
            rep = 3 + src.get(2) if s == 16 else 3 + src.get(3) if s == 17 else 11 + src.get(7)
            if len(lens) + rep > n:
                raise FormatError(f"{what}: a repeat passes the alphabet")
            lens.extend([prev if s == 16 else 0] * rep)
    lens += [0] * (n - len(lens))
    forms.append({"simple": None, "cl_used": sum(1 for l in cllen if l), "max_len": max(lens)})
    return _decoder(lens, what)


def _unprefix(src, p):
    if p < 4:
        return p + 1
    extra = (p - 2) >> 1
    return ((2 + (p & 1)) << extra) + src.get(extra) + 1


def read(data):
    """A file -> ((H, W, 4) RGBA, info). Strict: the sizes, every field of the subset the
    project writes, complete codes, copies at distance 1 inside a row, no bits after the
    image but zeros up to the byte, no bytes after the chunk but its pad."""
    if len(data) < RIFF or data[:4] != b"RIFF" or data[8:16] != b"WEBPVP8L":
        raise FormatError("header: not a RIFF WEBP VP8L file")
    riff, n = struct.unpack("<I", data[4:8])[0], struct.unpack("<I", data[16:20])[0]
    pad = n & 1
    if riff != 12 + n + pad:
        raise FormatError("chunk sizes: the RIFF size is not the chunk's")
    if len(data) < RIFF + n + pad:
        raise FormatError("short: the file ends inside the chunk")
    if len(data) > RIFF + n + pad:
        raise FormatError("trailing bytes after the chunk")
    if pad and data[-1] != 0:
        raise FormatError("trailing: the pad byte is not 0")
    src = _In(data[RIFF:RIFF + n])
    if src.get(8) != 0x2F:
        raise FormatError("header: signature")
    w, h, alpha = src.get(14) + 1, src.get(14) + 1, src.get(1)
    if src.get(3) != 0:
        raise FormatError("header: version")
    if (src.get(1), src.get(2)) != (1, 2):
        raise FormatError("header: subtract-green is not the first transform")
    if (src.get(1), src.get(2)) != (1, 0):
        raise FormatError("header: the predictor is not the second transform")
    block_bits = src.get(3) + 2
    if src.get(1):
        raise FormatError("header: a colour cache in the predictor's sub-image")
    sub = []
    sub_codes = [_read_code(src, s, "sub-image", sub) for s in SIZES]
    blocks = -(-w // (1 << block_bits)) * -(-h // (1 << block_bits))
    for _ in range(blocks):
        if any(f["simple"] != 1 for f in sub) or sub_codes[0](src) != 1:
            raise FormatError("header: the predictor's mode is not 1 at no bits")
    if src.get(1):
        raise FormatError("header: a third transform")
    if src.get(1) or src.get(1):
        raise FormatError("header: a colour cache or meta prefix codes")
    forms = []
    g, r, b, a, d = [_read_code(src, s, name, forms) for s, name in zip(SIZES, ("green", "red", "blue", "alpha",
                                                                                 "distance"))]
    header_bits = src.pos
    res = np.zeros((h, w), np.uint32)
    toks = []
    for y in range(h):
        x, row = 0, []
        while x < w:
            s = g(src)
            if s < 256:
                red, blue = r(src), b(src)
                res[y, x] = a(src) << 24 | red << 16 | s << 8 | blue
                row.append(("lit", int(res[y, x])))
                x += 1
                continue
            n_ = _unprefix(src, s - 256)
            if _unprefix(src, d(src)) != 2:
                raise FormatError("a copy at a distance code other than 2")
            if x == 0 or x + n_ > w:
                raise FormatError("a copy crosses a row")
            res[y, x:x + n_] = res[y, x - 1]
            row.append(("copy", n_))
            x += n_
        toks.append(row)
    end = src.pos
    if (end + 7) // 8 != n:
        raise FormatError("trailing bytes in the chunk" if (end + 7) // 8 < n else "short")
    if src.get(8 * n - end):
        raise FormatError("trailing bits after the image")
    px = from_residuals(res)
    if not alpha and not np.all(px[..., 3] == 255):
        raise FormatError("header: alpha hint 0 with alpha below 255")
    return px, {"width": w, "height": h, "alpha": alpha, "tokens": toks, "codes": forms, "bits": end,
                "header_bits": header_bits, "payload": n}


# ----------------------------------------------------------------- images ----
SIZES_HOST = [(1, 1), (2, 1), (1, 2), (3, 5), (65, 3), (300, 17), (40, 130)]


def _content(kind, w, h, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(np.array([10, 20, 30, 200], np.uint8), (h, w, 4)).copy()
    if kind == "half flat":
        img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        img[:, w // 2:] = (9, 9, 9, 255)
        return img
    if kind == "ramp":
        x, y = np.meshgrid(np.arange(w), np.arange(h))
        return np.stack([x, x + y, 2 * x + y, 255 - y], -1).astype(np.uint8)
    assert kind == "sparse"  # mostly one colour: runs of every length between the others
    img = np.full((h, w, 4), 100, np.uint8)
    hit = rng.random((h, w)) < 0.12
    img[hit] = rng.integers(0, 256, (int(hit.sum()), 4), dtype=np.uint8)
    return img


def images():
    out = {}
    for k, (w, h) in enumerate(SIZES_HOST):
        for j, kind in enumerate(("random", "flat", "half flat", "ramp", "sparse")):
            out[f"{kind} {w}x{h}"] = _content(kind, w, h, 10 * k + j)
    return out


def _word(a, r, g, b):
    return (a << 24 | r << 16 | g << 8 | b) & 0xFFFFFFFF


def _noise_words(rng, n):
    """n residual words, no two neighbours equal: all literals."""
    g = rng.integers(0, 256, n)
    g[1:][g[1:] == g[:-1]] ^= 1
    return (rng.integers(0, 256, n) << 16 | g << 8 | rng.integers(0, 256, n)).astype(np.uint32)


def stretch_rows(width=4104):
    """Rows of residual words, each with one stretch of exactly n equal-to-the-left pixels, n in
    STRETCHES, between words that alternate; then a row that ends in a stretch and a row that
    goes on with the same residual from its first pixel."""
    rows = []
    alt = np.where(np.arange(width) % 2, _word(0, 1, 255, 1), _word(0, 2, 254, 2)).astype(np.uint32)
    for n in STRETCHES:
        row = alt.copy()
        row[3:3 + n + 1] = _word(0, 251, 5, 251)  # n + 1 equal words: n of them equal their left neighbour
        rows.append(row)
    five = _word(0, 251, 5, 251)
    a, b = alt.copy(), alt.copy()
    a[-5:] = five
    b[:4] = five
    return np.stack(rows + [a, b])


STRETCHES = (2, 3, 4096, 4097, 4098, 4099)


def fibonacci_image(w=70, h=64):
    """Green residuals of 17 values whose counts are 1, 1, 2, 3, 5, ... 1597 and the rest on
    the most frequent: the unlimited tree is 16 deep. Red and blue are noise: no copies."""
    rng = np.random.default_rng(77)
    fib = [1, 1]
    while len(fib) < 17:
        fib.append(fib[-1] + fib[-2])
    n = w * h
    fib[-1] += n - sum(fib)
    g = np.repeat(np.arange(17) * 3 + 1, fib)
    rng.shuffle(g)
    res = (rng.integers(0, 256, n) << 16 | g << 8 | rng.integers(0, 256, n)).astype(np.uint32)
    return from_residuals(res.reshape(h, w))


def uniform_red_image(w=64, h=64):
    """Every red residual equally often (16 times): 256 codes of 8 bits, so the red code's
    code-length alphabet has one used symbol. Green and blue are noise."""
    rng = np.random.default_rng(78)
    n = w * h
    r = np.repeat(np.arange(256), n // 256)
    rng.shuffle(r)
    res = (r << 16 | rng.integers(0, 256, n) << 8 | rng.integers(0, 256, n)).astype(np.uint32)
    return from_residuals(res.reshape(h, w))


def device_images(chunk=256):
    """The shapes at which the device coder's steps meet: a wave (64), a workgroup step
    (`chunk`), the copy limit."""
    rng = np.random.default_rng(5)
    out = {}
    for w, h in ((1, 1), (1, 2), (2, 1), (3, 5)):
        out[f"random {w}x{h}"] = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    for w in (63, 64, 65, chunk - 1, chunk, chunk + 1):
        out[f"sparse {w}x3"] = _content("sparse", w, 3, w)
        out[f"random {w}x2"] = _content("random", w, 2, w + 1)
        out[f"flat {w}x2"] = _content("flat", w, 2, 0)
    out["flat row 16384"] = np.broadcast_to(np.array([0, 0, 0, 255], np.uint8), (1, MAX_SIDE, 4)).copy()
    out["stretches"] = from_residuals(stretch_rows())
    out["one colour 3x4"] = np.broadcast_to(np.array([7, 0, 9, 255], np.uint8), (4, 3, 4)).copy()
    out["one colour 40x9"] = _content("flat", 40, 9, 0)
    pick = lambda a, b: np.where(rng.random(2000) < 0.5, a, b).astype(np.uint32)  # noqa: E731
    two = pick(0, 255) << 24 | pick(3, 200) << 16 | rng.integers(0, 256, 2000).astype(np.uint32) << 8 | pick(0, 1)
    out["two values 50x40"] = from_residuals(two.reshape(40, 50))  # two residuals each in red, blue and alpha
    out["noise 64x64"] = _content("random", 64, 64, 64)
    out["fibonacci 70x64"] = fibonacci_image()
    out["uniform red 64x64"] = uniform_red_image()
    out["tall sparse 9x700"] = _content("sparse", 9, 700, 9)
    out["across steps"] = _content("sparse", 2 * chunk + 37, 5, 3)
    return out
