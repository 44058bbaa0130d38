"""TEST INFRASTRUCTURE ONLY — the checker of the device PNG encoder (png.hip, deflate.hip).

Pure Python and numpy; imports neither the package nor a GPU library. Two halves:

  * A strict, reporting inflate. parse_png() checks the signature and the chunk
    CRCs; inflate_blocks() walks the deflate bits (RFC 1951) itself and returns,
    per block, where it lies, its code lengths, its tokens and its bytes;
    bands() groups the blocks into the encoder's bands of 16 rows and checks
    the container scheme (independent byte-aligned pieces).
    zlib is never asked to decode; tests/test_png_oracle.py cross-checks this
    inflate against it.
  * A plain serial reference of what deflate.hip and DESIGN.md §4 say the encoder
    computes: the Sub filter, the greedy parse over the distances 1 / 4 / row
    above, the RFC's length and distance symbols as tables, and the cost and
    depth of an optimal (heap-built) Huffman code to judge the emitted codes
    by. Nothing here restates the encoder's segment / exit-table scheme.

Tokens are a literal byte (int) or a (length, distance) tuple.
"""
from __future__ import annotations

import heapq

import numpy as np

BAND_ROWS = 16      # kDeflateBandRows
WINDOW = 32768
MAX_MATCH = 258
MIN_MATCH = 3
FAR_STRIDE = 4096   # a 3-byte match further back than this is not taken
PIECE = 65535       # most bytes of one stored block

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195,
            227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
CL_EXTRA = {16: 2, 17: 3, 18: 7}


class PngError(ValueError):
    """The file or stream breaks PNG / zlib / deflate, or the encoder's container scheme."""


# ------------------------------------------------------------ checksums ------
_CRC_TABLE = []
for _n in range(256):
    _c = _n
    for _ in range(8):
        _c = (_c >> 1) ^ 0xEDB88320 if _c & 1 else _c >> 1
    _CRC_TABLE.append(_c)


def crc32(data) -> int:
    c = 0xFFFFFFFF
    t = _CRC_TABLE
    for b in bytes(data):
        c = t[(c ^ b) & 0xFF] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def adler32(data) -> int:
    b = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    if b.size == 0:
        return 1
    s1 = 1 + np.cumsum(b)  # < 2^63 for any input a test can hold
    return (int(s1.sum() % 65521) << 16) | int(s1[-1] % 65521)


# ------------------------------------------------------------ container ------
def parse_png(data: bytes):
    """(W, H, zlib stream) of an 8-bit RGBA, non-interlaced PNG; the IDAT chunks' data joined."""
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise PngError("bad PNG signature")
    at, chunks = 8, []
    while at < len(data):
        if at + 12 > len(data):
            raise PngError("truncated chunk")
        ln = int.from_bytes(data[at:at + 4], "big")
        kind = data[at + 4:at + 8]
        body = data[at + 8:at + 8 + ln]
        if len(body) != ln or at + 12 + ln > len(data):
            raise PngError("truncated chunk")
        if int.from_bytes(data[at + 8 + ln:at + 12 + ln], "big") != crc32(kind + body):
            raise PngError(f"bad CRC of chunk {kind!r}")
        chunks.append((kind, body))
        at += 12 + ln
    if not chunks or chunks[0][0] != b"IHDR" or len(chunks[0][1]) != 13 or chunks[-1] != (b"IEND", b""):
        raise PngError("IHDR must come first and an empty IEND last")
    hdr = chunks[0][1]
    W, H = int.from_bytes(hdr[:4], "big"), int.from_bytes(hdr[4:8], "big")
    if tuple(hdr[8:]) != (8, 6, 0, 0, 0) or W <= 0 or H <= 0:
        raise PngError("not an 8-bit RGBA non-interlaced image")
    idat = [c[1] for c in chunks if c[0] == b"IDAT"]
    if not idat:
        raise PngError("no IDAT")
    return W, H, b"".join(idat)


# -------------------------------------------------------------- inflate ------
def _decode_table(lens, what, strict):
    """Lookup table over the next maxlen stream bits (LSB first) of the canonical
    code with these lengths: len << 9 | symbol, or -1 where no code starts.
    Raises unless the Kraft sum is exactly 1; with strict off the RFC's one
    exception passes: a distance alphabet with at most one code."""
    used = [l for l in lens if l]
    maxl = max(used) if used else 1
    kraft = sum(1 << (maxl - l) for l in used)
    if kraft > 1 << maxl:
        raise PngError(f"{what} code is over-subscribed (Kraft sum {kraft} / {1 << maxl})")
    if kraft < 1 << maxl and (strict or what != "distance" or len(used) > 1):
        raise PngError(f"{what} code is incomplete (Kraft sum {kraft} / {1 << maxl})")
    count = [0] * (maxl + 2)
    for l in used:
        count[l] += 1
    nxt, code = [0] * (maxl + 2), 0
    for l in range(1, maxl + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    table = [-1] * (1 << maxl)
    for s, l in enumerate(lens):
        if not l:
            continue
        c = nxt[l]
        nxt[l] += 1
        r = int(format(c, f"0{l}b")[::-1], 2)
        for k in range(r, 1 << maxl, 1 << l):
            table[k] = (l << 9) | s
    return table, maxl


_FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_D = [5] * 32


class _Bits:
    """LSB-first reader of a byte string; pos is the next bit's index."""

    def __init__(self, data, pos):
        self.d, self.pos = data, pos

    def peek(self, n):  # zeros behind the stream's end; take() of the code found there raises
        p = self.pos
        return (int.from_bytes(self.d[p >> 3:(p + n + 7) >> 3], "little") >> (p & 7)) & ((1 << n) - 1)

    def take(self, n):
        p = self.pos
        if p + n > 8 * len(self.d):
            raise PngError("the stream ends inside a block")
        v = int.from_bytes(self.d[p >> 3:(p + n + 7) >> 3], "little") >> (p & 7)
        self.pos = p + n
        return v & ((1 << n) - 1)


def inflate_blocks(stream: bytes, strict: bool = True):
    """Blocks of a zlib stream, each a dict: bfinal, btype, start_bit, end_bit
    (bit indices into the stream, its two header bytes included), tokens, data;
    dynamic blocks add hlit, hdist, hclen, cl_lens (19, by symbol), cl_tokens
    ((symbol, extra) pairs), ll_lens (286), d_lens (30). Raises PngError on a
    code that is not exactly complete, an unused symbol in the stream, a
    distance that reaches before the data, LEN != ~NLEN, a wrong Adler-32 or
    bytes behind it."""
    stream = bytes(stream)
    if len(stream) < 6:
        raise PngError("zlib stream too short")
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf * 256 + flg) % 31 or flg & 0x20:
        raise PngError("bad zlib header")
    rd = _Bits(stream, 16)
    out = bytearray()
    blocks = []
    while True:
        blk = {"start_bit": rd.pos, "first_byte": len(out)}
        blk["bfinal"] = rd.take(1)
        blk["btype"] = btype = rd.take(2)
        toks = []
        if btype == 0:
            rd.pos = (rd.pos + 7) & ~7
            ln, nln = rd.take(16), rd.take(16)
            if ln ^ nln != 0xFFFF:
                raise PngError(f"stored block: LEN {ln:#06x} and NLEN {nln:#06x} do not match")
            p = rd.pos >> 3
            if p + ln > len(stream):
                raise PngError("the stream ends inside a stored block")
            out += stream[p:p + ln]
            rd.pos += 8 * ln
        elif btype == 3:
            raise PngError("block type 3")
        else:
            if btype == 1:
                ll_lens, d_lens = _FIXED_LL, _FIXED_D
            else:
                ll_lens, d_lens = _read_code_lengths(rd, blk, strict)
            if not ll_lens[256]:
                raise PngError("the end-of-block symbol has no code")
            lt, lbits = _decode_table(ll_lens, "literal/length", strict)
            dt, dbits = _decode_table(d_lens, "distance", strict)
            _inflate_tokens(rd, lt, lbits, dt, dbits, out, toks)
        blk["end_bit"] = rd.pos
        blk["tokens"] = toks
        blk["data"] = bytes(out[blk["first_byte"]:])
        blocks.append(blk)
        if blk["bfinal"]:
            break
    p = (rd.pos + 7) >> 3
    if len(stream) - p != 4:
        raise PngError(f"{len(stream) - p} bytes behind the final block, 4 expected")
    if int.from_bytes(stream[p:], "big") != adler32(out):
        raise PngError("wrong Adler-32")
    return blocks


def _read_code_lengths(rd, blk, strict):
    blk["hlit"], blk["hdist"], blk["hclen"] = hlit, hdist, hclen = rd.take(5) + 257, rd.take(5) + 1, rd.take(4) + 4
    if hlit > 286 or hdist > 30:
        raise PngError(f"HLIT {hlit} / HDIST {hdist} beyond the alphabets")
    cl = [0] * 19
    for i in range(hclen):
        cl[CL_ORDER[i]] = rd.take(3)
    blk["cl_lens"] = cl
    ct, cbits = _decode_table(cl, "code-length", strict)
    lens, ctoks = [], []
    while len(lens) < hlit + hdist:
        e = ct[rd.peek(cbits)]
        if e < 0:
            raise PngError("an unused code-length symbol appears in the stream")
        rd.take(e >> 9)
        s = e & 511
        x = rd.take(CL_EXTRA[s]) if s >= 16 else 0
        ctoks.append((s, x))
        if s < 16:
            lens.append(s)
        elif s == 16:
            if not lens:
                raise PngError("repeat of the previous code length at the first length")
            lens += [lens[-1]] * (3 + x)
        else:
            lens += [0] * ((3 if s == 17 else 11) + x)
    if len(lens) != hlit + hdist:
        raise PngError("a code-length run passes the end of the alphabets")
    blk["cl_tokens"] = ctoks
    blk["ll_lens"] = lens[:hlit] + [0] * (286 - hlit)
    blk["d_lens"] = lens[hlit:] + [0] * (30 - hdist)
    return blk["ll_lens"], blk["d_lens"]


def _inflate_tokens(rd, lt, lbits, dt, dbits, out, toks):
    d, nbytes = rd.d, len(rd.d)
    at = rd.pos >> 3
    buf, cnt = d[at] >> (rd.pos & 7) if at < nbytes else 0, 8 - (rd.pos & 7)
    at += 1
    lmask, dmask = (1 << lbits) - 1, (1 << dbits) - 1
    while True:
        if cnt < 56:  # a token has at most 15 + 5 + 15 + 13 bits
            chunk = d[at:at + 8]
            buf |= int.from_bytes(chunk, "little") << cnt
            cnt += 8 * len(chunk)
            at += len(chunk)
        e = lt[buf & lmask]
        if e < 0:
            raise PngError("an unused literal/length symbol appears in the stream")
        n = e >> 9
        s = e & 511
        buf >>= n
        cnt -= n
        if s < 256:
            out.append(s)
            toks.append(s)
        elif s == 256:
            break
        else:
            if s > 285:
                raise PngError(f"literal/length symbol {s} appears in the stream")
            x = LEN_EXTRA[s - 257]
            length = LEN_BASE[s - 257] + (buf & ((1 << x) - 1))
            buf >>= x
            cnt -= x
            e = dt[buf & dmask]
            if e < 0:
                raise PngError("an unused distance symbol appears in the stream")
            n = e >> 9
            s = e & 511
            if s > 29:
                raise PngError(f"distance symbol {s} appears in the stream")
            buf >>= n
            x = DIST_EXTRA[s]
            dist = DIST_BASE[s] + (buf & ((1 << x) - 1))
            buf >>= x
            cnt -= n + x
            if dist > len(out):
                raise PngError(f"distance {dist} reaches before the start of the data (at byte {len(out)})")
            if dist >= length:
                p = len(out) - dist
                out += out[p:p + length]
            else:
                for _ in range(length):
                    out.append(out[-dist])
            toks.append((length, dist))
        if cnt < 0:
            raise PngError("the stream ends inside a block")
    rd.pos = 8 * at - cnt
    if rd.pos > 8 * nbytes:
        raise PngError("the stream ends inside a block")


def expand(tokens, history: bytes = b"") -> bytes:
    """The bytes a token list stands for (behind an optional history)."""
    out = bytearray(history)
    for t in tokens:
        if isinstance(t, tuple):
            ln, dist = t
            if dist > len(out):
                raise PngError("distance before the start of the data")
            for _ in range(ln):
                out.append(out[-dist])
        else:
            out.append(t)
    return bytes(out[len(history):])


def bands(blocks, W, H):
    """Groups the blocks into the encoder's bands of min(16, remaining) rows by
    their decoded byte counts and checks the container scheme. A band is one
    dynamic block followed by an empty stored block, or stored pieces of at
    most 65,535 bytes; the last band has neither the empty block nor a cleared
    BFINAL on its last block; every band before the last ends on a byte
    boundary (the last is padded by the zlib trailer); BFINAL is set on the
    file's last block only; no match reaches before its own band's first byte.
    Returns per band: mode ("dynamic" / "stored"), row0, rows, n, blocks,
    tokens (dynamic), data, start_bit, end_bit, nbytes (emitted bytes)."""
    stride = 4 * W + 1
    for k, b in enumerate(blocks):
        if bool(b["bfinal"]) != (k + 1 == len(blocks)):
            raise PngError(f"BFINAL of block {k} of {len(blocks)} is {b['bfinal']}")
    res, k = [], 0
    for row0 in range(0, H, BAND_ROWS):
        rows = min(BAND_ROWS, H - row0)
        n = stride * rows
        last = row0 + rows == H
        if k >= len(blocks):
            raise PngError(f"no block left for the band at row {row0}")
        first = blocks[k]
        if first["btype"] == 2:
            mine = [first]
            k += 1
            if not last:
                if k >= len(blocks) or blocks[k]["btype"] != 0 or blocks[k]["data"]:
                    raise PngError(f"band at row {row0}: no empty stored block behind the dynamic block")
                mine.append(blocks[k])
                k += 1
            mode = "dynamic"
        elif first["btype"] == 0:
            mine, got = [], 0
            while got < n:
                if k >= len(blocks) or blocks[k]["btype"] != 0 or not blocks[k]["data"]:
                    raise PngError(f"band at row {row0}: stored pieces end after {got} of {n} bytes")
                mine.append(blocks[k])
                got += len(blocks[k]["data"])
                k += 1
            mode = "stored"
        else:
            raise PngError(f"band at row {row0}: block type {first['btype']}")
        data = b"".join(b["data"] for b in mine)
        if len(data) != n:
            raise PngError(f"band at row {row0}: {len(data)} bytes decoded, {n} expected")
        if not last and mine[-1]["end_bit"] % 8:
            raise PngError(f"band at row {row0} does not end on a byte boundary")
        if mine[0]["start_bit"] % 8:
            raise PngError(f"band at row {row0} does not start on a byte boundary")
        pos = 0
        for t in first["tokens"]:
            if isinstance(t, tuple):
                if t[1] > pos:
                    raise PngError(f"band at row {row0}: match of distance {t[1]} at byte {pos} reaches before its band")
                pos += t[0]
            else:
                pos += 1
        res.append({"mode": mode, "row0": row0, "rows": rows, "n": n, "blocks": mine, "tokens": first["tokens"],
                    "data": data, "start_bit": mine[0]["start_bit"], "end_bit": mine[-1]["end_bit"],
                    "nbytes": (mine[-1]["end_bit"] - mine[0]["start_bit"] + 7) // 8})
    if k != len(blocks):
        raise PngError(f"{len(blocks) - k} blocks behind the last band")
    return res


# ------------------------------------------------------------ reference ------
def sub_filter(rgba) -> np.ndarray:
    """PNG filter type 1 on every row: (H, 4W + 1) bytes, byte 0 of a row = 1,
    then each byte minus the byte one pixel (4 bytes) to its left, mod 256."""
    a = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w = a.shape[:2]
    row = a.reshape(h, 4 * w).astype(np.int16)
    left = np.zeros_like(row)
    left[:, 4:] = row[:, :-4]
    f = np.empty((h, 4 * w + 1), np.uint8)
    f[:, 0] = 1
    f[:, 1:] = ((row - left) & 0xFF).astype(np.uint8)
    return f


def image_from_filtered(f, W, H) -> np.ndarray:
    """Inverse of sub_filter: the (H, W, 4) image whose filtered stream is f
    (any bytes, byte 0 of every row being 1): a per-channel running sum mod 256."""
    f = np.asarray(f, np.uint8).reshape(H, 4 * W + 1)
    if not (f[:, 0] == 1).all():
        raise ValueError("byte 0 of every row must be the filter type 1")
    px = f[:, 1:].reshape(H, W, 4).astype(np.uint64)
    return (np.cumsum(px, axis=1) & 0xFF).astype(np.uint8)


def _runs(b, d):
    """run[i] = how many k >= 0 in a row have b[i + k] == b[i + k - d], i + k < n (0 for i < d)."""
    n = b.size
    eq = np.zeros(n + 1, bool)
    if d < n:
        eq[d:n] = b[d:] == b[:n - d]
    idx = np.arange(n + 1)
    stop = np.where(eq, n + 1, idx)  # the next position at or after i that does not match
    stop = np.minimum.accumulate(stop[::-1])[::-1]
    return (stop - idx)[:n]


def greedy_tokens(band_bytes, stride):
    """The documented parse of one band's filtered bytes. At each position the
    run of b[i] == b[i - d] for d = 1, 4 and the stride (the stride only when
    it is within the 32 KB window; never a distance beyond the position, never
    past the band's end; capped at 258); the longest wins if it is at least 3
    (at the stride: at least 4 when stride > 4096), ties to 1, then 4, then the
    stride; a match is taken and the parse goes on behind it, else a literal."""
    b = np.frombuffer(bytes(band_bytes), np.uint8)
    n = b.size
    dists = [1, 4] + ([stride] if stride <= WINDOW else [])
    runs = [np.minimum(_runs(b, d), MAX_MATCH).tolist() for d in dists]
    far_min = 4 if stride > FAR_STRIDE else MIN_MATCH
    vals = b.tolist()
    toks, i = [], 0
    while i < n:
        best, bd = 0, 0
        for d, r in zip(dists, runs):
            ln = r[i] if d <= i else 0
            if ln >= (far_min if d == stride else MIN_MATCH) and ln > best:
                best, bd = ln, d
        if best:
            toks.append((best, bd))
            i += best
        else:
            toks.append(vals[i])
            i += 1
    return toks


def len_symbol(length):
    """(symbol 257..285, extra bit count, extra bits' value) of a match length 3..258."""
    if not MIN_MATCH <= length <= MAX_MATCH:
        raise ValueError(length)
    k = max(i for i, base in enumerate(LEN_BASE) if base <= length)
    return 257 + k, LEN_EXTRA[k], length - LEN_BASE[k]


def dist_symbol(dist):
    """(symbol 0..29, extra bit count, extra bits' value) of a distance 1..32768."""
    if not 1 <= dist <= WINDOW:
        raise ValueError(dist)
    k = max(i for i, base in enumerate(DIST_BASE) if base <= dist)
    return k, DIST_EXTRA[k], dist - DIST_BASE[k]


def token_histograms(tokens):
    """(literal/length counts [286] with one end-of-block, distance counts [30], extra bits in all)."""
    ll, dd, extra = [0] * 286, [0] * 30, 0
    for t in tokens:
        if isinstance(t, tuple):
            s, nb, _ = len_symbol(t[0])
            ll[s] += 1
            extra += nb
            s, nb, _ = dist_symbol(t[1])
            dd[s] += 1
            extra += nb
        else:
            ll[t] += 1
    ll[256] += 1
    return ll, dd, extra


def huffman_lengths(freq):
    """Code lengths of a Huffman tree over the nonzero counts, built with a
    heap; among equal weights the shallower subtree is merged first. One symbol
    still takes one bit (deflate has no zero-length code)."""
    lens = [0] * len(freq)
    h = [(f, 0, [s]) for s, f in enumerate(freq) if f]
    if len(h) == 1:
        lens[h[0][2][0]] = 1
    heapq.heapify(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        for s in a[2] + b[2]:
            lens[s] += 1
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1, a[2] + b[2]))
    return lens


def _huffman(freq):
    lens = huffman_lengths(freq)
    return sum(f * l for f, l in zip(freq, lens)), max(lens, default=0)


def at_least_two_codes(freq):
    """The encoder gives every alphabet at least two codes, so that each is a
    complete prefix code (deflate.hip k_deflate_codes, as zlib does): unused symbols
    from the lowest index on count once until two are in use."""
    f = list(freq)
    for s in range(len(f)):
        if sum(1 for x in f if x) >= 2:
            break
        if not f[s]:
            f[s] = 1
    return f


def code_length_tokens(ll_lens, d_lens):
    """The 286 + 30 code lengths as one sequence in the code-length alphabet
    (RFC 1951 §3.2.7), every run taken as long as its symbol allows: zeros by
    18 (11..138) or 17 (3..10), other lengths once and then by 16 (3..6)."""
    seq = list(ll_lens) + list(d_lens)
    toks, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 3:
                r = min(run, 138)
                toks.append((17, r - 3) if r <= 10 else (18, r - 11))
                run -= r
        else:
            toks.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                toks.append((16, r - 3))
                run -= r
        toks += [(v, 0)] * run
    return toks


def symbol_counts(symbols, n):
    c = [0] * n
    for s in symbols:
        c[s] += 1
    return c


def optimal_cost(freq) -> int:
    """The least sum of count * code length any prefix code can reach."""
    return _huffman(freq)[0]


def unlimited_depth(freq) -> int:
    """The longest code of the heap-built Huffman tree, with no length limit."""
    return _huffman(freq)[1]


def stored_bytes(n) -> int:
    """n bytes as stored blocks: a 5-byte header per piece of at most 65,535 bytes."""
    return n + 5 * ((n + PIECE - 1) // PIECE)


def dynamic_lower_bound_bits(tokens) -> int:
    """A size no dynamic block of these tokens can go below: 3 + 5 + 5 + 4
    header bits before the code lengths, and the tokens under optimal codes."""
    ll, dd, extra = token_histograms(tokens)
    return 17 + optimal_cost(ll) + optimal_cost(dd) + extra
