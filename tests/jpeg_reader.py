"""A strict baseline JPEG reader for the tests, written from ITU-T T.81 (and the
JFIF 1.02 APP0 layout). Pure Python and numpy; it shares no table and no line
with the project's coders. No test functions.

read_jpeg(data) accepts exactly this: SOI, one JFIF APP0, then DQT / DHT / DRI
and one SOF0 in any order, one SOS, one entropy-coded segment, EOI, and nothing
after it. One component sampled 1x1, or three with Y 2x2 and Cb / Cr 1x1 in one
interleaved scan. Everything else raises FormatError, in particular:

 - any other marker (progressive, arithmetic, 12-bit, APPn, COM), a second SOF0
   or SOS, a table the scan names but no segment defined, a segment that runs
   past the file, bytes after EOI, a missing EOI;
 - a DHT whose code lengths overflow the code space, that lists a symbol twice,
   a DC symbol above 11, an AC symbol with a size above 10 or a size of 0 with a
   run other than 0 (EOB) or 15 (ZRL);
 - inside the scan: 0xFF followed by anything but 00, the expected RSTn or EOI
   (a marker inside an interval, fill bytes, an un-stuffed 0xFF); an RSTn whose
   number is not the count of intervals before it modulo 8; an RSTn in a file
   without DRI; more or fewer intervals than the frame has MCUs for;
 - inside an interval: a bit pattern that is no code of the table the file
   gave, a run that passes coefficient 63, a symbol cut short by the interval's
   end, bits left over that are not fewer than 8 one-bits, whole bytes left over.

The DC predictions are reset at every restart. Decode tables are built from the
file's DHT segments alone.
"""
import struct

import numpy as np


class FormatError(ValueError):
    pass


def _zigzag():
    """Figure 5 of T.81: natural index of zigzag position k, walked, not listed."""
    order, x, y, up = [], 0, 0, True
    for _ in range(64):
        order.append(8 * y + x)
        if up:
            if x == 7:
                y, up = y + 1, False
            elif y == 0:
                x, up = x + 1, False
            else:
                x, y = x + 1, y - 1
        else:
            if y == 7:
                x, up = x + 1, True
            elif x == 0:
                y, up = y + 1, True
            else:
                x, y = x - 1, y + 1
    return np.array(order, np.int64)


ZIGZAG = _zigzag()


def dct_matrix():
    """C[u, x] = c(u) / 2 cos((2x + 1) u pi / 16), c(0) = 1 / sqrt 2: the orthonormal DCT-II (A.3.3)."""
    u, x = np.mgrid[0:8, 0:8].astype(np.float64)
    c = np.where(u == 0, np.sqrt(0.5), 1.0) * 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    return c


class Jpeg:
    """What read_jpeg returns.

    width, height, precision, dri   header fields
    jfif                            (major, minor, units, xdensity, ydensity)
    components                      [(id, h, v, tq)] of SOF0
    scan                            [(id, td, ta)] of SOS
    qtables                         {tq: (64,) int64, natural order}
    coeffs                          per component (blocks_y, blocks_x, 64) int64, natural order
    symbols                         per component [by][bx] -> [(run, size), ...]: the DC symbol as
                                    (0, size) first, then the AC symbols, ZRL (15, 0) and EOB (0, 0) included
    block_bits                      per component (blocks_y, blocks_x) coded bits of the block
    block_order                     per interval [(component, by, bx)] in coded order
    intervals                       [{"bytes", "stuffed", "pad_bits", "last_byte"}]: the interval's data
                                    bytes before stuffing, its stuffed 0xFF count, its padding bits and the
                                    last data byte (padding included)
    dqt_segments, dht_segments      the segments' bytes, marker and length included, in file order
    """

    def quantiser(self, ci):
        return self.qtables[self.components[ci][3]]

    def idct_pixels(self):
        """One-component files: dequantise, float64 IDCT (A.3.3), + 128; (height, width) float64, unclipped."""
        if len(self.components) != 1:
            raise ValueError("one-component files only")
        c = dct_matrix()
        f = (self.coeffs[0] * self.qtables[self.components[0][3]]).astype(np.float64)
        by, bx = f.shape[:2]
        px = np.einsum("vy,abvu,ux->abyx", c, f.reshape(by, bx, 8, 8), c) + 128.0
        return px.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)[:self.height, :self.width]


def _lut(bits, vals, what):
    """16-bit peek -> len << 8 | symbol (0: no code), from BITS and HUFFVAL (Annex C)."""
    lut = np.zeros(1 << 16, np.int64)
    code, k = 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            if code >= (1 << ln) - 1:  # the all-ones code of every length stays free (Annex C)
                raise FormatError(f"{what}: code lengths overflow the code space")
            lut[code << (16 - ln):(code + 1) << (16 - ln)] = (ln << 8) | vals[k]
            code += 1
            k += 1
        code <<= 1
    return lut.tolist()


def _segments(data):
    """-> ([(marker, payload, raw)] up to and including SOS, offset of the entropy-coded data)."""
    if data[:2] != b"\xff\xd8":
        raise FormatError("no SOI")
    at, segs = 2, []
    while True:
        if at + 4 > len(data):
            raise FormatError("file ends inside the headers")
        if data[at] != 0xFF:
            raise FormatError(f"byte {data[at]:#x} at {at} where a marker belongs")
        m = data[at + 1]
        n = struct.unpack_from(">H", data, at + 2)[0]
        if n < 2 or at + 2 + n > len(data):
            raise FormatError(f"segment {m:#x} at {at}: length {n} runs past the file")
        segs.append((m, data[at + 4:at + 2 + n], data[at:at + 2 + n]))
        at += 2 + n
        if m == 0xDA:
            return segs, at


def _parse_headers(segs, j):
    if not segs or segs[0][0] != 0xE0:
        raise FormatError("APP0 does not follow SOI")
    p = segs[0][1]
    if len(p) < 14 or p[:5] != b"JFIF\0":
        raise FormatError("APP0 is no JFIF segment")
    j.jfif = (p[5], p[6], p[7]) + struct.unpack_from(">HH", p, 8)
    if p[5] != 1 or len(p) != 14 + 3 * p[12] * p[13]:
        raise FormatError(f"JFIF version {p[5]}.{p[6]:02d}, segment of {len(p)} bytes")
    j.qtables, j.dht, j.dri = {}, {}, 0
    j.dqt_segments, j.dht_segments = [], []
    sof = sos = None
    for m, p, raw in segs[1:]:
        if m == 0xDB:
            j.dqt_segments.append(raw)
            at = 0
            if not p:
                raise FormatError("empty DQT")
            while at < len(p):
                pq, tq = p[at] >> 4, p[at] & 15
                if pq != 0 or tq > 3 or at + 65 > len(p):
                    raise FormatError(f"DQT: precision {pq}, table {tq}, {len(p) - at} bytes")
                q = np.frombuffer(p, np.uint8, 64, at + 1).astype(np.int64)
                if q.min() < 1:
                    raise FormatError("DQT: a quantiser of 0")
                nat = np.zeros(64, np.int64)
                nat[ZIGZAG] = q
                j.qtables[tq] = nat
                at += 65
        elif m == 0xC4:
            j.dht_segments.append(raw)
            at = 0
            if not p:
                raise FormatError("empty DHT")
            while at < len(p):
                if at + 17 > len(p):
                    raise FormatError("DHT: truncated")
                tc, th = p[at] >> 4, p[at] & 15
                bits = list(p[at + 1:at + 17])
                n = sum(bits)
                if tc > 1 or th > 1 or n == 0 or n > 256 or at + 17 + n > len(p):
                    raise FormatError(f"DHT: class {tc}, table {th}, {n} symbols")
                vals = list(p[at + 17:at + 17 + n])
                what = f"DHT {'AC' if tc else 'DC'} {th}"
                if len(set(vals)) != n:
                    raise FormatError(f"{what}: a symbol listed twice")
                for v in vals:
                    if tc == 0 and v > 11:
                        raise FormatError(f"{what}: magnitude category {v} above 11")
                    if tc == 1 and ((v & 15) > 10 or ((v & 15) == 0 and (v >> 4) not in (0, 15))):
                        raise FormatError(f"{what}: symbol {v:#04x} (category above 10, or a size of 0)")
                j.dht[(tc, th)] = _lut(bits, vals, what)
                at += 17 + n
        elif m == 0xDD:
            if len(p) != 2:
                raise FormatError("DRI length")
            j.dri = struct.unpack(">H", p)[0]
        elif m == 0xC0:
            if sof is not None:
                raise FormatError("a second SOF0")
            sof = p
        elif m == 0xDA:
            sos = p
        else:
            raise FormatError(f"marker {m:#x} is outside what this reader takes")
        if sos is not None and m != 0xDA:
            raise FormatError("segment after SOS")
    if sof is None or sos is None:
        raise FormatError("no SOF0 / SOS")
    if len(sof) < 6:
        raise FormatError("SOF0 length")
    j.precision, j.height, j.width, nf = struct.unpack_from(">BHHB", sof, 0)
    if j.precision != 8 or j.height == 0 or j.width == 0 or len(sof) != 6 + 3 * nf:
        raise FormatError(f"SOF0: precision {j.precision}, {j.width} x {j.height}, {nf} components, {len(sof)} bytes")
    j.components = [(sof[6 + 3 * i], sof[7 + 3 * i] >> 4, sof[7 + 3 * i] & 15, sof[8 + 3 * i]) for i in range(nf)]
    samp = [(h, v) for _, h, v, _ in j.components]
    if samp not in ([(1, 1)], [(2, 2), (1, 1), (1, 1)]):
        raise FormatError(f"sampling factors {samp}")
    if len({c[0] for c in j.components}) != nf:
        raise FormatError("component ids repeat")
    if len(sos) != 4 + 2 * nf or sos[0] != nf:
        raise FormatError(f"SOS: {sos[0] if sos else None} components in {len(sos)} bytes")
    j.scan = [(sos[1 + 2 * i], sos[2 + 2 * i] >> 4, sos[2 + 2 * i] & 15) for i in range(nf)]
    if tuple(sos[1 + 2 * nf:]) != (0, 63, 0):
        raise FormatError(f"SOS: spectral selection / approximation {tuple(sos[1 + 2 * nf:])}")
    if [s[0] for s in j.scan] != [c[0] for c in j.components]:
        raise FormatError("the scan's components are not the frame's, in order")
    for (_, _, _, tq), (_, td, ta) in zip(j.components, j.scan):
        if tq not in j.qtables or (0, td) not in j.dht or (1, ta) not in j.dht:
            raise FormatError(f"tables the scan names are not defined: Tq {tq}, Td {td}, Ta {ta}")


def _split_scan(data, at, j, n_intervals):
    """The entropy-coded segment from `at`: -> [(un-stuffed bytes, stuffed count)] per interval."""
    out, start, rst = [], at, 0
    find = data.find
    while True:
        k = find(b"\xff", at)
        if k < 0 or k + 1 >= len(data):
            raise FormatError("the scan runs to the end of the file: no EOI")
        b = data[k + 1]
        if b == 0:
            at = k + 2
            continue
        raw = data[start:k]
        if 0xD0 <= b <= 0xD7:
            if j.dri == 0:
                raise FormatError(f"RST{b - 0xD0} at {k} in a file without DRI")
            if b - 0xD0 != rst % 8:
                raise FormatError(f"RST{b - 0xD0} at {k} where RST{rst % 8} belongs")
            rst += 1
        elif b != 0xD9:
            raise FormatError(f"0xFF {b:#04x} at {k} inside an interval (marker, fill byte or un-stuffed 0xFF)")
        out.append((raw.replace(b"\xff\x00", b"\xff"), raw.count(b"\xff\x00")))
        if len(out) > n_intervals:
            raise FormatError(f"more than the {n_intervals} intervals the frame has MCUs for")
        at = start = k + 2
        if b == 0xD9:
            break
    if at != len(data):
        raise FormatError(f"{len(data) - at} bytes after EOI")
    if len(out) != n_intervals:
        raise FormatError(f"{len(out)} intervals, the frame has MCUs for {n_intervals}")
    return out


def _decode_interval(data, mcus, layout, zz_out, sym_out, bits_out, order, where):
    """Decode `mcus` = [(mx, my)] from one interval's un-stuffed bytes.
    layout: [(ci, h, v, dy, dx, dc_lut, ac_lut)] per block of an MCU.
    -> (pad_bits, last_byte)."""
    acc = n = pos = 0
    size = len(data)
    pred = {}
    for mx, my in mcus:
        for ci, h, v, dy, dx, dcl, acl in layout:
            by, bx = my * v + dy, mx * h + dx
            begin = 8 * pos - n
            zz = [0] * 64
            syms = []
            k = 0
            while k < 64:
                if n < 32:
                    while n <= 56 and pos < size:
                        acc = (acc << 8) | data[pos]
                        pos += 1
                        n += 8
                if n >= 16:
                    peek = (acc >> (n - 16)) & 0xFFFF
                else:  # virtual 1-bits past the end; a code that needs them is refused below
                    peek = ((acc << (16 - n)) | ((1 << (16 - n)) - 1)) & 0xFFFF
                e = (acl if k else dcl)[peek]
                ln = e >> 8
                if ln == 0:
                    raise FormatError(f"{where}, component {ci} block ({by}, {bx}), coefficient {k}: "
                                      f"bits {peek:016b} are no code of the table")
                if ln > n:
                    raise FormatError(f"{where}, component {ci} block ({by}, {bx}): the interval ends inside a code")
                n -= ln
                rs = e & 255
                r, s = rs >> 4, rs & 15
                if k == 0:
                    s, r = rs, 0
                    if s > 11:
                        raise FormatError(f"{where}: DC magnitude category {s}")
                elif s > 10:
                    raise FormatError(f"{where}: AC magnitude category {s}")
                syms.append((r, s))
                if s:
                    if s > n:
                        raise FormatError(f"{where}, component {ci} block ({by}, {bx}): "
                                          "the interval ends inside a magnitude")
                    n -= s
                    val = (acc >> n) & ((1 << s) - 1)
                    if val < (1 << (s - 1)):
                        val -= (1 << s) - 1
                    if k == 0:
                        val += pred.get(ci, 0)
                        pred[ci] = val
                    else:
                        k += r
                        if k > 63:
                            raise FormatError(f"{where}, component {ci} block ({by}, {bx}): "
                                              f"run of {r} passes coefficient 63")
                    zz[k] = val
                    k += 1
                elif k == 0:
                    pred.setdefault(ci, 0)
                    zz[0] = pred[ci]
                    k = 1
                elif r == 15:
                    k += 16
                    if k > 63:
                        raise FormatError(f"{where}, component {ci} block ({by}, {bx}): ZRL passes coefficient 63")
                elif r == 0:
                    k = 64
                else:
                    raise FormatError(f"{where}: AC symbol {rs:#04x}")
                acc &= (1 << n) - 1
            zz_out[ci][by, bx] = zz
            sym_out[ci][by][bx] = syms
            bits_out[ci][by, bx] = 8 * pos - n - begin
            order.append((ci, by, bx))
    if pos < size or n >= 8:
        raise FormatError(f"{where}: {size - pos + n // 8} whole bytes left after its last MCU")
    if acc != (1 << n) - 1:
        raise FormatError(f"{where}: padding bits {acc:0{n}b} are not 1-bits")
    return n, (data[-1] if size else None)


def read_jpeg(data):
    data = bytes(data)
    j = Jpeg()
    segs, at = _segments(data)
    _parse_headers(segs, j)
    colour = len(j.components) == 3
    mw = 16 if colour else 8
    mcux, mcuy = (j.width + mw - 1) // mw, (j.height + mw - 1) // mw
    total = mcux * mcuy
    per = j.dri if j.dri else total
    n_int = (total + per - 1) // per
    layout = []
    for ci, ((_, h, v, _), (_, td, ta)) in enumerate(zip(j.components, j.scan)):
        for dy in range(v):
            for dx in range(h):
                layout.append((ci, h, v, dy, dx, j.dht[(0, td)], j.dht[(1, ta)]))
    shapes = [(mcuy * v, mcux * h) for _, h, v, _ in j.components]
    zz = [np.zeros(s + (64,), np.int64) for s in shapes]
    syms = [[[None] * s[1] for _ in range(s[0])] for s in shapes]
    bits = [np.zeros(s, np.int64) for s in shapes]
    j.intervals, j.block_order = [], []
    for i, (raw, stuffed) in enumerate(_split_scan(data, at, j, n_int)):
        mcus = [(g % mcux, g // mcux) for g in range(i * per, min(total, (i + 1) * per))]
        j.block_order.append([])
        pad, last = _decode_interval(raw, mcus, layout, zz, syms, bits, j.block_order[-1], f"interval {i}")
        j.intervals.append({"bytes": len(raw), "stuffed": stuffed, "pad_bits": pad, "last_byte": last})
    j.coeffs = []
    for z in zz:
        nat = np.zeros_like(z)
        nat[..., ZIGZAG] = z
        j.coeffs.append(nat)
    j.symbols, j.block_bits = syms, bits
    return j


def segments_of(data, marker):
    """The raw bytes of every `marker` segment before the scan, in file order."""
    return [raw for m, _, raw in _segments(bytes(data))[0] if m == marker]
