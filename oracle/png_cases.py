"""TEST INFRASTRUCTURE ONLY — crafted inputs of the device PNG encoder's tests.

Every generator returns the filtered stream (H, 4W + 1) it wants the encoder
to see; image_of() turns it into the image (png_oracle.image_from_filtered).
tests/test_png_oracle.py proves on the CPU, with png_oracle's reference parse,
that each input reaches the edge it is named after; tests/test_gpu_png_tokens.py
imports the same functions and seeds."""
from __future__ import annotations

import numpy as np

from oracle import png_oracle as P

# Widths of the distance sweep: 4W = stride - 1 walks the distance symbols 4 and
# 6..29 (symbol 5 is the distances 7 and 8; no 4W + 1 is either, and the fixed
# distances 1 and 4 are the symbols 0 and 3). 8191 is the last width whose row
# above lies inside the 32 KB window (distance 32765), 8192 the first beyond it.
_SWEEP_BASE = [1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048, 3072,
               4096, 6144, 8191]
DIST_SWEEP_WIDTHS = sorted(set(_SWEEP_BASE) | {w - 1 for w in _SWEEP_BASE if w >= 4})
DIST_SWEEP_BEYOND = 8192
DIST_SWEEP_TALL = [(1, 16), (2, 16), (3, 16)]  # (W, H): bands long enough to be dynamic at the shortest strides

LENGTH_SWEEP_SHAPE = (1023, 48)  # stride 4093 <= 4096: a 3-byte match at the stride still counts
LL_LIMIT_SHAPE = (2100, 16)
CL_LIMIT_SHAPE = (300, 16)
MIXED_SHAPE = (300, 53)


def image_of(f):
    h, s = f.shape
    return P.image_from_filtered(f, (s - 1) // 4, h)


def _noise_rows(rng, W, H):
    f = rng.integers(0, 256, (H, 4 * W + 1), dtype=np.uint8)
    f[:, 0] = 1
    return f


def kind_image(kind, w, h, seed=0):
    """The image kinds of tests/test_gpu_png.py (noise4: random alpha too)."""
    rng = np.random.default_rng(seed)
    if kind in ("noise", "noise4"):
        a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    elif kind == "flat":
        a = np.full((h, w, 4), 77, np.uint8)
    elif kind == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) % 256), np.full_like(x, 255)],
                     -1).astype(np.uint8)
    elif kind == "sparse":
        a = np.full((h, w, 4), 128, np.uint8)
        m = rng.random((h, w)) < 0.01
        a[m, :3] = 255
    else:
        raise ValueError(kind)
    if kind != "noise4":
        a[..., 3] = 255
    return a


def band_rows(H, W=37, seed=5):
    """Rows that repeat the row above but for a few bytes, drawn from 8 values:
    in every band's first row a match into the previous band would pay."""
    rng = np.random.default_rng(seed)
    s = 4 * W + 1
    f = np.empty((H, s), np.uint8)
    row = rng.integers(0, 8, s, dtype=np.uint8) * 31
    for r in range(H):
        row = row.copy()
        at = rng.integers(1, s, 3)
        row[at] = rng.integers(0, 8, 3, dtype=np.uint8) * 31
        f[r] = row
    f[:, 0] = 1
    return f


def dist_sweep(W, H=3, seed=11):
    """W x H, identical noise rows: the rows below the first are matches at the stride."""
    rng = np.random.default_rng(seed + W)
    return np.repeat(_noise_rows(rng, W, 1), H, axis=0)


def far_threshold(W, seed=13, every=40):
    """Noise rows in cells of 40 columns: 3 bytes of each cell repeat the row
    above, the bytes on either side differing (row matches of exactly 3 bytes);
    the cell's last 32 bytes are zero in every row, so that the band compresses
    and stays dynamic on both sides of the threshold."""
    rng = np.random.default_rng(seed)
    H = 4
    f = _noise_rows(rng, W, H)
    s = 4 * W + 1
    cells = range(8, s - every, every)
    for c in cells:
        f[:, c + 8:c + every] = 0
    for r in range(1, H):
        for c in cells:
            f[r, c:c + 3] = f[r - 1, c:c + 3]
            f[r, c - 1] = f[r - 1, c - 1] ^ 0x55
            f[r, c + 3] = f[r - 1, c + 3] ^ 0xAA
    return f


def length_sweep(seed=3):
    """Every match length 3..258 at each of the distances 1, 4 and the stride,
    then further matches of random lengths until the rows are full, so that
    most 512-position segments of the parse are entered inside a match.

    Columns 1..split-1 of every row hold runs of one byte (distance 1) and of a
    4-byte period (distance 4); the columns from split on hold copies of the row
    above, in every row but a band's first. Each event is led by one byte that
    ends the event before it. Band 0's row 0 starts with a 258-byte run placed
    so that it begins at position 511: the parse enters segment 1 at 257."""
    W, H = LENGTH_SWEEP_SHAPE
    rng = np.random.default_rng(seed)
    s = 4 * W + 1
    split = 2 * s // 3
    f = _noise_rows(rng, W, H)
    lengths = list(range(P.MIN_MATCH, P.MAX_MATCH + 1))
    near = [(d, ln) for d in (1, 4) for ln in lengths]
    far = list(lengths)
    rng.shuffle(near)
    rng.shuffle(far)

    def lead(r, c, avoid):  # a byte at (r, c) that differs from every value in avoid
        v = int(rng.integers(0, 256))
        while v in avoid:
            v = (v + 1) & 0xFF
        f[r, c] = v

    for r in range(H):
        c, end_prev = 1, set()
        if r == 0:  # positions 1..508 stay noise; lead at 509, the run's 259 bytes from 510, the match from 511
            c = 509
            near.insert(0, (1, 258))
        while True:
            if not near:
                near.append((int(rng.choice([1, 4])), int(rng.integers(P.MIN_MATCH, P.MAX_MATCH + 1))))
            d, ln = near[0]
            need = 1 + ln + d + 1  # lead, body, and the byte that ends it
            if c + need > split:
                break
            near.pop(0)
            if d == 1:
                v = int(rng.integers(0, 256))
                lead(r, c, end_prev | {v})
                f[r, c + 1:c + 2 + ln] = v
                end_prev = {v}
            else:
                p = rng.choice(256, 4, replace=False).astype(np.uint8)
                lead(r, c, end_prev | {int(x) for x in p})
                body = np.tile(p, (ln + 4 + 3) // 4)[:ln + 4]
                f[r, c + 1:c + 5 + ln] = body
                end_prev = {int(p[(ln + 4) % 4])}
            c += 1 + ln + d
        lead(r, c, end_prev)
        if r % P.BAND_ROWS == 0:
            continue
        c = split
        while True:
            if not far:
                far.append(int(rng.integers(P.MIN_MATCH, P.MAX_MATCH + 1)))
            ln = far[0]
            if c + 1 + ln + 1 > s:
                break
            far.pop(0)
            lead(r, c, {int(f[r - 1, c])})
            f[r, c + 1:c + 1 + ln] = f[r - 1, c + 1:c + 1 + ln]
            c += 1 + ln
            lead(r, c, {int(f[r - 1, c])})  # ends the copy; the next event's lead overwrites it alike
    return f


def _fill(rng, values, counts, W, H):
    """Free bytes of a W x H stream: each value counts[k] times, the rest drawn
    from the same distribution, all shuffled."""
    free = 4 * W * H
    base = np.repeat(np.asarray(values, np.uint8), counts)
    assert base.size <= free
    p = np.asarray(counts, np.float64) / np.sum(counts)
    rest = rng.choice(np.asarray(values, np.uint8), free - base.size, p=p)
    body = np.concatenate([base, rest])
    rng.shuffle(body)
    f = np.empty((H, 4 * W + 1), np.uint8)
    f[:, 0] = 1
    f[:, 1:] = body.reshape(H, 4 * W)
    return f


def ll_limit(seed=17):
    """18 byte values with the counts 1, 1, 2, 4, ..., 2^16: the literal/length
    tree of such a band wants more than 15 bits for the rarest."""
    W, H = LL_LIMIT_SHAPE
    rng = np.random.default_rng(seed)
    values = [3 + 7 * k for k in range(18)]  # none is the filter byte 1
    counts = [1] + [1 << k for k in range(17)]
    return _fill(rng, values, counts, W, H)


# Code-length classes of the code-length limit case: (length l, how many of the
# 257 symbols 0..256 are meant to get it). The counts 3, 5, 8, 13, 21, 34, 55
# grow like Fibonacci numbers and the last class completes the Kraft sum
# (3/8 + 5/32 + 8/64 + 13/128 + 21/256 + 34/512 + 55/1024 + 118/2048 = 1.017:
# the end-of-block symbol and a few others slip one bit deeper).
CL_CLASSES = [(3, 3), (5, 5), (6, 8), (7, 13), (8, 21), (9, 34), (10, 55), (11, 118)]


def _no_long_runs(classes):
    """The classes' lengths as one sequence without three equal neighbours, so
    that no code-length run is long enough for a repeat symbol."""
    left = dict(classes)
    seq = []
    while any(left.values()):
        for l in sorted(left, key=lambda k: -left[k]):
            if left[l] and not (len(seq) >= 2 and seq[-1] == l and seq[-2] == l):
                seq.append(l)
                left[l] -= 1
                break
        else:
            raise ValueError("classes cannot be interleaved")
    return seq


def cl_limit(seed=19):
    """All 256 byte values occur, value v about 19216 / 2^l times for its class
    length l (the issue's recipe: 2^(12-l)-like counts, Fibonacci many values
    per length), no three neighbouring values in one class, and the bytes are
    swapped about until the reference parse finds no match: the code lengths
    are then written one token each, their counts are the class sizes, and a
    tree over 2, 2, 3, 5, 8, 13, 21, 34, 55, 118 wants more than 7 bits."""
    W, H = CL_LIMIT_SHAPE
    rng = np.random.default_rng(seed)
    s = 4 * W + 1
    seq = _no_long_runs(CL_CLASSES)

    def pin(pos, want):  # symbol pos gets class want
        k = next(i for i, l in enumerate(seq) if l == want and i not in (1, 256))
        seq[k], seq[pos] = seq[pos], seq[k]

    pin(256, 11)  # end of block: once
    pin(1, 10)    # the filter byte: 16 times
    counts = [max(1, round(s * H * 2.0 ** -l)) for l in seq[:256]]
    counts[1] = 0  # the rows' first bytes are not free
    counts[seq.index(3)] += 4 * W * H - sum(counts)
    body = np.repeat(np.arange(256, dtype=np.uint8), counts)
    rng.shuffle(body)
    f = np.empty((H, s), np.uint8)
    f[:, 0] = 1
    f[:, 1:] = body.reshape(H, 4 * W)
    flat = f.reshape(-1)
    for _ in range(100):
        pos, hits = 0, []
        for t in P.greedy_tokens(flat.tobytes(), s):
            if isinstance(t, tuple):
                hits.append(pos)
                pos += t[0]
            else:
                pos += 1
        if not hits:
            return f
        for p in hits:  # break the match: its second byte changes places with a free byte elsewhere
            a = p + 1 if (p + 1) % s else p + 2
            b = int(rng.integers(0, flat.size))
            while b % s == 0:
                b = int(rng.integers(0, flat.size))
            flat[a], flat[b] = flat[b], flat[a]
    raise RuntimeError("matches left")


def mixed(seed=23):
    """300 x 53: rows 0-15 noise with random alpha, 16-31 flat, 32-47 noise, 48-52 a gradient."""
    W, H = MIXED_SHAPE
    img = np.empty((H, W, 4), np.uint8)
    img[0:16] = kind_image("noise4", W, 16, seed)
    img[16:32] = kind_image("flat", W, 16)
    img[32:48] = kind_image("noise4", W, 16, seed + 1)
    img[48:53] = kind_image("gradient", W, 5)
    return img
