"""The view settings (Filmic looks, Filmic Log, False Color, display gamma)
restated for the tests in numpy float32, one rounded operation a step, in the
order csrc/view_filmic.h, csrc/view.hip k_view and csrc/png16.hip Png16Sub
compute them. No test functions.

 - log2_fixed / exp2_fixed / display_gamma: the fixed polynomials by bit
   operations;
 - lut1d / lut3d_tetra: OCIO's linear and tetrahedral lookups in the device's
   operation order;
 - display: film means -> display-referred floats of a view, look and gamma at
   8 bits (the 8-bit sRGB table, read with a fused multiply-add as
   rr_device.h table_lerp does) or 16 bits (the finer table of the PNG path);
 - view8 / view16: the quantised images rr_debug_view_device and the 16-bit
   PNG front end form;
 - writers of synthetic look curves and a false-colour cube in the spi
   formats, next to host_oracle.write_synthetic_filmic_luts (the base pair),
   and load_luts, which reads a directory back through host_oracle's parsers.
"""
import os

import numpy as np

import color_modes as CM
import png16_reader as P
from oracle import host_oracle as HO

F32 = np.float32
I32 = np.int32

STANDARD, RAW, FILMIC, FILMIC_LOG, FALSE_COLOR = 0, 1, 2, 3, 4

# Blender 3.6's looks of the Filmic view and the file of each one's curve
# (None: the base curve, no file of its own)
LOOK_FILES = {
    "None": None,
    "Very High Contrast": "filmic_to_1.20_1-00.spi1d",
    "High Contrast": "filmic_to_0.99_1-0075.spi1d",
    "Medium High Contrast": "filmic_to_0-85_1-011.spi1d",
    "Medium Contrast": None,
    "Medium Low Contrast": "filmic_to_0-60_1-04.spi1d",
    "Low Contrast": "filmic_to_0-48_1-09.spi1d",
    "Very Low Contrast": "filmic_to_0-35_1-30.spi1d",
}
FALSE_COLOR_FILE = "filmic_false_color.spi3d"
GAMMAS = [0.2, 0.45, 0.7, 1.5, 2.2, 5.0]

# the edge values every crafted image carries (NaN is excluded: the device's
# fmaxf / fminf and its float -> int conversion of a NaN are not restated)
EDGES = np.array([0.0, -0.0, -1.0, -1e30, 1e-45, 1.17549435e-38, 1e-7, 0.0031308, 0.18, 0.5, 1.0, 1.0000001,
                  16.0, 65504.0, 1e30, np.inf, -np.inf], F32)


def _f(x):
    return np.ascontiguousarray(x, F32)


# ------------------------------------------------------ fixed polynomials --
def log2_fixed(x):
    """view_filmic.h log2_fixed."""
    x = _f(x)
    bits = x.view(I32)
    e = ((bits >> 23) & 0xFF) - 127
    m = ((bits & 0x007FFFFF) | 0x3F800000).astype(I32).view(F32)
    big = m > F32(1.41421356)
    m = np.where(big, m * F32(0.5), m).astype(F32)
    e = np.where(big, e + 1, e)
    t = (m - F32(1.0)) / (m + F32(1.0))
    t2 = t * t
    p = t2 * F32(0.111111112) + F32(0.142857149)
    p = p * t2 + F32(0.2)
    p = p * t2 + F32(0.333333343)
    p = p * t2 + F32(1.0)
    p = p * t
    return (e.astype(F32) + p * F32(2.88539004)).astype(F32)


def exp2_fixed(x):
    """view_filmic.h exp2_fixed."""
    x = _f(x)
    lo, hi = x < F32(-125.0), x >= F32(127.0)
    xs = np.where(lo | hi, F32(0.0), x).astype(F32)  # the middle branch's inputs only
    h = xs + F32(0.5)
    n = h.astype(I32)  # truncation, as the C cast
    n = np.where(n.astype(F32) > h, n - 1, n).astype(I32)
    f = xs - n.astype(F32)
    u = f * F32(0.693147182)
    p = u * F32(1.98412701e-4) + F32(1.38888892e-3)
    p = p * u + F32(8.33333377e-3)
    p = p * u + F32(4.16666679e-2)
    p = p * u + F32(0.166666672)
    p = p * u + F32(0.5)
    p = p * u + F32(1.0)
    p = p * u + F32(1.0)
    r = (np.ascontiguousarray(p, F32).view(I32) + n * I32(8388608)).astype(I32).view(F32)
    return np.where(lo, F32(0.0), np.where(hi, F32(1.70141183e38), r)).astype(F32)


def display_gamma(d, g):
    """view_filmic.h display_gamma with inv_g = 1.0f / g."""
    d = _f(d)
    inv = F32(1.0) / F32(g)
    pos = d > 0
    safe = np.where(pos, d, F32(1.0)).astype(F32)
    return np.where(pos, exp2_fixed(log2_fixed(safe) * inv), F32(0.0)).astype(F32)


def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays: the product is exact in float64, the sum
    is rounded to float64 and then to float32; where that first rounding lands
    on a tie of two float32 values, the sum's exact error (TwoSum) breaks it."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    tie = (np.ascontiguousarray(s).view(np.int64) & 0x1FFFFFFF) == 0x10000000
    s = np.where(tie & (err != 0), np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


# ----------------------------------------------------------------- lookups --
def _sat(x):
    return np.fmin(np.fmax(_f(x), F32(0.0)), F32(1.0))


def lut1d(curve, x, ch):
    """view_filmic.h lut1d over curve = {"lut1": (n, comps), "lo1", "hi1"}, for
    channel ch of a 3-component curve (a 1-component curve serves every channel)."""
    t = np.asarray(curve["lut1"], F32)
    n, comps = t.shape
    c = ch if comps == 3 else 0
    lo, hi = F32(curve["lo1"]), F32(curve["hi1"])
    with np.errstate(invalid="ignore", over="ignore"):
        f = (_f(x) - lo) / (hi - lo) * F32(n - 1)
    f = np.fmin(np.fmax(f, F32(0.0)), F32(n - 1)).astype(F32)
    i = f.astype(I32)
    top = i >= n - 1
    i = np.minimum(i, n - 2)
    fr = f - i.astype(F32)
    a, b = t[i, c], t[i + 1, c]
    return np.where(top, t[n - 1, c], a + (b - a) * fr).astype(F32)


def lut3d_tetra(cube, r, g, b):
    """view_filmic.h lut3d_tetra over cube (n, n, n, 3) indexed [red, green, blue]."""
    cube = np.asarray(cube, F32)
    n = cube.shape[0]
    s = F32(n - 1)
    fr, fg, fb = _sat(r) * s, _sat(g) * s, _sat(b) * s
    ir, ig, ib = (np.minimum(v.astype(I32), n - 2) for v in (fr, fg, fb))
    fr, fg, fb = fr - ir.astype(F32), fg - ig.astype(F32), fb - ib.astype(F32)
    one = F32(1.0)
    rg, gb, rb, bg, br = fr > fg, fg > fb, fr > fb, fb > fg, fb > fr
    cases = [rg & gb, rg & ~gb & rb, rg & ~gb & ~rb, ~rg & bg, ~rg & ~bg & br, ~rg & ~bg & ~br]
    c1o = [(1, 0, 0), (1, 0, 0), (0, 0, 1), (0, 0, 1), (0, 1, 0), (0, 1, 0)]
    c2o = [(1, 1, 0), (1, 0, 1), (1, 0, 1), (0, 1, 1), (0, 1, 1), (1, 1, 0)]
    ws = [(one - fr, fr - fg, fg - fb, fb), (one - fr, fr - fb, fb - fg, fg), (one - fb, fb - fr, fr - fg, fg),
          (one - fb, fb - fg, fg - fr, fr), (one - fg, fg - fb, fb - fr, fr), (one - fg, fg - fr, fr - fb, fb)]
    d1 = [np.select(cases, [o[a] for o in c1o]) for a in range(3)]
    d2 = [np.select(cases, [o[a] for o in c2o]) for a in range(3)]
    w = [np.select(cases, [x[k] for x in ws]).astype(F32) for k in range(4)]
    c000, c111 = cube[ir, ig, ib], cube[ir + 1, ig + 1, ib + 1]
    c1 = cube[ir + d1[0], ig + d1[1], ib + d1[2]]
    c2 = cube[ir + d2[0], ig + d2[1], ib + d2[2]]
    out = ((w[0][..., None] * c000 + w[1][..., None] * c1) + w[2][..., None] * c2) + w[3][..., None] * c111
    return out.astype(F32)


def filmic_log(luts, c):
    """view_filmic.h filmic_log: scene-linear (..., 3) -> Filmic Log."""
    c = _f(c)
    a = (log2_fixed(np.fmax(c, F32(1.17549435e-38))) + F32(12.473931188)) / F32(25.0)
    b = lut3d_tetra(luts["cube"], a[..., 0], a[..., 1], a[..., 2])
    return (b / F32(0.66)).astype(F32)


def srgb_oetf8(x, table):
    """rr_device.h srgb_oetf over the 8-bit path's table (intervals + 1 floats,
    oracle.srgb_lut()): table_lerp's read, with its fused multiply-add."""
    x = _f(x)
    t = np.asarray(table, F32)
    n = len(t)
    f = x * F32(n - 1)
    i = f.astype(I32)
    top = i >= n - 1
    i = np.clip(i, 0, n - 2)
    fr = f - i.astype(F32)
    lerp = fma32(t[i + 1] - t[i], fr, t[i])
    return np.where(x <= F32(0.0031308), x * F32(12.92), np.where(top, t[n - 1], lerp)).astype(F32)


# ----------------------------------------------------------- the chain ------
def curve_of(luts, look):
    """The 1D curve a Filmic frame with `look` reads: the look's, else the base."""
    look = look[len("Filmic - "):] if look.startswith("Filmic - ") else look
    return luts if LOOK_FILES[look] is None else luts["looks"][look]


def display(rgb, view, bits, luts=None, look="None", gamma=1.0, exposure_scale=1.0, table=None):
    """Film means (..., >= 3) -> display-referred float32 (..., 3) after the view
    transform and the display gamma, before BW luma and quantisation. bits 8:
    table = the 8-bit sRGB table (oracle.srgb_lut()); 16: rr.native.srgb16_table()."""
    c = (_f(rgb)[..., :3] * F32(1.0)) * F32(exposure_scale)
    if view in (STANDARD, RAW):
        d = np.fmin(np.fmax(c, F32(0.0)), F32(1.0)).astype(F32)
        if view == STANDARD:
            d = srgb_oetf8(d, table) if bits == 8 else P.srgb_oetf16(d, table)
    else:
        L = filmic_log(luts, c)
        if view == FILMIC_LOG:
            d = L
        elif view == FALSE_COLOR:
            pr, pg, pb = F32(0.2126729) * L[..., 0], F32(0.7151521) * L[..., 1], F32(0.0721750) * L[..., 2]
            y = (pr + pg) + pb
            d = lut3d_tetra(luts["fcube"], y, y, y)
        elif view == FILMIC:
            cv = curve_of(luts, look)
            d = np.stack([lut1d(cv, L[..., k], k) for k in range(3)], axis=-1)
        else:
            raise ValueError(view)
    if gamma != 1.0:
        d = display_gamma(d, gamma)
    return _f(d)


def quantize8(v):
    """rr_device.h quantize8."""
    v = _f(v)
    with np.errstate(invalid="ignore", over="ignore"):
        q = (v * F32(255.0) + F32(0.5)).astype(np.int64)
    return np.where(v <= 0, 0, np.where(v >= 1, 255, q)).astype(np.uint8)


quantize16 = P.quantize16


def view8(rgba, view, luts=None, look="None", gamma=1.0, exposure_scale=1.0, table=None):
    """(H, W, 4) float means -> (H, W, 4) uint8 as k_view writes it (alpha 255)."""
    q = quantize8(display(rgba, view, 8, luts, look, gamma, exposure_scale, table))
    return np.concatenate([q, np.full(q.shape[:-1] + (1,), 255, np.uint8)], axis=-1)


def view16(rgba, c, view, luts=None, look="None", gamma=1.0, exposure_scale=1.0, table=None):
    """(H, W, 4) float means -> (H, W, c) uint16 samples of the 16-bit PNG."""
    d = display(rgba, view, 16, luts, look, gamma, exposure_scale, table)
    if c == 1:
        return quantize16(CM.luma(d[..., 0], d[..., 1], d[..., 2]))[..., None]
    q = quantize16(d)
    if c == 3:
        return q
    return np.concatenate([q, np.full(q.shape[:-1] + (1,), 65535, np.uint16)], axis=-1)


# ------------------------------------------------------------ LUT files -----
def write_look_curve(directory, look, n1=257, comps=1, lo=-0.0625, hi=1.0625, seed=0):
    """A synthetic curve for `look` in the .spi1d format, distinct from the base
    curve host_oracle writes (another steepness, its own length and domain; with
    3 components a different curve a channel). Not monotone noise-free data: a
    small jitter makes neighbouring entries differ in every bit."""
    rng = np.random.default_rng(seed + 11)
    steep = 4.0 + 1.5 * list(LOOK_FILES).index(look)
    x = np.linspace(lo, hi, n1)
    cols = []
    for k in range(comps):
        cols.append(1.0 / (1.0 + np.exp(-steep * (x - 0.45 - 0.03 * k))) + rng.normal(0, 0.002, n1))
    os.makedirs(os.path.join(directory, "luts"), exist_ok=True)
    with open(os.path.join(directory, "luts", LOOK_FILES[look]), "w") as fh:
        fh.write(f"Version 1\nFrom {lo} {hi}\nLength {n1}\nComponents {comps}\n{{\n")
        for row in zip(*cols):
            fh.write("  " + " ".join(f"{v:.8f}" for v in row) + "\n")
        fh.write("}\n")


def write_false_color_cube(directory, n3=17, seed=0):
    """A synthetic false-colour cube in the .spi3d format: a hue ramp along the
    diagonal the view reads, distinct values off it."""
    rng = np.random.default_rng(seed + 23)
    os.makedirs(os.path.join(directory, "luts"), exist_ok=True)
    g = np.linspace(0.0, 1.0, n3)
    with open(os.path.join(directory, "luts", FALSE_COLOR_FILE), "w") as fh:
        fh.write(f"SPILUT 1.0\n3 3\n{n3} {n3} {n3}\n")
        for i in range(n3):
            for j in range(n3):
                for k in range(n3):
                    y = (g[i] + g[j] + g[k]) / 3.0
                    v = np.array([y * y, 4.0 * y * (1.0 - y), 1.0 - y]) + 0.1 * np.array([g[i], g[j], g[k]])
                    v = v + rng.normal(0, 0.003, 3)
                    fh.write(f"{i} {j} {k} {v[0]:.6f} {v[1]:.6f} {v[2]:.6f}\n")


def write_luts(directory, n3=17, n1=1024, looks=(), comps=1, false_color_n3=0, look_n1=257):
    """The base pair (host_oracle's writer) and, next to it, the given looks'
    curves and a false-colour cube of edge false_color_n3 (0: none)."""
    HO.write_synthetic_filmic_luts(directory, n3=n3, n1=n1)
    for k, look in enumerate(looks):
        write_look_curve(directory, look, n1=look_n1 + 16 * k, comps=comps, seed=k)
    if false_color_n3:
        write_false_color_cube(directory, false_color_n3)


def load_luts(directory):
    """What write_luts wrote, through host_oracle's parsers: load_filmic_luts'
    dict (cube, lut1, lo1, hi1) plus "looks" {name: curve} and "fcube"."""
    luts = HO.load_filmic_luts(directory)
    luts["looks"] = {}
    for look, name in LOOK_FILES.items():
        p = os.path.join(directory, "luts", name) if name else None
        if p and os.path.isfile(p):
            luts["looks"][look] = HO.parse_spi1d(p)
    p = os.path.join(directory, "luts", FALSE_COLOR_FILE)
    if os.path.isfile(p):
        luts["fcube"] = HO.parse_spi3d(p)
    return luts


# ----------------------------------------------------------- test images ----
def edge_image(w, h, seed=0):
    """(H, W, 4) float32: EDGES in every channel position and in mixed triples
    first, then the color_modes.float_image kinds in turn, cut to w * h pixels."""
    rng = np.random.default_rng(seed)
    px = []
    for v in EDGES:
        px.append([v, v, v])
    for _ in range(3 * len(EDGES)):
        px.append(list(rng.choice(EDGES, 3)))
    px = np.array(px, F32)
    parts = [px]
    total = len(px)
    k = 0
    while total < w * h:
        kind = CM.KINDS[k % len(CM.KINDS)]
        img = CM.float_image(kind, 61, 7, seed + k)[..., :3].reshape(-1, 3)
        if k % 2:
            img = img * F32(4.0 ** (k % 5) / 16.0)  # through the cube's whole log range
        parts.append(img)
        total += len(img)
        k += 1
    flat = np.concatenate(parts)[:w * h]
    out = np.zeros((h, w, 4), F32)
    out[..., :3] = flat.reshape(h, w, 3)
    out[..., 3] = rng.random((h, w), F32) * 2.0 - 0.5  # alpha junk the pass must ignore
    return out
