"""numpy float32 restatement of the 8-bit dither (rr_set_dither): the fixed
sine, the per-pixel noise and the quantiser. Not a test. Written from the
rule's statement (include/rr.h rr_set_dither, csrc/dither.h's header comment),
operation by operation in float32, so the library's host and device code can
be compared with it bit for bit."""
from __future__ import annotations

import numpy as np

F = np.float32

AX, AY, AM = F(12.9898), F(78.233), F(43758.5453)
BX, BY, BM = F(19.9898), F(119.233), F(798.5453)
SCALE = F(0.0033)

TWO_OVER_PI = F(0.636619747)
PIO2_1, PIO2_2, PIO2_3 = F(1.5703125), F(4.83751297e-4), F(7.54978996e-8)
S1, S2, S3 = F(-1.95152959e-4), F(8.33216123e-3), F(0.166666552)
C1, C2, C3 = F(2.44331568e-5), F(1.38873165e-3), F(4.16666456e-2)


def sin_fixed(a: np.ndarray) -> np.ndarray:
    """a = n pi/2 + r, n the nearest integer, pi/2 in three parts; sin r by
    its odd polynomial to r^7 or cos r by its even one to r^8, picked and
    signed by n mod 4. 0 outside |a| <= 8192."""
    a = np.asarray(a, dtype=F)
    ok = np.abs(a) <= F(8192.0)
    a0 = np.where(ok, a, F(0.0)).astype(F)
    h = a0 * TWO_OVER_PI + F(0.5)
    n = h.astype(np.int32)  # truncates toward zero, as the C cast does
    n = np.where(n.astype(F) > h, n - 1, n).astype(np.int32)
    fn = n.astype(F)
    r = ((a0 - fn * PIO2_1) - fn * PIO2_2) - fn * PIO2_3
    z = r * r
    c = ((C1 * z - C2) * z + C3) * z * z - F(0.5) * z + F(1.0)
    s = ((S1 * z + S2) * z - S3) * z * r + r
    v = np.where((n & 1) != 0, c, s).astype(F)
    v = np.where((n & 2) != 0, F(0.0) - v, v).astype(F)
    return np.where(ok, v, F(0.0)).astype(F)


def hash_args(w: int, h: int):
    """The arguments of the two sines for every pixel, (h, w) each, rows top
    to bottom (row r uses yb = h - 1 - r)."""
    inv_w = F(1.0) / F(w)
    inv_h = F(1.0) / F(h)
    x = np.arange(w, dtype=np.int32).astype(F)[None, :]
    yb = (h - 1 - np.arange(h, dtype=np.int32)).astype(F)[:, None]
    s = x * inv_w
    t = yb * inv_h
    return (s * AX + t * AY).astype(F), (s * BX + t * BY).astype(F)


def noise(w: int, h: int) -> np.ndarray:
    """n of every pixel, (h, w) float32, rows top to bottom."""
    a0, a1 = hash_args(w, h)
    h0 = sin_fixed(a0) * AM
    h0 = h0 - np.floor(h0)
    h1 = sin_fixed(a1) * BM
    h1 = h1 - np.floor(h1)
    return (h0 + h1 - F(0.5)).astype(F)


def quantize8(v: np.ndarray) -> np.ndarray:
    v = np.asarray(v, dtype=F)
    q = (np.clip(v, F(0.0), F(1.0)) * F(255.0) + F(0.5)).astype(np.uint8)
    return np.where(v <= 0, 0, np.where(v >= 1, 255, q)).astype(np.uint8)


def dither_codes(d: np.ndarray, intensity: float) -> np.ndarray:
    """d: (h, w, 3) float32 display-referred values (after view transform and
    display gamma). Returns (h, w, 4) uint8: quantize8(d + dv), alpha 255."""
    d = np.asarray(d, dtype=F)
    h, w = d.shape[:2]
    dv = noise(w, h) * SCALE * F(intensity)
    out = np.empty((h, w, 4), np.uint8)
    out[..., :3] = quantize8(d[..., :3] + dv[..., None])
    out[..., 3] = 255
    return out
