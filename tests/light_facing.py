"""numpy float32 restatement of light_behind (csrc/rr_device.h) and of the
point / disk light branch of shade() (csrc/paths.hpp) up to wi. Not a test.
Written from the helper's comment and the branch's text, operation by
operation in float32 over arrays of configurations.

fmaf is formed through float64 (the product of two floats is exact there; the
sum is rounded to double, then to float): in rare double-rounding cases the
last bit differs from the device's single rounding, 2^-24 relative, which is
below everything the bound is compared with."""
from __future__ import annotations

import numpy as np

F = np.float32
D = np.float64

SLACK = F(2.0 ** -10)        # kLightSlack
MARGIN = F(2.0 ** -10)       # kLightMargin
BEHIND_COS = -0.5 * 2.0 ** -10  # kLightBehindCos: what the helper's comment claims of dot(N, wi) where the rule holds


def fma(a, b, c):
    return (a.astype(D) * b.astype(D) + c.astype(D)).astype(F)


def dot3(a, b):
    """fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); vectors are (n, 3) arrays"""
    return fma(a[:, 2], b[:, 2], fma(a[:, 1], b[:, 1], a[:, 0] * b[:, 0]))


def light_behind(N, P, lp, radius):
    radius = np.where(radius > 0, radius, F(0.0)).astype(F)  # fmaxf(radius, 0): not above 0, or NaN, is the point light
    h = dot3(N, lp - P)
    m = (np.abs(lp[:, 0]) + np.abs(lp[:, 1]) + np.abs(lp[:, 2])) + (np.abs(P[:, 0]) + np.abs(P[:, 1]) + np.abs(P[:, 2]))
    return h <= -fma(np.full_like(m, MARGIN), m, radius * (F(1.0) + SLACK + MARGIN))


def margin(P, lp, radius):
    """The rule's margin k (|lp|_1 + |P|_1 + radius), in float64."""
    return float(MARGIN) * (np.abs(lp.astype(D)).sum(1) + np.abs(P.astype(D)).sum(1) + radius.astype(D))


def sqrt_rcp(x):
    s = np.sqrt(x)  # IEEE, as sqrtf
    return s, F(1.0) / s


def sincos_small(x):
    z = x * x
    ps = fma(fma(np.full_like(z, F(-1.9515295891e-4)), z, np.full_like(z, F(8.3321608736e-3))), z,
             np.full_like(z, F(-1.6666654611e-1)))
    s = fma(ps * z, x, x)
    pc = fma(fma(np.full_like(z, F(2.443315711809948e-5)), z, np.full_like(z, F(-1.388731625493765e-3))), z,
             np.full_like(z, F(4.166664568298827e-2)))
    c = fma(pc * z, z, fma(np.full_like(z, F(-0.5)), z, np.full_like(z, F(1.0))))
    return s, c


def concentric_disk(u1, u2):
    two, one = np.full_like(u1, F(2.0)), np.full_like(u1, F(-1.0))
    a, b = fma(two, u1, one), fma(two, u2, one)
    wide = np.abs(a) > np.abs(b)
    num, r = np.where(wide, b, a), np.where(wide, a, b)
    origin = (a == 0) & (b == 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        s, c = sincos_small(F(0.785398163397448) * (num / r))
    x = np.where(origin, F(0.0), r * np.where(wide, c, s))
    y = np.where(origin, F(0.0), r * np.where(wide, s, c))
    return x.astype(F), y.astype(F)


def make_onb(n):
    sign = np.copysign(F(1.0), n[:, 2])
    a = -(F(1.0) / (sign + n[:, 2]))
    b = n[:, 0] * n[:, 1] * a
    one = np.full_like(a, F(1.0))
    b1 = np.stack([fma(sign * n[:, 0] * n[:, 0], a, one), sign * b, -sign * n[:, 0]], 1)
    b2 = np.stack([b, fma(n[:, 1] * n[:, 1], a, sign), -n[:, 1]], 1)
    return b1.astype(F), b2.astype(F)


def madd3(a, b, s):
    return np.stack([fma(b[:, k], s, a[:, k]) for k in range(3)], 1)


def light_frame(P, lp):
    """wl and the disk's frame b1, b2, as the disk case forms them."""
    tl = lp - P
    _, rl = sqrt_rcp(dot3(tl, tl))
    wl = tl * rl[:, None]
    return (wl,) + make_onb(wl)


def light_wi(P, lp, radius, u1, u2):
    """wi of the branch: the disk case where radius > 0 (the disk point of
    (u1, u2)), the plain point light's for every other radius."""
    tl = lp - P
    _, b1, b2 = light_frame(P, lp)
    dx, dy = concentric_disk(u1, u2)
    dx, dy = dx * radius, dy * radius
    sp = madd3(madd3(lp, b1, dx), b2, dy)
    ts = np.where((radius > 0)[:, None], sp - P, tl).astype(F)
    _, idist = sqrt_rcp(dot3(ts, ts))
    return ts * idist[:, None]


def rim_uv(phi):
    """(u1, u2) on the RNG's 2^-16 grid whose disk point lies on the rim at
    angle phi (float64, in [-pi, pi]): concentric_disk inverted."""
    q = np.pi / 4
    a = np.where(np.abs(phi) <= q, 1.0, np.where(np.abs(phi) >= 3 * q, -1.0,
                 np.where(phi > 0, (2 * q - phi) / q, (phi + 2 * q) / q)))
    b = np.where(np.abs(phi) <= q, phi / q, np.where(phi >= 3 * q, (np.pi - phi) / q,
                 np.where(phi <= -3 * q, (-np.pi - phi) / q, np.where(phi > 0, 1.0, -1.0))))

    def grid(v):
        return (np.clip(np.floor((v + 1.0) * 0.5 * 65536.0), 0, 65535) / 65536.0).astype(F)
    return grid(a), grid(b)
