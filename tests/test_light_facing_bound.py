"""The bound of light_behind (csrc/rr_device.h), checked on the CPU: the rule
and the light branch of shade() restated in numpy float32 (tests/light_facing.py)
over 2^20 seeded configurations.

(a) Soundness. Wherever the rule holds, dot(N, wi) of the branch's float32 wi,
    evaluated in float64, is at most half of what the helper's comment claims
    (kLightBehindCos = -2^-11, so -2^-12): far below the 2^-21 a float32 dot3
    of unit vectors can be off by, so the computed cosN is negative and the
    skipped draw would have been discarded.
(b) Not vacuous. Among the configurations whose dot(N, wi) is below -2^-8 the
    rule holds in at least 99 %.

The configurations. Unit normals (normalised in float32, as the staged ones).
Population A, three quarters: in general position. A scale S, log-uniform
in [1e-2, 1e4]; P = S v with v uniform in [-1, 1]^3; the light at distance
d = S 2^U(-1, 3) in a direction whose cosine with N is uniform in [-1, 1/4];
radius 0 in one of eight, else min(1, d 2^U(-14, -5)). Population B, a quarter:
at the threshold. The light's centre at height -(radius (1 + slack) + t margin)
with t uniform in [-3, 5] (the rule holds from t = 1 on, up to rounding) and
radius 0 in one of eight, else uniform in (0, 1]. B1, 31 of 32 of B: d >= 2048
radius and |P| <= d / 8. B2, the rest: large coordinates, |P| up to 2^10 d, any
radius. Where radius > 0, half of the disk points are random and half are the
rim point highest along N, the one the slack has to cover.

Why (b) holds for these. The rule cannot hold while the disk reaches over the
plane: it misses a sample with dot(N, wi) < -2^-8 only if the centre's cosine
c is above -(radius + margin) / d while the sample's is below -2^-8. In A, c is
uniform over a range of 5/4, radius / d <= 2^-5 with a log-uniform mean of
0.005, and margin / d = 2^-10 (|lp|_1 + |P|_1 + radius) / d <= 2^-10 x 13.9
(|P|_1 <= 3 S <= 6 d, |lp|_1 <= |P|_1 + 1.74 d): the band of c that the rule
misses is at most 0.005 + 0.0136 - 2^-8 = 0.015 wide on average against the
0.996 that lies below -2^-8, and it is that wide only where S = 2 d. In B1 a
configuration the rule misses (t < 1) has every sample's cosine above
-(2 radius + margin) / d >= -(2^-10 + 2^-10 x 2.5) > -2^-8: none counts. B2 is
1/128 of all configurations, and fewer than half of them are missed. Together
below 1 %; the test prints the share it finds.
"""
import numpy as np

import light_facing as LF

F, D = np.float32, np.float64
N_CONF = 1 << 20


def unit32(v):
    v = v.astype(F)
    inv = F(1.0) / np.sqrt(LF.dot3(v, v))
    return v * inv[:, None]


def configurations(seed=20241):
    rng = np.random.default_rng(seed)
    n = N_CONF
    nb = n // 4          # population B
    nb2 = nb // 32       # its large-coordinate part
    is_b = np.arange(n) < nb
    is_b2 = np.arange(n) < nb2
    N = unit32(rng.normal(size=(n, 3)))
    Nd = N.astype(D)
    t0 = np.cross(Nd, rng.normal(size=(n, 3)))
    tang = t0 / np.linalg.norm(t0, axis=1)[:, None]   # a unit tangent (float64)
    v = rng.uniform(-1.0, 1.0, size=(n, 3))
    S = 10.0 ** rng.uniform(-2.0, 4.0, size=n)
    zero_r = rng.random(n) < 0.125

    # A
    d = S * 2.0 ** rng.uniform(-1.0, 3.0, size=n)
    radius = np.minimum(1.0, d * 2.0 ** rng.uniform(-14.0, -5.0, size=n))
    c = rng.uniform(-1.0, 0.25, size=n)
    P = S[:, None] * v
    # B
    rb = 1.0 - rng.random(n)  # (0, 1]
    radius = np.where(is_b, rb, radius)
    radius = np.where(zero_r, 0.0, radius)
    db1 = np.maximum(S, 2048.0 * radius) * 2.0 ** rng.uniform(0.0, 2.0, size=n)
    db2 = 10.0 ** rng.uniform(-2.0, 4.0, size=n)
    d = np.where(is_b, np.where(is_b2, db2, db1), d)
    pb2 = np.minimum(db2 * 2.0 ** rng.uniform(0.0, 10.0, size=n), 1.0e4)
    P = np.where(is_b[:, None], np.where(is_b2[:, None], pb2[:, None] * v, (db1 / 8.0)[:, None] * v), P)
    P = P.astype(F)
    Pd = P.astype(D)
    lp0 = Pd + d[:, None] * tang
    m0 = np.abs(lp0).sum(1) + np.abs(Pd).sum(1) + radius
    t = rng.uniform(-3.0, 5.0, size=n)
    for _ in range(2):  # the margin depends on |lp|_1, which the height moves (where radius is not small against d)
        hb = -(radius * (1.0 + float(LF.SLACK)) + t * float(LF.MARGIN) * m0)
        lp_b = lp0 + hb[:, None] * Nd
        m0 = np.abs(lp_b).sum(1) + np.abs(Pd).sum(1) + radius
    lp_a = Pd + d[:, None] * (c[:, None] * Nd + np.sqrt(1.0 - c * c)[:, None] * tang)
    lp = np.where(is_b[:, None], lp_b, lp_a).astype(F)
    radius = radius.astype(F)

    # disk points: random, or the rim point highest along N
    u1 = (rng.integers(0, 65536, size=n) / 65536.0).astype(F)
    u2 = (rng.integers(0, 65536, size=n) / 65536.0).astype(F)
    _, b1, b2 = LF.light_frame(P, lp)
    with np.errstate(invalid="ignore"):
        phi = np.arctan2((b2.astype(D) * Nd).sum(1), (b1.astype(D) * Nd).sum(1))
    a1, a2 = LF.rim_uv(np.nan_to_num(phi))
    worst = rng.random(n) < 0.5
    u1, u2 = np.where(worst, a1, u1), np.where(worst, a2, u2)
    return N, P, lp, radius, u1, u2, is_b, is_b2


def test_light_behind_bound():
    N, P, lp, radius, u1, u2, is_b, is_b2 = configurations()
    assert len(N) >= 10 ** 6
    for x in (P, lp):  # the magnitudes asked for are there
        mag = np.abs(x).max(1)
        assert mag.min() < 2e-2 and mag.max() > 1e4 * 0.5
    assert radius.min() == 0.0 and radius.max() == 1.0
    fired = LF.light_behind(N, P, lp, radius)
    wi = LF.light_wi(P, lp, radius, u1, u2)
    cos = (N.astype(D) * wi.astype(D)).sum(1)
    assert np.isfinite(cos).all()
    # the configurations at the threshold sit on both sides of it, within a few margins
    h = (N.astype(D) * (lp.astype(D) - P.astype(D))).sum(1)
    over = (-h - radius.astype(D) * (1.0 + float(LF.SLACK))) / LF.margin(P, lp, radius)
    assert np.all((over[is_b] > -3.1) & (over[is_b] < 5.1))
    for part in (is_b & ~is_b2, is_b2):
        share = fired[part].mean()
        print("threshold population: fired", share)
        assert 0.4 < share < 0.6
    # and the rule switches where its statement says: t = 1 (to within 2^-6 of a margin)
    assert fired[is_b & (over > 1.0 + 2.0 ** -6)].all() and not fired[is_b & (over < 1.0 - 2.0 ** -6)].any()

    # (a)
    worst = cos[fired].max()
    print("fired", int(fired.sum()), "of", len(fired), "largest dot(N, wi) where fired", worst,
          "claimed", LF.BEHIND_COS)
    assert fired.sum() > len(fired) // 4
    assert worst <= 0.5 * LF.BEHIND_COS

    # (b)
    clear = cos < -2.0 ** -8
    share = fired[clear].mean()
    print("dot(N, wi) < -2^-8:", int(clear.sum()), "fired in", share)
    assert clear.sum() > len(fired) // 2
    assert share >= 0.99


def test_never_fires_in_front():
    """A light whose centre is not behind the plane is never skipped, whatever
    the magnitudes (the right side of the rule is negative)."""
    N, P, lp, radius, _, _, _, _ = configurations(seed=7)
    h = LF.dot3(N, lp - P)
    fired = LF.light_behind(N, P, lp, radius)
    assert not fired[h >= 0].any()
    # NaN coordinates compare false
    bad = lp.copy()
    bad[:, 0] = np.nan
    assert not LF.light_behind(N, P, bad, radius).any()


def test_radius_not_above_zero_is_the_point_light():
    """The branch draws on a disk only where radius > 0; a negative radius (the
    scene loader passes one on) or a NaN is the plain point light, for the
    rule too: it fires exactly where it fires at radius 0, and (a) holds."""
    N, P, lp, radius, u1, u2, _, _ = configurations(seed=11)
    n = 1 << 17
    N, P, lp, u1, u2 = N[:n], P[:n], lp[:n], u1[:n], u2[:n]
    rng = np.random.default_rng(5)
    neg = (-(10.0 ** rng.uniform(-3.0, 2.0, size=n))).astype(F)
    neg[::7] = np.nan
    neg[1::7] = F(-0.0)
    zero = np.zeros(n, F)
    fired = LF.light_behind(N, P, lp, neg)
    assert np.array_equal(fired, LF.light_behind(N, P, lp, zero))
    assert 0.05 < fired.mean() < 0.95
    with np.errstate(invalid="ignore"):
        wi = LF.light_wi(P, lp, neg, u1, u2)
    assert np.array_equal(wi, LF.light_wi(P, lp, zero, u1, u2))
    cos = (N.astype(D) * wi.astype(D)).sum(1)
    assert cos[fired].max() <= 0.5 * LF.BEHIND_COS
    # a light half a unit in front of the surface with radius -1: not skipped
    one = lambda *v: np.array([v], F)
    assert not LF.light_behind(one(0, 0, 1), one(0, 0, 0), one(0, 0, 0.5), np.array([-1.0], F))[0]
