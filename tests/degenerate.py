"""Degenerate and boundary-size scenes for the device hierarchy build and walks
(test infrastructure, in the style of soups.py).

Every generator returns (n, 3, 3) float32 triangles in the 04vs cube's object
space from a fixed seed; `scene` writes them as a copy of the 04vs stand-in
.rrscene with the mesh replaced (soups.soup_scene). The cube's object transform
is a pure translation (identity rotation, unit scale), so identical triangles
stay identical in world space and axis-aligned flatness survives exactly;
`check_property` asserts that on the world triangles a test is about to use.

The ray batches (`rays`, `packet_rays`, `edge_rays`) are functions of the world
triangles and the case name alone, so the CPU test of the oracle
(test_oracle.py) and the device tests (test_gpu_degenerate.py) trace the same
rays.
"""
from __future__ import annotations

import zlib

import numpy as np

import soups

RAND_SIZES = (15, 16, 17, 31, 32, 33, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 2049, 4096, 4097)
BUILD_ONLY = ("rand20000",)  # hierarchy checks only (no ray batch)
DEGENERATE = ("n1", "n2", "n3", "same50", "same600", "coplanar700", "coplanar40", "line40", "point20",
              "zeroarea300", "outlier1500")
TRACE_CASES = DEGENERATE + tuple(f"rand{n}" for n in RAND_SIZES)
CASES = TRACE_CASES + BUILD_ONLY
NO_AREA = ("line40", "point20")  # no triangle of non-zero area: nothing can be hit


def _seed(name: str) -> int:
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def _rand(rng, n):
    c = rng.uniform(-1.0, 1.0, (n, 1, 3))
    return (c + rng.normal(0.0, 0.1, (n, 3, 3))).astype(np.float32)


def triangles(name: str) -> np.ndarray:
    rng = np.random.default_rng(_seed(name))
    if name in ("n1", "n2", "n3"):
        c = rng.uniform(-0.5, 0.5, (int(name[1:]), 1, 3))
        t = c + rng.normal(0.0, 0.4, (int(name[1:]), 3, 3))
    elif name.startswith("same"):
        t = np.repeat(rng.uniform(-0.8, 0.8, (1, 3, 3)), int(name[4:]), axis=0)
    elif name.startswith("coplanar"):
        n = int(name[8:])
        t = rng.uniform(-1.0, 1.0, (n, 1, 3)) + rng.normal(0.0, 0.15, (n, 3, 3))
        t[..., 2] = 0.25
    elif name == "line40":
        t = np.zeros((40, 3, 3))
        t[..., 0] = rng.uniform(-1.0, 1.0, (40, 3))
    elif name == "point20":
        t = np.broadcast_to(rng.uniform(-0.5, 0.5, 3), (20, 3, 3)).copy()
    elif name == "zeroarea300":
        t = _rand(rng, 300).astype(np.float64)
        t[0::3, 1] = t[0::3, 0]                      # two equal vertices
        t[1::3, 1] = t[1::3, 2] = t[1::3, 0]         # three equal vertices
    elif name == "outlier1500":
        t = rng.uniform(-1.0, 1.0, (1500, 1, 3)) + rng.normal(0.0, 0.1, (1500, 3, 3))
        t[-1] += 1.0e6
    elif name.startswith("rand"):
        t = _rand(rng, int(name[4:]))
    else:
        raise KeyError(name)
    return np.ascontiguousarray(t, dtype=np.float32)


def scene_dict(base_scene_path: str, name: str) -> dict:
    return soups.soup_scene_dict(base_scene_path, name, tris=triangles(name))


def scene(base_scene_path: str, name: str, out_path: str) -> np.ndarray:
    return soups.soup_scene(base_scene_path, name, out_path, tris=triangles(name))


def cluster(name: str, tris: np.ndarray) -> np.ndarray:
    """The triangles the ray batches are aimed at (all but outlier1500's outlier)."""
    return tris[:-1] if name == "outlier1500" else tris


def zero_area(tris: np.ndarray) -> np.ndarray:
    t = tris.astype(np.float64)
    return np.all(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]) == 0.0, axis=1)


def morton_keys(tris: np.ndarray) -> np.ndarray:
    """30-bit Morton keys of the centroid sums, float32 op for op as k_morton
    (unsorted, one per triangle)."""
    t = tris.astype(np.float32)
    c = (t[:, 0] + t[:, 1]) + t[:, 2]
    lo, hi = c.min(0), c.max(0)
    ext = (hi - lo).astype(np.float32)
    with np.errstate(divide="ignore"):
        s = np.where(ext > 0, np.float32(1024.0) / ext, np.float32(0.0)).astype(np.float32)
    q = np.clip(((c - lo).astype(np.float32) * s).astype(np.float32), 0.0, 1023.0).astype(np.uint32)

    def expand(v):
        v = (v * np.uint32(0x00010001)) & np.uint32(0xFF0000FF)
        v = (v * np.uint32(0x00000101)) & np.uint32(0x0F00F00F)
        v = (v * np.uint32(0x00000011)) & np.uint32(0xC30C30C3)
        return (v * np.uint32(0x00000005)) & np.uint32(0x49249249)
    return (expand(q[:, 0]) << np.uint32(2)) | (expand(q[:, 1]) << np.uint32(1)) | expand(q[:, 2])


def check_property(name: str, tris: np.ndarray) -> None:
    """The property the degenerate case exists for still holds on these (world)
    triangles."""
    n = tris.shape[0]
    assert n == triangles(name).shape[0]
    keys = morton_keys(tris)
    if name.startswith("same"):
        assert np.all(tris == tris[0]) and len(np.unique(keys)) == 1 and not zero_area(tris).any()
    elif name.startswith("coplanar"):
        assert np.ptp(tris[..., 2]) == 0 and np.ptp(tris[..., 0]) > 0 and np.ptp(tris[..., 1]) > 0
        assert not zero_area(tris).all()
    elif name == "line40":
        assert np.ptp(tris[..., 1]) == 0 and np.ptp(tris[..., 2]) == 0 and np.ptp(tris[..., 0]) > 0
        assert zero_area(tris).all()
    elif name == "point20":
        assert np.all(tris == tris[0, 0]) and len(np.unique(keys)) == 1 and zero_area(tris).all()
    elif name == "zeroarea300":
        assert int(zero_area(tris).sum()) == 200
        assert int(np.all(tris[:, 0] == tris[:, 1], axis=1).sum()) == 200
        assert int((np.all(tris[:, 0] == tris[:, 1], axis=1) & np.all(tris[:, 0] == tris[:, 2], axis=1)).sum()) == 100
    elif name == "outlier1500":
        assert len(np.unique(keys[:-1])) == 1 and keys[-1] != keys[0]
    elif name in ("n1", "n2", "n3"):
        assert not zero_area(tris).any()


def _centre_extent(c: np.ndarray):
    v = c.reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    ext = float(np.linalg.norm(hi - lo))
    return (lo + hi) / 2, lo, hi, (ext if ext > 0 else 1.0)


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _pack(o, d, tmin=0.0, tmax=1e30):
    r = np.zeros((len(o), 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, tmin, d, tmax
    return r


def rays(name: str, tris: np.ndarray, n: int = 4096) -> np.ndarray:
    """n rays (o, tmin, d, tmax): half start 1-4 extents of the cluster from its
    centre, aimed at jittered vertices (a vertex pulled a random part of the
    way to its triangle's centroid, plus a little noise); half start inside
    the cluster's bounding box, padded by 2 % of the extent on every axis, in
    random directions. (The padding keeps the origins off a box without
    volume: a ray that starts exactly on the line of a collinear triangle sees
    three sheared vertices that are multiples of one vector, its edge functions
    are rounding noise, and a quarter of such rays "hit" with a meaningless t,
    in the oracle's walks and in its brute force alike. Origins exactly on
    geometry are edge_rays' business.)"""
    rng = np.random.default_rng(_seed(name) ^ 0x5EED)
    c = cluster(name, tris).astype(np.float64)
    centre, lo, hi, ext = _centre_extent(c)
    h = n // 2
    o1 = centre + _unit(rng, h) * rng.uniform(1.0, 4.0, (h, 1)) * ext
    ti, vi = rng.integers(0, len(c), h), rng.integers(0, 3, h)
    a = rng.uniform(-0.2, 0.7, (h, 1))
    tgt = c[ti, vi] * (1 - a) + c[ti].mean(axis=1) * a + rng.normal(0.0, 2e-3 * ext, (h, 3))
    d1 = tgt - o1
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    o2 = rng.uniform(lo - 0.02 * ext, hi + 0.02 * ext, (n - h, 3))
    return np.concatenate([_pack(o1, d1), _pack(o2, _unit(rng, n - h))])


def packet_rays(name: str, tris: np.ndarray, tiles: int = 8) -> np.ndarray:
    """Rays of one pinhole (shared origin, 2.5 extents from the cluster's
    centre) through a grid of sensor points in 8x8 tiles, one tile per 64-ray
    packet, the frustum about as wide as the cluster."""
    c = cluster(name, tris)
    centre, lo, hi, ext = _centre_extent(c)
    back = np.array([0.48, -0.62, 0.62])
    back /= np.linalg.norm(back)
    right = np.cross([0.0, 0.0, 1.0], back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    o = centre + back * 2.5 * ext
    half = 0.15
    W = 8 * tiles
    ty, tx, yy, xx = np.meshgrid(np.arange(tiles), np.arange(tiles), np.arange(8), np.arange(8), indexing="ij")
    px, py = (tx * 8 + xx).reshape(-1), (ty * 8 + yy).reshape(-1)
    sx = ((px + 0.5) / W * 2 - 1) * half
    sy = (1 - (py + 0.5) / W * 2) * half
    d = right[None] * sx[:, None] + up[None] * sy[:, None] - back[None]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return _pack(np.broadcast_to(o, d.shape), d)


def edge_rays(name: str, tris: np.ndarray, brute) -> np.ndarray:
    """Ray edge cases on the world triangles of a case; brute(tris, rays) ->
    (hits, prims) gives the exact hit distance the tmin == tmax rays use.
    NaN and zero-length directions are left out: the ABI does not define them."""
    rng = np.random.default_rng(_seed(name) ^ 0xED6E)
    t = tris.astype(np.float64)
    centre, lo, hi, ext = _centre_extent(t)
    good = np.nonzero(~zero_area(tris))[0]
    rows = []

    def aim(tgt, dist=2.0):
        o = tgt + _unit(rng, 1)[0] * dist * ext
        d = tgt - o
        return o, d / np.linalg.norm(d)

    for k in range(24):  # +0.0 / -0.0 direction components on each axis
        tri = t[good[rng.integers(0, len(good))]]
        o, d = aim(tri.mean(0))
        ax = k % 3
        d[ax] = 0.0 if (k // 3) % 2 == 0 else -0.0
        o[ax] = tri.mean(0)[ax]
        d /= np.linalg.norm(d)
        rows.append([*o, 0.0, *d, 1e30])
        if k >= 12:  # two zero components: an axis-parallel ray
            ax2 = (ax + 1) % 3
            d[ax2] = -0.0 if (k // 3) % 2 == 0 else 0.0
            o[ax2] = tri.mean(0)[ax2]
            rows.append([*o, 0.0, *d / np.linalg.norm(d), 1e30])
    for k in range(12):  # one subnormal component
        tri = t[good[rng.integers(0, len(good))]]
        o, d = aim(tri.mean(0))
        ax = k % 3
        d[ax] = 0.0
        d /= np.linalg.norm(d)
        d[ax] = (1e-40, -1e-40, 1.4e-45, -3e-39)[k // 3]
        o[ax] = tri.mean(0)[ax]
        rows.append([*o, 0.0, *d, 1e30])
    z = float(tris[0, 0, 2])
    for k in range(16):  # rays lying in the plane z = const of the first vertex (coplanar40: of every triangle)
        a = rng.uniform(0, 2 * np.pi)
        d = np.array([np.cos(a), np.sin(a), 0.0])
        o = np.array([*(centre[:2] + rng.uniform(-0.4, 0.4, 2) * ext), z]) - d * ext * (k % 2)
        rows.append([*o, 0.0, *d, 1e30])
    for k in range(24):  # origins exactly on a vertex, on an edge, in the interior, tmin = 0
        tri = tris[good[rng.integers(0, len(good))]]
        p = (tri[0], (tri[0] + tri[1]) * np.float32(0.5), ((tri[0] + tri[1]) + tri[2]) / np.float32(3.0))[k % 3]
        nrm = np.cross(tri[1].astype(np.float64) - tri[0], tri[2].astype(np.float64) - tri[0])
        d = (nrm / np.linalg.norm(nrm), _unit(rng, 1)[0], (tri[1] - tri[0]) / np.linalg.norm(tri[1] - tri[0]),
             -nrm / np.linalg.norm(nrm))[(k // 3) % 4]
        rows.append([*p, 0.0, *d, 1e30])
    blo, bhi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)  # the root box (float32, exact)
    for ax in range(3):  # rays along a face of the root box
        for face in (blo, bhi):
            for k in range(2):
                u = (ax + 1 + k) % 3
                o = np.array(centre)
                o[ax] = face[ax]
                o[u] = blo[u] - 0.5 * ext
                d = np.zeros(3)
                d[u] = 1.0
                rows.append([*o, 0.0, *d, 1e30])
                w = 3 - ax - u
                d2 = d.copy()
                d2[w] = 0.3  # in the face's plane, not along an axis
                rows.append([*o, 0.0, *(d2 / np.linalg.norm(d2)), 1e30])
    base = rays(name, tris, 64)
    inf = base.copy()  # tmax = inf
    inf[:, 7] = np.inf
    rows += inf.tolist()
    bh, bp = brute(tris, base)
    hit = base[bp >= 0].copy()
    assert len(hit) >= 4
    eq = hit.copy()  # tmin == tmax at an exact hit distance
    eq[:, 3] = eq[:, 7] = bh[bp >= 0, 0]
    rows += eq.tolist()
    rev = hit.copy()  # tmin > tmax
    rev[:, 3], rev[:, 7] = bh[bp >= 0, 0] * np.float32(2.0), bh[bp >= 0, 0] * np.float32(0.5)
    rows += rev.tolist()
    out = np.array(rows, np.float32)
    assert np.all(np.isfinite(out[:, 0:7])) and np.all(np.linalg.norm(out[:, 4:7].astype(np.float64), axis=1) > 0.5)
    return out
