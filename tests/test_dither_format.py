"""The 8-bit dither (rr_set_dither) on the host, no GPU: the fixed sine and the
noise against the numpy float32 restatement of tests/dither.py bit for bit and
against libm in double, the noise's range, orientation and mean, the setter's
NULL check, the scene field, the binding's export list and the ABI number."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest

import dither as D
from conftest import ROOT, scene_path

F32 = np.float32
SIZES = [(1, 1), (37, 19), (256, 256), (1920, 1080)]
# |sin_fixed(a) - sin(a)| <= 2^-18: half an ulp of the hash's arguments above 64
# (they reach 139.2) moves the sine by as much, so nothing finer shows
SIN_BOUND = 2.0 ** -18
ENDPOINTS = np.array([0.0, 139.2227], F32)


def _hash_arguments():
    parts = [ENDPOINTS]
    for w, h in ((1920, 1080), (37, 19), (1, 1)):
        a0, a1 = D.hash_args(w, h)
        parts += [a0.ravel(), a1.ravel()]
    return np.concatenate(parts)


@pytest.fixture(scope="module")
def sine_inputs():
    rnd = (np.random.default_rng(20) .random(1 << 20) * 140.0).astype(F32)
    rnd = rnd[rnd < F32(140.0)]
    return {"hash": _hash_arguments(), "random": rnd, "ends": ENDPOINTS}


@pytest.mark.parametrize("which", ["hash", "random", "ends"])
def test_sin_fixed_matches_restatement_and_libm(rr, sine_inputs, which):
    a = sine_inputs[which]
    got = rr.sin_fixed(a)
    want = D.sin_fixed(a)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{len(bad)} of {len(a)} differ, first a = {a[bad[0]]!r}: {got[bad[0]]!r} != {want[bad[0]]!r}"
    ref = np.sin(a.astype(np.float64))
    assert ref[0] == math.sin(float(a[0]))  # numpy's double sine is libm's
    err = np.abs(got.astype(np.float64) - ref)
    print(f"sin_fixed {which}: max error {err.max():.3e} (bound {SIN_BOUND:.3e})")
    assert err.max() <= SIN_BOUND, f"a = {a[np.argmax(err)]!r}: error {err.max():.3e}"


def test_sin_fixed_outside_its_domain(rr):
    a = np.array([8192.0, -8192.0, 8193.0, -1e30, np.inf, -np.inf, np.nan, -0.5, -139.2227], F32)
    got = rr.sin_fixed(a)
    assert np.array_equal(got.view(np.uint32), D.sin_fixed(a).view(np.uint32))
    assert np.all(got[2:7] == 0.0)
    assert np.abs(got[7:].astype(np.float64) - np.sin(a[7:].astype(np.float64))).max() <= SIN_BOUND


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_noise_matches_restatement(rr, size):
    w, h = size
    got = rr.dither_noise(w, h)
    want = D.noise(w, h)
    assert got.shape == (h, w)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{len(bad)} pixels differ, first {bad[0]}: {got[tuple(bad[0])]!r} != {want[tuple(bad[0])]!r}"
    assert got.min() >= -0.5 and got.max() < 1.5, (got.min(), got.max())


def test_noise_rows_run_top_to_bottom(rr):
    """Row 0 of the output is the image's top row, which Blender counts as
    y = H - 1: its first pixel hashes t = (H - 1) / H, the last row's t = 0."""
    w, h = 37, 19
    n = rr.dither_noise(w, h)

    def first_pixel(yb):
        t = F32(yb) * (F32(1.0) / F32(h))
        h0 = D.sin_fixed(np.array([F32(0.0) * D.AX + t * D.AY], F32)) * D.AM
        h1 = D.sin_fixed(np.array([F32(0.0) * D.BX + t * D.BY], F32)) * D.BM
        return ((h0 - np.floor(h0)) + (h1 - np.floor(h1)) - F32(0.5))[0]

    assert n[0, 0] == first_pixel(h - 1)
    assert n[h - 1, 0] == first_pixel(0) == F32(-0.5)  # s = t = 0: both sines are 0
    assert n[0, 0] != n[h - 1, 0]


def test_noise_mean():
    """Float64 evaluation of the rule with libm's sine first: the bound has to
    hold for the rule itself before it is asked of the code."""
    w = h = 256
    tol = 5.0 * math.sqrt(1.0 / 6.0) / 256.0  # 5 standard errors of a triangle distribution over 256 x 256 values
    x = np.arange(w)[None, :] / w
    yb = (h - 1 - np.arange(h))[:, None] / h
    h0 = np.sin(x * 12.9898 + yb * 78.233) * 43758.5453
    h1 = np.sin(x * 19.9898 + yb * 119.233) * 798.5453
    n64 = (h0 - np.floor(h0)) + (h1 - np.floor(h1)) - 0.5
    print(f"float64 mean {n64.mean():.6f}, tolerance {tol:.6f}")
    assert abs(n64.mean() - 0.5) <= tol


def test_noise_mean_of_the_library(rr):
    tol = 5.0 * math.sqrt(1.0 / 6.0) / 256.0
    m = float(rr.dither_noise(256, 256).astype(np.float64).mean())
    print(f"library mean {m:.6f}, tolerance {tol:.6f}")
    assert abs(m - 0.5) <= tol


# ------------------------------------------------- setter, scene, binding ----
def test_set_dither_null_ctx(rr):
    L = rr.lib()
    for v in (0.0, 1.0, rr.native.RR_DITHER_SCENE):
        assert L.rr_set_dither(None, ctypes.c_float(v)) == rr.native.RR_EINVAL
    assert L.rr_debug_dither_noise(0, 4, None) == rr.native.RR_EINVAL
    out = (ctypes.c_float * 4)()
    assert L.rr_debug_dither_noise(0, 4, out) == rr.native.RR_EINVAL
    assert L.rr_debug_dither_noise(2, -1, out) == rr.native.RR_EINVAL
    assert L.rr_debug_sin_fixed(None, 3, out) == rr.native.RR_EINVAL
    assert L.rr_debug_sin_fixed(None, 0, None) == 0


def _scene_with(tmp_path, name, **render):
    doc = json.load(open(scene_path("04_very-simple-standin.rrscene")))
    doc["render"].pop("dither_intensity", None)
    for k, v in render.items():
        doc["render"][k] = v
    p = str(tmp_path / (name + ".rrscene"))
    with open(p, "w") as fh:
        json.dump(doc, fh)
    return p


@pytest.mark.parametrize("value", [0, 1, 2, 0.5])
def test_scene_field_loads(rr, tmp_path, value):
    rr.Scene(_scene_with(tmp_path, "ok", dither_intensity=value)).close()


def test_scene_without_the_field_loads(rr, tmp_path):
    rr.Scene(_scene_with(tmp_path, "none")).close()


@pytest.mark.parametrize("value", [-0.1, 2.5, "1", None], ids=["neg", "above", "string", "null"])
def test_scene_field_refused(rr, tmp_path, value):
    with pytest.raises(rr.RRError) as e:
        rr.Scene(_scene_with(tmp_path, "bad", dither_intensity=value))
    assert e.value.code == rr.native.RR_EINVAL
    assert "render.dither_intensity" in str(e.value)


def test_committed_scenes_ask_for_blenders_default():
    for name in ("01_simple-animation.rrscene", "04_very-simple-standin.rrscene"):
        assert json.load(open(scene_path(name)))["render"]["dither_intensity"] == 1.0


def test_exports_match_header_and_abi_stays(rr):
    src = open(os.path.join(ROOT, "include", "rr.h")).read()
    assert re.search(r"#define RR_DITHER_SCENE \(-1\.0f\)", src)
    assert re.search(r"#define RR_ABI_VERSION 8\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(rr_[a-z_0-9]+)\s*\(", code)))
    assert sorted(rr.EXPORTS) == names
    for n in ("rr_set_dither", "rr_debug_dither_noise", "rr_debug_sin_fixed"):
        assert n in names and hasattr(rr.lib(), n)
    assert rr.lib().rr_abi_version() == 8 == rr.native.RR_ABI_VERSION
    assert rr.native.RR_DITHER_SCENE == -1.0
