"""PNG compression (rr_set_png_compression), the parts that need no GPU: the
adaptive filter rule in C against numpy and against libpng's own files; the
host coder's files at 0, 15 and 100; legacy bytes; the setter's, the host
functions' and the scene field's errors; header, binding and exporter."""
import argparse
import ctypes
import io
import json
import os
import re
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

import png_filters as F
from conftest import ROOT, scene_path

S01 = scene_path("01_simple-animation.rrscene")
S04 = scene_path("04_very-simple-standin.rrscene")
BLEND01 = os.path.join(ROOT, "blender-projects", "01_simple-animation", "01_simple-animation.blend")
SIZES = [(1, 1), (7, 5), (64, 17), (65, 33), (200, 40)]
MODES = {"BW": 1, "RGB": 3, "RGBA": 4}
ALL_TYPES = {0, 1, 2, 3, 4}


def _samples(img, c):
    """The (H, W, c) samples an 8-bit file of c channels holds of generator image img
    (grey: the red channel stands in, the rule sees bytes only)."""
    return np.ascontiguousarray(img[..., :c])


# ---------------------------------------------------------------- the rule --
@pytest.mark.parametrize("bpp", [1, 2, 3, 4, 6, 8])
def test_c_rule_equals_numpy(rr, bpp):
    seen = set()
    for w, h in SIZES:
        for seed in range(3):
            # bpp bytes a pixel: the generator's bytes taken as they come
            img = np.concatenate([F.image(w, h, 4, seed), F.image(w, h, 4, seed + 7)], axis=-1)[..., :bpp]
            raw = img.reshape(h, w * bpp)
            want = F.rule(raw, bpp)
            got = rr.png_filters(raw, bpp)
            assert np.array_equal(got, want), (bpp, w, h, seed, got, want)
            seen |= set(want.tolist())
    assert seen == ALL_TYPES, seen


def test_rule_on_thin_images(rr):
    """One row, or one pixel's width: no Average, as in libpng (checked against
    it below); the C statement and numpy agree on them too."""
    for w, h in [(1, 9), (9, 1), (1, 33), (64, 1)]:
        for c in (1, 3, 4):
            for seed in range(3):
                raw = F.scanlines(_samples(F.image(w, h, c, seed), c), 8)
                want = F.rule(raw, c)
                assert np.array_equal(rr.png_filters(raw, c), want)
                assert 3 not in want


@pytest.mark.parametrize("c", [1, 3, 4])
def test_rule_equals_libpng(rr, c):
    """libpng's own file (simplified write API, default filters), in a plain
    process: its rows' filter bytes are the rule's, in C and in numpy."""
    if F.libpng() is None:
        pytest.skip("libpng16 does not load through ctypes (ctypes.util.find_library('png16'))")
    counts = np.zeros(5, np.int64)
    for w, h in SIZES + [(1, 9), (9, 1)]:
        for seed in range(4):
            s = _samples(F.image(w, h, c, seed), c)
            px, info = F.read_png(F.libpng_file(s), one_idat=False)
            assert info["depth"] == 8 and info["channels"] == c and np.array_equal(px, s)
            raw = F.scanlines(s, 8)
            want = F.rule(raw, c)
            assert np.array_equal(info["filters"], want), (w, h, seed, info["filters"], want)
            assert np.array_equal(rr.png_filters(raw, c), info["filters"])
            counts += np.bincount(want, minlength=5)
    print("filter types (None, Sub, Up, Average, Paeth):", counts.tolist())
    assert np.all(counts > 0), counts


def test_filter_functions_errors(rr):
    L, n = rr.lib(), rr.native
    raw = np.zeros((2, 8), np.uint8)
    out = np.zeros(2, np.uint8)
    p, o = raw.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert L.rr_debug_png_filters(p, 8, 2, 4, o) == n.RR_OK
    for args in ((None, 8, 2, 4, o), (p, 8, 2, 4, None), (p, 0, 2, 4, o), (p, 8, 0, 4, o), (p, 8, 2, 0, o),
                 (p, 8, 2, 9, o)):
        assert L.rr_debug_png_filters(*args) == n.RR_EINVAL, args[1:4]


# -------------------------------------------------------------- host files --
@pytest.mark.parametrize("mode", ["BW", "RGB", "RGBA"])
def test_host_files(rr, tmp_path, mode):
    import color_modes as M
    c = MODES[mode]
    seen = set()
    for w, h in SIZES + [(333, 70)]:  # 70 rows: several thread bands, rows filtered across them
        img = F.image(w, h, c, seed=w)
        want = M.expected_png8(img, c)
        raw = F.scanlines(want, 8)
        types = F.rule(raw, c)
        seen |= set(types.tolist())
        filtered = F.filter_rows(raw, c, types).tobytes()
        size = {}
        for comp in (0, 15, 100):
            n = rr.encode_image_png(img, str(tmp_path / "a"), mode, comp)
            data = (tmp_path / "a.png").read_bytes()
            assert n == len(data)
            px, info = F.read_png(data)
            assert info["depth"] == 8 and info["channels"] == c
            assert np.array_equal(px, want), (w, h, comp)
            assert np.array_equal(info["filters"], types), (w, h, comp)
            assert info["filtered"] == filtered
            assert F.stored_only(info["zlib"]) == (comp == 0), (w, h, comp)
            im = Image.open(io.BytesIO(data))
            assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[c]
            assert np.array_equal(np.asarray(im).reshape(h, w, c), want)
            size[comp] = len(data)
        # where zlib itself, over the same filtered bytes, gains from level 9: so does the file
        if len(zlib.compress(filtered, 9)) <= len(zlib.compress(filtered, 1)):
            assert size[100] <= size[15], (w, h, size)
        # legacy: rr_encode_image_mode's bytes
        rr.encode_image_png(img, str(tmp_path / "l"), mode, "legacy")
        rr.encode_image_mode(img, str(tmp_path / "m"), "PNG", 90, mode)
        assert (tmp_path / "l.png").read_bytes() == (tmp_path / "m.png").read_bytes()
        assert set(F.read_png((tmp_path / "l.png").read_bytes())[1]["filters"].tolist()) == {1}
    assert seen == ALL_TYPES, seen


def test_zlib_level_of_the_setting(rr, tmp_path):
    """Blender's level = (int)(compression / 11.1111f), 0 .. 9: a file written at
    a setting is the file of every other setting with that level."""
    img = F.image(200, 40, 4, seed=2)
    sizes = {}
    for comp in (0, 11, 12, 15, 22, 23, 50, 99, 100):
        rr.encode_image_png(img, str(tmp_path / "z"), "RGBA", comp)
        sizes[comp] = (tmp_path / "z.png").read_bytes()
    assert sizes[0] == sizes[11] and sizes[12] == sizes[15] == sizes[22]  # levels 0, 0, 1, 1, 1
    assert sizes[0] != sizes[12] and sizes[22] != sizes[23]  # levels 0 | 1, 1 | 2
    assert len(sizes[100]) < len(sizes[12]) < len(sizes[0])


def test_host_encoder_errors(rr, tmp_path):
    L, n = rr.lib(), rr.native
    img = F.image(4, 4, 4)
    p = img.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    path = str(tmp_path / "e").encode()
    nb = ctypes.c_uint64()
    assert L.rr_encode_image_png(p, 4, 4, path, 4, 15, ctypes.byref(nb)) == n.RR_OK
    for comp in (101, -3, n.RR_PNG_COMPRESSION_SCENE, 1000):
        assert L.rr_encode_image_png(p, 4, 4, path, 4, comp, ctypes.byref(nb)) == n.RR_EINVAL, comp
    assert L.rr_encode_image_png(None, 4, 4, path, 4, 15, ctypes.byref(nb)) == n.RR_EINVAL
    assert L.rr_encode_image_png(p, 4, 4, path, 2, 15, ctypes.byref(nb)) == n.RR_EINVAL


# --------------------------------------------------------------- interface --
def test_setter_null_ctx(rr):
    L, n = rr.lib(), rr.native
    for v in (15, 0, 100, 101, -3, n.RR_PNG_COMPRESSION_LEGACY, n.RR_PNG_COMPRESSION_SCENE):
        assert L.rr_set_png_compression(None, v) == n.RR_EINVAL


def test_values_header_and_binding(rr):
    n = rr.native
    assert (n.RR_PNG_COMPRESSION_LEGACY, n.RR_PNG_COMPRESSION_SCENE) == (-1, -2)
    src = open(os.path.join(ROOT, "include", "rr.h")).read()
    assert re.search(r"#define RR_PNG_COMPRESSION_LEGACY \(-1\)", src)
    assert re.search(r"#define RR_PNG_COMPRESSION_SCENE \(-2\)", src)
    assert re.search(r"#define RR_ABI_VERSION 8\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for sym in ("rr_set_png_compression", "rr_encode_image_png", "rr_debug_png_filters",
                "rr_debug_scene_png_compression"):
        assert re.search(rf"\b{sym}\s*\(", code), sym
        assert sym in n.EXPORTS and hasattr(rr.lib(), sym)
        assert getattr(rr.lib(), sym).argtypes is not None, sym
    assert rr.lib().rr_abi_version() == 8 == n.RR_ABI_VERSION
    assert [n.png_compression_value(v) for v in (None, "legacy", "scene", 0, 15, 100, -1)] == [-1, -1, -2, 0, 15, 100, -1]
    with pytest.raises(ValueError):
        n.png_compression_value("small")
    # every declaration cites the reference lines it replaces, as its neighbours do
    for sym in ("rr_set_png_compression", "rr_encode_image_png", "rr_debug_png_filters"):
        head = src[:src.index(sym + "(")]
        assert "render-timing-script.py:83-92" in head[head.rindex("/*"):], sym


def _scene_with(tmp_path, name, **render):
    doc = json.load(open(S04))
    for k, v in render.items():
        doc["render"][k] = v
    p = tmp_path / (name + ".rrscene")
    p.write_text(json.dumps(doc))
    return str(p)


@pytest.mark.parametrize("value", [0, 15, 100])
def test_scene_field_is_parsed(rr, tmp_path, value):
    s = rr.Scene(_scene_with(tmp_path, "ok", png_compression=value))
    try:
        assert s.png_compression() == value
    finally:
        s.close()


def test_scene_without_the_field_means_legacy(rr):
    for path in (S01, S04):
        assert "png_compression" not in json.load(open(path))["render"]
        s = rr.Scene(path)
        try:
            assert s.png_compression() == rr.native.RR_PNG_COMPRESSION_LEGACY
        finally:
            s.close()


@pytest.mark.parametrize("value", [101, -1, -3, 15.5, "15", None, 1e9])
def test_scene_field_is_refused(rr, tmp_path, value):
    with pytest.raises(rr.RRError) as e:
        rr.Scene(_scene_with(tmp_path, "bad", png_compression=value))
    assert e.value.code == rr.native.RR_EINVAL and "png_compression" in str(e.value)


class _Ctx:
    def __init__(self):
        self.calls = []

    def set_png_compression(self, v):
        self.calls.append(v)


def test_runner_passes_the_setting_through(rr):
    c = _Ctx()
    rr.BackendRunner(ROOT, ctx=c, png_compression=15)
    assert c.calls == [15]
    c = _Ctx()
    rr.BackendRunner(ROOT, ctx=c, png_compression=0)  # 0 is a setting, not "none"
    assert c.calls == [0]
    c = _Ctx()
    rr.BackendRunner(ROOT, ctx=c)
    assert c.calls == []


def _export(blend, **kw):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from blend_export import export
    args = argparse.Namespace(samples=128, max_bounces=12, clamp_indirect=10.0, seed=0, **kw)
    return json.loads(json.dumps(export(blend, args)))


def test_exporter_keep_and_project(rr, tmp_path):
    committed = json.load(open(S01))
    assert _export(BLEND01) == committed  # no attribute: keep
    assert _export(BLEND01, png_compression="keep") == committed
    proj = _export(BLEND01, png_compression="project")
    v = proj["render"]["png_compression"]
    assert isinstance(v, int) and v == 100  # ImageFormatData.compress of the 01 project (PNG, quality 90)
    p = tmp_path / "p.rrscene"
    p.write_text(json.dumps(proj))
    s = rr.Scene(str(p))
    try:
        assert s.png_compression() == 100
    finally:
        s.close()
    del proj["render"]["png_compression"]
    assert proj == committed
