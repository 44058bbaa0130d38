"""PNG compression on the device (rr_set_png_compression): the adaptive row
filter of png.hip / png16.hip through rr_debug_encode_device at both depths and
in every colour mode, against the numpy rule of tests/png_filters.py; legacy
bytes; one effort level; rendered frames by the three coders; frames in flight
keep their setting; the setter's values and the environment."""
import io
import json

import numpy as np
import pytest
from PIL import Image

import color_modes as M
import png_filters as F
import view_settings as V
from conftest import scene_path

pytestmark = pytest.mark.gpu

S04 = scene_path("04_very-simple-standin.rrscene")
MODES = {"BW": 1, "RGB": 3, "RGBA": 4}
ALL_TYPES = {0, 1, 2, 3, 4}
# 64 x 17: row 16 opens the second band, its Up / Average / Paeth read across
# the band boundary; 65 x 33: three bands; 1100 x 3 at four channels: rows of
# 4401 bytes, a 4096-position chunk boundary inside a row
SIZES = [(1, 1), (7, 5), (64, 17), (65, 33)]


def _sizes(c):
    return SIZES + ([(1100, 3)] if c == 4 else [])


@pytest.fixture()
def pctx(ctx):
    """The session's context, handed back with the legacy setting."""
    yield ctx
    ctx.set_png_compression("legacy")
    ctx.set_device_png(False)
    ctx.set_png_depth(0)
    ctx.set_ocio_config(None)


def _check_file(data, want, depth, c, what):
    """Strict reader, samples bit for bit, filter bytes by the rule over the raw
    scanlines; returns the rows' types."""
    px, info = F.read_png(data)
    assert (info["depth"], info["channels"]) == (depth, c), what
    assert px.shape == want.shape and np.array_equal(px, want), (what, int(np.count_nonzero(px != want)))
    raw = F.scanlines(want, depth)
    assert np.array_equal(info["raw"], raw), what
    types = F.rule(raw, info["bpp"])
    assert np.array_equal(info["filters"], types), (what, info["filters"].tolist(), types.tolist())
    return types


@pytest.mark.parametrize("mode", ["BW", "RGB", "RGBA"])
def test_png8_adaptive(pctx, mode):
    c = MODES[mode]
    pctx.set_png_compression(15)
    seen = set()
    for w, h in _sizes(c):
        for seed in range(2):
            img = F.image(w, h, c, seed)
            data = pctx.encode_device("PNG", img, 8, mode)
            want = M.expected_png8(img, c)
            seen |= set(_check_file(data, want, 8, c, (mode, w, h, seed)).tolist())
            im = Image.open(io.BytesIO(data))
            assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[c]
            assert np.array_equal(np.asarray(im).reshape(h, w, c), want)
    assert seen == ALL_TYPES, seen


@pytest.mark.parametrize("mode", ["BW", "RGB", "RGBA"])
def test_png16_adaptive(pctx, rr, tmp_path, mode):
    """Standard over every shape (samples by tests/png16_reader.py's restatement
    through color_modes), then Filmic and Filmic Log on synthetic LUTs (the plain
    and the extended raw-scanline kernel; samples by tests/view_settings.py's)."""
    c = MODES[mode]
    table = rr.native.srgb16_table()
    pctx.set_png_compression(15)
    seen = set()
    for w, h in _sizes(c):
        for seed in range(2):
            img = F.float_image(w, h, seed)
            data = pctx.encode_device("PNG", img, 16, mode, view_transform=0, exposure_scale=1.25)
            want = M.expected_png16(img, c, 0, 1.25, table)
            seen |= set(_check_file(data, want, 16, c, (mode, w, h, seed)).tolist())
            im = Image.open(io.BytesIO(data))
            if c == 1:  # PIL reads 16-bit grey at full precision
                assert np.array_equal(np.asarray(im).astype(np.uint16).reshape(h, w, 1), want)
            else:  # and the top bytes of the others
                assert np.array_equal(np.asarray(im.convert("RGBA" if c == 4 else "RGB")).reshape(h, w, c),
                                      (want >> 8).astype(np.uint8))
    V.write_luts(str(tmp_path), n3=17, n1=1024)
    luts = V.load_luts(str(tmp_path))
    pctx.set_ocio_config(str(tmp_path))
    for view in (V.FILMIC, V.FILMIC_LOG):
        img = F.float_image(65, 33, seed=c)
        data = pctx.encode_device("PNG", img, 16, mode, view_transform=view, exposure_scale=0.8)
        want = V.view16(img, c, view, luts, "None", 1.0, 0.8, table).reshape(33, 65, c)
        seen |= set(_check_file(data, want, 16, c, (mode, view)).tolist())
    assert seen == ALL_TYPES, seen


def test_legacy_bytes(pctx, rr):
    """A context that never called the setter writes what one writes that called
    it with 15 and then with legacy, and the old entry points follow the setting."""
    img8 = F.image(65, 33, 4, 1)
    imgf = F.float_image(65, 33, 1)
    with rr.RenderContext(0) as fresh:
        never = [fresh.encode_device("PNG", img8, 8, m) for m in MODES] + \
                [fresh.encode_device("PNG", imgf, 16, m, exposure_scale=1.25) for m in MODES] + \
                [fresh.png_device(img8), fresh.png16_device(imgf, 0, 1.25)]
    pctx.set_png_compression(15)
    on = [pctx.encode_device("PNG", img8, 8, "RGBA"), pctx.encode_device("PNG", imgf, 16, "RGBA", exposure_scale=1.25),
          pctx.png_device(img8), pctx.png16_device(imgf, 0, 1.25)]
    assert on[0] == on[2] and on[1] == on[3]  # the old entries take the setting too
    assert on[0] != never[2] and on[1] != never[5]
    pctx.set_png_compression("legacy")
    back = [pctx.encode_device("PNG", img8, 8, m) for m in MODES] + \
           [pctx.encode_device("PNG", imgf, 16, m, exposure_scale=1.25) for m in MODES] + \
           [pctx.png_device(img8), pctx.png16_device(imgf, 0, 1.25)]
    assert back == never
    for data in never:
        assert set(F.read_png(data)[1]["filters"].tolist()) == {1}
    pctx.set_png_compression("scene")  # no scene behind an image of the caller's: legacy
    assert pctx.encode_device("PNG", img8, 8, "RGBA") == never[2]
    # JPEG and OPEN_EXR do not see the setting
    jpeg, exr = pctx.encode_device("JPEG", img8, 8, "RGB"), pctx.encode_device("OPEN_EXR", imgf, 16, "RGBA")
    pctx.set_png_compression(100)
    assert pctx.encode_device("JPEG", img8, 8, "RGB") == jpeg
    assert pctx.encode_device("OPEN_EXR", imgf, 16, "RGBA") == exr


def test_one_effort_level(pctx):
    """The device coders have one effort level: 0, 15 and 100 give one file."""
    img8 = F.image(64, 17, 4, 0)
    imgf = F.float_image(64, 17, 0)
    files = []
    for comp in (0, 15, 100):
        pctx.set_png_compression(comp)
        files.append((pctx.encode_device("PNG", img8, 8, "RGB"), pctx.encode_device("PNG", imgf, 16, "BW")))
    assert files[0] == files[1] == files[2]
    assert not F.stored_only(F.read_png(files[0][0])[1]["zlib"])  # smaller than Blender's file at 0


def _render(c, s, p, tmp, name, device_png, depth):
    c.set_device_png(device_png)
    c.set_png_depth(depth)
    c.render_frame(s, 3, p, str(tmp / name), "PNG", 90)
    return (tmp / (name + ".png")).read_bytes()


def test_rendered_frames(pctx, rr, tmp_path):
    s = pctx.load_scene(S04)
    p = rr.default_params(spp=4, width=96, height=64)
    try:
        film, rgba8, _ = pctx.render_to_memory(s, 3, p)
        scale = float(pctx.frame_state(s, 3, p).render_floats[2])
        legacy = {k: _render(pctx, s, p, tmp_path, "l" + k, dp, d)
                  for k, dp, d in (("host", False, 8), ("dev", True, 8), ("p16", False, 16))}
        pctx.set_png_compression(15)
        want8 = rgba8.copy()
        want8[..., 3] = 255
        for k, dp in (("host", False), ("dev", True)):
            data = _render(pctx, s, p, tmp_path, "a" + k, dp, 8)
            types = _check_file(data, want8, 8, 4, k)
            assert set(types.tolist()) != {1} and data != legacy[k]
            print(f"{k}: legacy {len(legacy[k])} bytes, adaptive {len(data)}; types {np.bincount(types, minlength=5).tolist()}")
        data = _render(pctx, s, p, tmp_path, "ap16", False, 16)
        want16 = M.expected_png16(film, 4, 0, scale, rr.native.srgb16_table())
        types = _check_file(data, want16, 16, 4, "p16")
        assert set(types.tolist()) != {1} and data != legacy["p16"]
        # the legacy files are what they were: Sub on every row
        for k, d in legacy.items():
            assert set(F.read_png(d)[1]["filters"].tolist()) == {1}, k
        # the scene's own field, where the context asks for it
        doc = json.load(open(S04))
        doc["render"]["png_compression"] = 40
        (tmp_path / "c.rrscene").write_text(json.dumps(doc))
        s2 = pctx.load_scene(str(tmp_path / "c.rrscene"))
        try:
            pctx.set_png_compression("scene")
            assert _render(pctx, s2, p, tmp_path, "s2", True, 8) == (tmp_path / "adev.png").read_bytes()
            assert _render(pctx, s, p, tmp_path, "s1", True, 8) == legacy["dev"]  # no field: legacy
            pctx.set_png_compression("legacy")
            assert _render(pctx, s2, p, tmp_path, "s3", True, 8) == legacy["dev"]  # the context's goes first
        finally:
            s2.close()
    finally:
        s.close()


@pytest.mark.parametrize("coder", ["host", "dev", "p16"])
def test_frames_in_flight_keep_their_setting(pctx, rr, tmp_path, coder):
    s = pctx.load_scene(S04)
    p = rr.default_params(spp=4, width=96, height=64)
    try:
        pctx.set_device_png(coder == "dev")
        pctx.set_png_depth(16 if coder == "p16" else 8)
        pctx.set_png_compression(15)
        t1 = pctx.submit_frame(s, 3, p, str(tmp_path / "f1"), "PNG", 90)
        pctx.set_png_compression("legacy")
        t2 = pctx.submit_frame(s, 3, p, str(tmp_path / "f2"), "PNG", 90)
        pctx.complete_frame(t1)
        pctx.complete_frame(t2)
        a, b = F.read_png((tmp_path / "f1.png").read_bytes()), F.read_png((tmp_path / "f2.png").read_bytes())
        assert np.array_equal(a[0], b[0])
        assert np.array_equal(a[1]["filters"], F.rule(a[1]["raw"], a[1]["bpp"])) and set(a[1]["filters"].tolist()) != {1}
        assert set(b[1]["filters"].tolist()) == {1}
    finally:
        s.close()


def test_setter_values_and_environment(rr, monkeypatch):
    n = rr.native
    img = F.image(64, 17, 4, 0)
    monkeypatch.delenv("RR_PNG_COMPRESSION", raising=False)
    with rr.RenderContext(0) as c:
        legacy = c.encode_device("PNG", img, 8, "RGBA")
        c.set_png_compression(15)
        adaptive = c.encode_device("PNG", img, 8, "RGBA")
        assert adaptive != legacy
        for bad in (101, -3, 1000, -100):
            with pytest.raises(rr.RRError) as e:
                c.set_png_compression(bad)
            assert e.value.code == n.RR_EINVAL
        assert c.encode_device("PNG", img, 8, "RGBA") == adaptive  # a refused value changes nothing
    for text, want in (("15", adaptive), ("0", adaptive), ("100", adaptive), ("scene", legacy), ("", legacy)):
        monkeypatch.setenv("RR_PNG_COMPRESSION", text)
        with rr.RenderContext(0) as c:
            assert c.encode_device("PNG", img, 8, "RGBA") == want, text
    for text in ("101", "-3", "-1", "fast", "15%", "1.5"):
        monkeypatch.setenv("RR_PNG_COMPRESSION", text)
        with pytest.raises(rr.RRError) as e:
            rr.RenderContext(0)
        assert e.value.code == n.RR_EINVAL, text
    monkeypatch.delenv("RR_PNG_COMPRESSION")
    with rr.RenderContext(0, png_compression=15) as c:
        assert c.encode_device("PNG", img, 8, "RGBA") == adaptive
