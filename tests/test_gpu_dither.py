"""The 8-bit dither on the device (csrc/view.hip k_view<.., DITHER>, csrc/dither.h)
against the numpy float32 restatement of tests/dither.py, bit for bit: the view
pass on crafted images, rendered frames of both render paths, the files of
every 8-bit format, the formats that stay undithered, the scene's value and the
setting of frames in flight."""
import io
import json
import os

import numpy as np
import pytest
from PIL import Image

import color_modes as CM
import dither as D
import view_settings as V
from conftest import scene_path
from oracle import oracle as O

pytestmark = pytest.mark.gpu

F32 = np.float32
S01 = scene_path("01_simple-animation.rrscene")
S04 = scene_path("04_very-simple-standin.rrscene")
WAVEFRONT = 4  # RR_FLAG_WAVEFRONT
FRAME, W, H, SPP = 5, 64, 36, 4


@pytest.fixture(scope="module")
def luts(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("luts_dither"))
    V.write_luts(d, n3=17, n1=1024, false_color_n3=17)
    return d, V.load_luts(d)


@pytest.fixture(scope="module")
def table():
    return O.srgb_lut()


@pytest.fixture()
def dctx(ctx):
    """The session's context, handed back with every setting these tests touch at its default."""
    yield ctx
    ctx.set_dither(0.0)
    ctx.set_ocio_config(None)
    ctx.set_display_gamma(0.0)
    ctx.set_device_png(False)
    ctx.set_png_depth(0)
    ctx.set_exr_depth(0)
    ctx.set_color_mode(0)


# ------------------------------------------------------------- view pass -----
def _crafted_pixels():
    """4099 pixels (a prime: no row of any test size repeats the one above):
    the values (k +- 0.42) / 255 around every code boundary, then ramps over
    [0, 1] and over [0, 4], another phase a channel."""
    k = np.arange(256, dtype=np.float64)
    edge = np.concatenate([(k - 0.42) / 255.0, (k + 0.42) / 255.0]).astype(F32)
    ramp = np.linspace(0.0, 1.0, 2500).astype(F32)
    wide = np.linspace(0.0, 4.0, 4099 - 512 - 2500).astype(F32)
    v = np.concatenate([edge, ramp, wide])
    return np.stack([v, np.roll(v, 1371), np.roll(v, 2742)], axis=-1)


def _image(w, h):
    """(H, W, 4) float32 of the crafted pixels, repeated, and the index of each
    pixel's source (the display-referred values are a function of the pixel)."""
    px = _crafted_pixels()
    idx = np.arange(w * h) % len(px)
    img = np.zeros((h, w, 4), F32)
    img[..., :3] = px[idx].reshape(h, w, 3)
    img[..., 3] = 0.25
    return img, idx


VIEW_SIZES = [(37, 19), (1, 1), (1100, 1000)]
VIEW_CASES = [(v, g) for v in (V.STANDARD, V.RAW, V.FILMIC, V.FALSE_COLOR) for g in (1.0, 2.2)]


def _display_of(img, idx, view, gamma, lut, table):
    """V.display of the crafted pixels once, spread over the image."""
    px = _crafted_pixels()[None, :, :]
    d = V.display(px, view, 8, lut, "None", gamma, 1.0, table)[0]
    return d[idx].reshape(img.shape[0], img.shape[1], 3)


def _report(got, want, what):
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


@pytest.mark.parametrize("case", VIEW_CASES, ids=lambda c: f"{['std', 'raw', 'filmic', 'log', 'false'][c[0]]}-g{c[1]}")
def test_view_device_bit_exact(dctx, luts, table, case):
    """37 x 19: one partial block; 1 x 1; 1100 x 1000: more than 4096 blocks of
    256 pixels, so the last pixels come from the grid-stride loop's second trip
    and recover their column and row after it."""
    view, gamma = case
    d, lut = luts
    dctx.set_ocio_config(d)
    dctx.set_display_gamma(0.0 if gamma == 1.0 else gamma)
    assert 1100 * 1000 > 4096 * 256
    for w, h in VIEW_SIZES:
        img, idx = _image(w, h)
        disp = _display_of(img, idx, view, gamma, lut, table)
        dctx.set_dither(0.0)
        plain = dctx.view_device(img, view, 1.0)
        _report(plain, D.dither_codes(disp, 0.0), f"{w}x{h} intensity 0")
        dctx.set_dither(1.0)
        got = dctx.view_device(img, view, 1.0)
        _report(got, D.dither_codes(disp, 1.0), f"{w}x{h} intensity 1")
        assert np.all(got[..., 3] == 255)
        if w * h > 1:
            assert not np.array_equal(got, plain)


def test_view_device_other_intensities(dctx, table):
    img, idx = _image(37, 19)
    disp = _display_of(img, idx, V.STANDARD, 1.0, None, table)
    seen = []
    for g in (2.0, 0.5):
        dctx.set_dither(g)
        got = dctx.view_device(img, V.STANDARD, 1.0)
        _report(got, D.dither_codes(disp, g), f"intensity {g}")
        seen.append(got)
    assert not np.array_equal(seen[0], seen[1])
    dctx.set_dither("scene")  # an inspection call has no scene: no dither
    _report(dctx.view_device(img, V.STANDARD, 1.0), D.dither_codes(disp, 0.0), "scene")


def test_setter_range(dctx, rr):
    for bad in (-0.5, 2.0001, float("nan"), float("inf"), -2.0):
        with pytest.raises(rr.RRError) as e:
            dctx.set_dither(bad)
        assert e.value.code == rr.native.RR_EINVAL
    for ok in (0.0, 2.0, 1.0, rr.native.RR_DITHER_SCENE, "scene"):
        dctx.set_dither(ok)


# -------------------------------------------------------- rendered frames ----
def _params(rr, flags=0):
    return rr.default_params(width=W, height=H, spp=SPP, flags=flags)


def _want(ctx, scene, params, film, view, lut, table, g):
    scale = float(ctx.frame_state(scene, FRAME, params).render_floats[2])
    return D.dither_codes(V.display(film, view, 8, lut, "None", 1.0, scale, table), g)


@pytest.mark.parametrize("which", ["04vs-tiles", "04vs-wavefront", "01-filmic"])
def test_rendered_frame_is_dithered(dctx, rr, luts, table, which):
    """rr_render_frame_to_memory gives film and rgba8 of one frame: rgba8 is the
    restatement applied to that film, and not the undithered image."""
    d, lut = luts
    flags = WAVEFRONT if which == "04vs-wavefront" else 0
    path, view = (S01, V.FILMIC) if which == "01-filmic" else (S04, V.STANDARD)
    if view == V.FILMIC:
        dctx.set_ocio_config(d)
    s = dctx.load_scene(path)
    try:
        p = _params(rr, flags)
        film0, rgba0, st0 = dctx.render_to_memory(s, FRAME, p)
        assert (st0.view_transform, st0.view_transform_substituted) == (view, 0)
        _report(rgba0, _want(dctx, s, p, film0, view, lut, table, 0.0), "intensity 0")
        dctx.set_dither(1.0)
        film1, rgba1, st1 = dctx.render_to_memory(s, FRAME, p)
        assert (st1.view_transform, st1.view_transform_substituted) == (view, 0)
        assert np.array_equal(film1, film0)
        _report(rgba1, _want(dctx, s, p, film1, view, lut, table, 1.0), "intensity 1")
        assert not np.array_equal(rgba1, rgba0)
    finally:
        s.close()


@pytest.fixture(scope="module")
def frame04(ctx, rr, table):
    """The 04vs frame the file tests write: its undithered and dithered rgba8
    (intensity 1), checked by test_rendered_frame_is_dithered."""
    s = ctx.load_scene(S04)
    try:
        p = _params(rr)
        ctx.set_dither(0.0)
        film, plain, _ = ctx.render_to_memory(s, FRAME, p)
        scale = float(ctx.frame_state(s, FRAME, p).render_floats[2])
    finally:
        s.close()
    disp = V.display(film, V.STANDARD, 8, None, "None", 1.0, scale, table)
    return {"plain": plain, 1.0: D.dither_codes(disp, 1.0), 0.5: D.dither_codes(disp, 0.5)}


def _write(ctx, rr, scene, tmp_path, name, fmt):
    out = str(tmp_path / name)
    ctx.render_frame(scene, FRAME, _params(rr), out, fmt, 90)
    ext = {"JPEG": ".jpg", "PNG": ".png", "OPEN_EXR": ".exr"}[fmt]
    return open(out + ext, "rb").read()


def _decode(png_bytes):
    return np.asarray(Image.open(io.BytesIO(png_bytes)))


def test_files_hold_the_dithered_image(dctx, rr, frame04, tmp_path):
    s = dctx.load_scene(S04)
    try:
        dctx.set_dither(1.0)
        want = frame04[1.0]
        assert not np.array_equal(want, frame04["plain"])
        for device in (False, True):
            dctx.set_device_png(device)
            dctx.set_color_mode(0)
            px = _decode(_write(dctx, rr, s, tmp_path, f"rgba{int(device)}", "PNG"))
            assert px.shape == want.shape and np.array_equal(px, want), f"device coder {device}"
            dctx.set_color_mode("BW")
            grey = _decode(_write(dctx, rr, s, tmp_path, f"bw{int(device)}", "PNG"))
            assert grey.shape == (H, W) and np.array_equal(grey, CM.grey8(want)), f"BW, device coder {device}"
        dctx.set_color_mode(0)
        jpg = _write(dctx, rr, s, tmp_path, "frame", "JPEG")
        assert jpg == dctx.jpeg_device(want, 90)
        assert jpg != dctx.jpeg_device(frame04["plain"], 90)
    finally:
        s.close()


def test_intensity_zero_and_other_formats_unchanged(dctx, rr, frame04, tmp_path):
    """Intensity 0 writes the files of a context that never heard of the
    setting; 16-bit PNG and OPEN_EXR files are the same at intensity 1."""
    def files(c, s, tag, formats):
        out = {}
        for fmt, device, png_depth, exr_depth in formats:
            c.set_device_png(device)
            c.set_png_depth(png_depth)
            c.set_exr_depth(exr_depth)
            out[(fmt, device, png_depth, exr_depth)] = _write(c, rr, s, tmp_path, tag, fmt)
        return out

    eight = [("JPEG", False, 0, 0), ("PNG", False, 0, 0), ("PNG", True, 0, 0)]
    deep = [("PNG", False, 16, 0), ("OPEN_EXR", False, 0, 16), ("OPEN_EXR", False, 0, 32)]
    with rr.RenderContext(0) as fresh:
        s = fresh.load_scene(S04)
        try:
            never = files(fresh, s, "never", eight + deep)
        finally:
            s.close()
    s = dctx.load_scene(S04)
    try:
        dctx.set_dither(1.0)
        on = files(dctx, s, "on", eight + deep)
        dctx.set_dither(0.0)
        off = files(dctx, s, "off", eight + deep)
    finally:
        s.close()
    for k in eight + deep:
        assert off[k] == never[k], k
    for k in deep:
        assert on[k] == never[k], k
    for k in eight:
        assert on[k] != never[k], k
    assert np.array_equal(_decode(never[eight[1]]), frame04["plain"])


def _temp_scene(tmp_path, name, value):
    doc = json.load(open(S04))
    doc["render"].pop("dither_intensity", None)
    if value is not None:
        doc["render"]["dither_intensity"] = value
    p = str(tmp_path / name)
    with open(p, "w") as fh:
        json.dump(doc, fh)
    return p


def test_scene_value(dctx, rr, frame04, tmp_path):
    """RR_DITHER_SCENE takes the scene's render.dither_intensity (0 without
    one); any other value of the context's overrides it; a new context's is 0."""
    def rgba(scene_file, setting):
        dctx.set_dither(setting)
        s = dctx.load_scene(scene_file)
        try:
            return dctx.render_to_memory(s, FRAME, _params(rr))[1]
        finally:
            s.close()

    half = _temp_scene(tmp_path, "half.rrscene", 0.5)
    none = _temp_scene(tmp_path, "none.rrscene", None)
    assert np.array_equal(rgba(half, "scene"), frame04[0.5])
    assert np.array_equal(rgba(half, 0.5), frame04[0.5])
    assert np.array_equal(rgba(none, "scene"), frame04["plain"])
    assert np.array_equal(rgba(half, 0.0), frame04["plain"])
    assert np.array_equal(rgba(half, 1.0), frame04[1.0])
    assert np.array_equal(rgba(S04, "scene"), frame04[1.0])  # the committed scene says 1.0
    with rr.RenderContext(0) as fresh:  # the default: 0 although the scene says 1.0
        s = fresh.load_scene(S04)
        try:
            assert np.array_equal(fresh.render_to_memory(s, FRAME, _params(rr))[1], frame04["plain"])
        finally:
            s.close()


def test_environment_and_constructor(rr, frame04, monkeypatch):
    def rgba(**kw):
        with rr.RenderContext(0, **kw) as c:
            s = c.load_scene(S04)
            try:
                return c.render_to_memory(s, FRAME, _params(rr))[1]
            finally:
                s.close()

    monkeypatch.setenv("RR_DITHER", "0.5")
    assert np.array_equal(rgba(), frame04[0.5])
    assert np.array_equal(rgba(dither=0.0), frame04["plain"])
    monkeypatch.setenv("RR_DITHER", "scene")
    assert np.array_equal(rgba(), frame04[1.0])
    monkeypatch.setenv("RR_DITHER", "")
    assert np.array_equal(rgba(), frame04["plain"])
    for bad in ("2.5", "-1", "on", "nan", "1x"):
        monkeypatch.setenv("RR_DITHER", bad)
        with pytest.raises(rr.RRError) as e:
            rr.RenderContext(0)
        assert e.value.code == rr.native.RR_EINVAL and "RR_DITHER" in str(e.value)
    monkeypatch.delenv("RR_DITHER")
    assert np.array_equal(rgba(dither=1.0), frame04[1.0])
    assert np.array_equal(rgba(dither="scene"), frame04[1.0])


def test_frames_in_flight_keep_their_setting(dctx, rr, frame04, tmp_path):
    s = dctx.load_scene(S04)
    try:
        tickets = []
        for k, g in enumerate((0.0, 1.0, 0.0)):
            dctx.set_dither(g)
            tickets.append(dctx.submit_frame(s, FRAME, _params(rr), str(tmp_path / f"f{k}"), "PNG"))
        dctx.set_dither(2.0)  # after the submits: none of the three takes it
        for t in tickets:
            dctx.complete_frame(t)
        got = [_decode(open(str(tmp_path / f"f{k}.png"), "rb").read()) for k in range(3)]
        assert np.array_equal(got[0], frame04["plain"])
        assert np.array_equal(got[1], frame04[1.0])
        assert np.array_equal(got[2], frame04["plain"])
    finally:
        s.close()
