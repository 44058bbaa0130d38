"""Colour modes on the device: every format x depth x mode through
rr_debug_encode_device decodes to the restatement of tests/color_modes.py bit
for bit; JPEG BW bytes equal the host encoder's; rendered frames on both render
paths; frames in flight keep the mode of their submit; scene field, setter and
environment; the runner; sizes outside a plan."""
import io
import json

import numpy as np
import pytest
from PIL import Image

import color_modes as M
import exr_reader as X
from conftest import scene_path

pytestmark = pytest.mark.gpu

S04 = scene_path("04_very-simple-standin.rrscene")
SIZES = [(1, 1), (2, 1), (3, 17), (64, 15), (333, 33), (513, 16)]
MODES = ["BW", "RGB", "RGBA"]


def _sizes(mode):
    # a PNG 8 grey row of 4098 bytes crosses the 4096-byte chunk inside a row
    return SIZES + ([(4097, 17)] if mode == "BW" else [])


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} samples differ, first at {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


@pytest.mark.parametrize("mode", MODES)
def test_png8_round_trip(ctx, mode):
    c = M.MODES[mode]
    for w, h in _sizes(mode):
        for kind in M.KINDS:
            img = M.rgba8_image(kind, w, h, seed=w + h)
            data = ctx.encode_device("PNG", img, 8, mode)
            px, info = M.read_png(data)
            assert info["depth"] == 8 and info["colour_type"] == M.COLOUR_TYPE[c]
            want = M.expected_png8(img, c)
            _same(px, want, (kind, w, h))
            assert info["raw"] == M.png_front_bytes(want, 8)
            im = Image.open(io.BytesIO(data))
            assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[c]
            _same(np.asarray(im).reshape(h, w, c), want, ("PIL", kind, w, h))


@pytest.mark.parametrize("view", [0, 1])
@pytest.mark.parametrize("mode", MODES)
def test_png16_round_trip(ctx, rr, mode, view):
    c = M.MODES[mode]
    table = rr.native.srgb16_table()
    for w, h in _sizes(mode):
        for kind in M.KINDS:
            img = M.float_image(kind, w, h, seed=w + h)
            data = ctx.encode_device("PNG", img, 16, mode, view_transform=view, exposure_scale=1.25)
            px, info = M.read_png(data)
            assert info["depth"] == 16 and info["colour_type"] == M.COLOUR_TYPE[c]
            want = M.expected_png16(img, c, view, 1.25, table)
            _same(px, want, (kind, w, h))
            if c == 1:  # PIL reads 16-bit grey at full precision
                im = Image.open(io.BytesIO(data))
                assert im.mode in ("I;16", "I;16B")
                _same(np.asarray(im).astype(np.uint16).reshape(h, w, 1), want, ("PIL", kind, w, h))


@pytest.mark.parametrize("depth", [16, 32])
@pytest.mark.parametrize("mode", MODES)
def test_exr_round_trip(ctx, mode, depth):
    c = M.MODES[mode]
    for w, h in _sizes(mode):
        for kind in M.KINDS:
            img = M.float_image(kind, w, h, seed=w + h)
            px, info = M.read_exr(ctx.encode_device("OPEN_EXR", img, depth, mode))
            assert info["channels"] == M.EXR_CHANNELS[c] and info["pixel_type"] == (2 if depth == 32 else 1)
            _same(px, M.expected_exr(img, c, depth == 32), (kind, w, h))


@pytest.mark.parametrize("depth", [16, 32])
@pytest.mark.parametrize("mode", ["BW", "RGB"])
def test_exr_raw_chunks(ctx, mode, depth):
    """Random bit patterns do not deflate: the chunks carry their raw bytes."""
    c = M.MODES[mode]
    rng = np.random.default_rng(11)
    if depth == 32:  # every float bit pattern but NaN and infinity
        b = rng.integers(0, 1 << 32, (33, 128, 4), dtype=np.uint32)
        b = np.where((b & 0x7F800000) == 0x7F800000, b & np.uint32(0xBFFFFFFF), b).astype(np.uint32)
        img = b.view(np.float32).copy()
    else:  # every half bit pattern but NaN and infinity
        img = X.make_image("bits", 128, 33, seed=11)
    if c == 1:  # Y = 0.2126 r of r = pattern / 0.2126: as random as the patterns
        with np.errstate(all="ignore"):
            img[..., 0] = img[..., 0] / np.float32(0.2126)
        img[..., 1:3] = 0.0
    px, info = M.read_exr(ctx.encode_device("OPEN_EXR", img, depth, mode))
    with np.errstate(all="ignore"):
        _same(px, M.expected_exr(img, c, depth == 32), (mode, depth))
    assert "raw" in info["modes"], info["modes"]


@pytest.mark.parametrize("quality", [50, 90])
@pytest.mark.parametrize("w,h", [(1, 1), (7, 9), (8, 8), (17, 33), (250, 141)])
def test_jpeg_bw_equals_host(ctx, rr, tmp_path, w, h, quality):
    for img in (M.smooth_image(w, h), M.rgba8_image("noise", w, h, seed=3)):
        dev = ctx.encode_device("JPEG", img, 8, "BW", quality=quality)
        rr.encode_image_mode(img, str(tmp_path / "h"), "JPEG", quality, "BW")
        assert dev == (tmp_path / "h.jpg").read_bytes()
        im = Image.open(io.BytesIO(dev))
        assert im.mode == "L" and im.size == (w, h)
        im.load()
    # RGB and RGBA are the three-component file of rr_debug_jpeg_device
    img = M.smooth_image(w, h)
    for mode in ("RGB", "RGBA", 0):
        assert ctx.encode_device("JPEG", img, 8, mode, quality=quality) == ctx.jpeg_device(img, quality)


def test_default_modes_are_the_old_entries(ctx):
    img8 = M.rgba8_image("gradient", 333, 33)
    assert ctx.encode_device("PNG", img8, 8, 0) == ctx.png_device(img8)
    assert ctx.encode_device("PNG", img8, 8, "RGBA") == ctx.png_device(img8)
    f = M.float_image("gradient", 333, 33)
    assert ctx.encode_device("PNG", f, 16, 0, view_transform=0, exposure_scale=1.5) == ctx.png16_device(f, 0, 1.5)
    f[..., 3] = 1.0  # the old entries take alpha from the image
    assert ctx.encode_device("OPEN_EXR", f, 16, 0) == ctx.exr_device(f)
    assert ctx.encode_device("OPEN_EXR", f, 32, "RGBA") == ctx.exr32_device(f)


def _frame_files(c, rr, s, p, tmp, tag, mode, frame=3):
    """The six files of a frame in `mode`: name -> bytes."""
    c.set_color_mode(mode)
    out = {}
    jobs = [("png8h", "PNG", dict(png=False, pd=8)), ("png8d", "PNG", dict(png=True, pd=8)),
            ("png16", "PNG", dict(png=False, pd=16)), ("exr16", "OPEN_EXR", dict(ed=16)),
            ("exr32", "OPEN_EXR", dict(ed=32)), ("jpeg", "JPEG", {})]
    ext = {"PNG": ".png", "OPEN_EXR": ".exr", "JPEG": ".jpg"}
    try:
        for name, fmt, o in jobs:
            c.set_device_png(o.get("png", False))
            c.set_png_depth(o.get("pd", 0))
            c.set_exr_depth(o.get("ed", 0))
            c.render_frame(s, frame, p, str(tmp / f"{tag}{name}"), fmt, 90)
            out[name] = (tmp / f"{tag}{name}{ext[fmt]}").read_bytes()
    finally:
        c.set_device_png(False)
        c.set_png_depth(0)
        c.set_exr_depth(0)
        c.set_color_mode(0)
    return out


@pytest.mark.parametrize("path", ["tiles", "wavefront"])
def test_rendered_frames(ctx, rr, tmp_path, path):
    flags = rr.native.RR_FLAG_WAVEFRONT if path == "wavefront" else 0
    p = rr.default_params(spp=4, width=250, height=141, flags=flags)
    s = ctx.load_scene(S04)
    try:
        film, rgba8, _ = ctx.render_to_memory(s, 3, p)
        scale = float(ctx.frame_state(s, 3, p).render_floats[2])
        full = _frame_files(ctx, rr, s, p, tmp_path, "a", "RGBA")
        none = _frame_files(ctx, rr, s, p, tmp_path, "n", 0)
        assert full == none  # RGBA (JPEG: RGB) is what a context without a mode writes
        rgb = _frame_files(ctx, rr, s, p, tmp_path, "c", "RGB")
        bw = _frame_files(ctx, rr, s, p, tmp_path, "g", "BW")
        table = rr.native.srgb16_table()
        for name in ("png8h", "png8d"):
            a = M.read_png(full[name])[0]
            _same(a[..., :3], rgba8[..., :3], name)
            _same(M.read_png(rgb[name])[0], a[..., :3], name + " RGB")
            _same(M.read_png(bw[name])[0], M.grey8(a)[..., None], name + " BW")
        a = M.read_png(full["png16"])[0]
        _same(M.read_png(rgb["png16"])[0], a[..., :3], "png16 RGB")
        _same(M.read_png(bw["png16"])[0], M.expected_png16(film, 1, 0, scale, table), "png16 BW")
        for name, is32 in (("exr16", False), ("exr32", True)):
            a = M.read_exr(full[name])[0]
            _same(a, M.expected_exr(film, 4, is32), name)
            _same(M.read_exr(rgb[name])[0], a[..., 1:], name + " RGB")
            _same(M.read_exr(bw[name])[0], M.expected_exr(film, 1, is32), name + " BW")
        assert rgb["jpeg"] == full["jpeg"]
        rr.encode_image_mode(rgba8, str(tmp_path / "hj"), "JPEG", 90, "BW")
        assert bw["jpeg"] == (tmp_path / "hj.jpg").read_bytes()
        assert Image.open(io.BytesIO(bw["jpeg"])).mode == "L"
    finally:
        s.close()


@pytest.mark.parametrize("which", ["04vs", "02"])
def test_file_sizes_against_zlib_level_1(ctx, rr, tmp_path, which):
    """Rendered frames in BW and RGB: every deflate-coded file is at most 1.25
    times the same file with its front-end bytes deflated by zlib level 1 (the
    bound DESIGN section 8 applies to every front end of the coder)."""
    s = ctx.load_scene(S04 if which == "04vs" else scene_path("02_physics-standin.rrscene"))
    p = rr.default_params(spp=4, width=250, height=141)
    try:
        for mode in ("BW", "RGB"):
            files = _frame_files(ctx, rr, s, p, tmp_path, which + mode, mode)
            for name, data in files.items():
                if name in ("png8h", "jpeg"):
                    continue
                if name.startswith("png"):
                    ref = M.png_zlib1_file_bytes(data, M.read_png(data)[1])
                else:
                    ref = M.read_exr(data)[1]["zlib1_file_bytes"]
                print(f"{which} {mode} {name}: device {len(data)} bytes, zlib level 1 {ref}, ratio {len(data) / ref:.4f}")
                assert len(data) <= 1.25 * ref, (which, mode, name)
    finally:
        s.close()


def test_png16_bw_filmic(ctx, rr, tmp_path):
    """Filmic has no numpy restatement. The BW sample is quantize16(luma(d)) of
    the floats d whose quantize16 the RGB file holds: |65535 d - q| <= 0.5 a
    channel and the weights sum to 1, so 65535 luma(d) is within 0.5 of the
    luma L of the RGB file's codes, and its rounding within 1 of L (plus the
    float32 error of three products and two sums at 65535, below 0.02)."""
    from oracle import host_oracle as HO
    HO.write_synthetic_filmic_luts(str(tmp_path), n3=33, n1=4096)
    ctx.set_ocio_config(str(tmp_path))
    try:
        for kind in ("gradient", "noise", "grey"):
            img = M.float_image(kind, 129, 33, seed=5)
            rgb = M.read_png(ctx.encode_device("PNG", img, 16, "RGB", view_transform=2, exposure_scale=1.25))[0]
            bw = M.read_png(ctx.encode_device("PNG", img, 16, "BW", view_transform=2, exposure_scale=1.25))[0]
            rgba = M.read_png(ctx.encode_device("PNG", img, 16, "RGBA", view_transform=2, exposure_scale=1.25))[0]
            _same(rgb, rgba[..., :3], kind)
            assert len(np.unique(rgb)) > 16, "the image exercises the chain"
            q = rgb.astype(np.float64)
            L = 0.2126 * q[..., 0] + 0.7152 * q[..., 1] + 0.0722 * q[..., 2]
            err = np.abs(bw[..., 0].astype(np.float64) - L)
            print(f"filmic BW {kind}: max |BW - luma(RGB codes)| = {err.max():.4f} (bound 1.02)")
            assert err.max() <= 1.02
    finally:
        ctx.set_ocio_config(None)


def _mode_of(data):
    if data[:2] == b"\xff\xd8":
        return {"L": "BW", "RGB": "RGB"}[Image.open(io.BytesIO(data)).mode]
    if data[:4] == b"\x89PNG":
        return {1: "BW", 3: "RGB", 4: "RGBA"}[M.read_png(data)[1]["channels"]]
    return {1: "BW", 3: "RGB", 4: "RGBA"}[len(M.read_exr(data)[1]["channels"])]


def test_frames_in_flight_keep_their_mode(ctx, rr, tmp_path):
    s = ctx.load_scene(S04)
    p = rr.default_params(spp=4, width=250, height=141)
    try:
        films = {f: ctx.render_to_memory(s, f, p)[0] for f in (3, 4, 5)}
        for fmt, ext in (("OPEN_EXR", ".exr"), ("PNG", ".png"), ("JPEG", ".jpg")):
            tickets = []
            for f, mode in ((3, "BW"), (4, "RGB"), (5, "RGBA")):
                ctx.set_color_mode(mode)
                tickets.append(ctx.submit_frame(s, f, p, str(tmp_path / f"f{f}"), fmt, 90))
            ctx.set_color_mode("BW")  # frames in flight keep the mode of their submit
            for t in tickets:
                ctx.complete_frame(t)
            got = [_mode_of((tmp_path / f"f{f}{ext}").read_bytes()) for f in (3, 4, 5)]
            assert got == ["BW", "RGB", "RGBA" if fmt != "JPEG" else "RGB"], fmt
            if fmt == "OPEN_EXR":
                for f, c in ((3, 1), (4, 3), (5, 4)):
                    _same(M.read_exr((tmp_path / f"f{f}.exr").read_bytes())[0], M.expected_exr(films[f], c, False), f)
    finally:
        ctx.set_color_mode(0)
        s.close()


def test_scene_setter_environment(rr, tmp_path, monkeypatch):
    with open(S04) as f:
        j = json.load(f)
    j["render"]["color_mode"] = "BW"
    (tmp_path / "bw.rrscene").write_text(json.dumps(j))
    sbw = str(tmp_path / "bw.rrscene")
    p = rr.default_params(spp=2, width=64, height=36)

    def mode_of(c, scene_file, name, fmt="PNG"):
        s = c.load_scene(scene_file)
        try:
            c.render_frame(s, 3, p, str(tmp_path / name), fmt, 90)
        finally:
            s.close()
        return _mode_of((tmp_path / (name + {"PNG": ".png", "JPEG": ".jpg", "OPEN_EXR": ".exr"}[fmt])).read_bytes())

    monkeypatch.delenv("RR_COLOR_MODE", raising=False)
    with rr.RenderContext(0) as c:
        assert mode_of(c, S04, "a") == "RGBA" and mode_of(c, S04, "a", "JPEG") == "RGB"
        assert mode_of(c, S04, "a", "OPEN_EXR") == "RGBA"
        assert mode_of(c, sbw, "b") == "BW" and mode_of(c, sbw, "b", "JPEG") == "BW"
        c.set_color_mode("RGB")  # the context's mode goes before the scene's
        assert mode_of(c, sbw, "c") == "RGB"
        c.set_color_mode(0)
        assert mode_of(c, sbw, "d") == "BW"
        for bad in (2, 5, -1, 32):
            with pytest.raises(rr.RRError) as e:
                c.set_color_mode(bad)
            assert e.value.code == rr.native.RR_EINVAL
        assert mode_of(c, sbw, "d2") == "BW"  # a refused value changes nothing
    monkeypatch.setenv("RR_COLOR_MODE", "RGB")
    with rr.RenderContext(0) as c:
        assert mode_of(c, S04, "e") == "RGB" and mode_of(c, sbw, "e2") == "RGB"
        c.set_color_mode("BW")  # the setter goes before the environment
        assert mode_of(c, S04, "e3") == "BW"
    monkeypatch.setenv("RR_COLOR_MODE", "")
    with rr.RenderContext(0) as c:
        assert mode_of(c, S04, "f") == "RGBA"
    monkeypatch.setenv("RR_COLOR_MODE", "GREY")
    with pytest.raises(rr.RRError) as e:
        rr.RenderContext(0)
    assert e.value.code == rr.native.RR_EINVAL
    monkeypatch.delenv("RR_COLOR_MODE")
    with rr.RenderContext(0, color_mode="BW") as c:
        assert mode_of(c, S04, "g", "OPEN_EXR") == "BW"


def test_backend_runner_color_mode(rr, tmp_path):
    import os
    from conftest import ROOT
    job = rr.BlenderJob.load_from_file(os.path.join(ROOT, "jobs", "04_very-simple_demo_10f-1w.toml"))
    job = rr.BlenderJob.from_dict({**job.to_dict(), "output_directory_path": str(tmp_path / "out"),
                                   "output_file_format": "PNG"})
    runner = rr.BackendRunner(ROOT, params=rr.default_params(spp=2, width=64, height=36), color_mode="BW")
    try:
        runner.render_frame(job, 3)
    finally:
        runner.close()
    files = sorted((tmp_path / "out").glob("*.png"))
    assert len(files) == 1 and _mode_of(files[0].read_bytes()) == "BW"


def test_sizes_outside_a_plan_are_refused(ctx, rr):
    """Widths above the plans' bounds (2^20 PNG 8, 2^19 PNG 16 and HALF, 2^18
    FLOAT) and a JPEG above 65535: RR_EINVAL, in every mode, before any launch
    (the image is not read: the call would fault on the short buffer otherwise)."""
    tiny8, tinyf = np.zeros((1, 1, 4), np.uint8), np.zeros((1, 1, 4), np.float32)
    import ctypes
    L = rr.lib()
    n = ctypes.c_uint64()
    for mode in (1, 3, 4):
        for fmt, depth, img, isf, w in ((b"PNG", 8, tiny8, 0, (1 << 20) + 1), (b"PNG", 16, tinyf, 1, (1 << 19) + 1),
                                        (b"OPEN_EXR", 16, tinyf, 1, (1 << 19) + 1),
                                        (b"OPEN_EXR", 32, tinyf, 1, (1 << 18) + 1), (b"JPEG", 8, tiny8, 0, 65536)):
            rc = L.rr_debug_encode_device(ctx.handle, fmt, depth, mode, img.ctypes.data_as(ctypes.c_void_p), isf, w, 1,
                                          0, ctypes.c_float(1.0), 90, None, 0, ctypes.byref(n))
            assert rc == rr.native.RR_EINVAL, (fmt, depth, mode)
    for args in (("PNG", tiny8, 16), ("OPEN_EXR", tiny8, 16), ("PNG", tinyf, 8), ("JPEG", tinyf, 8), ("TIFF", tiny8, 8),
                 ("PNG", tiny8, 12)):
        with pytest.raises(rr.RRError) as e:
            ctx.encode_device(args[0], args[1], args[2], "RGB")
        assert e.value.code == rr.native.RR_EINVAL
    with pytest.raises(rr.RRError):
        ctx.encode_device("PNG", tiny8, 8, 2)
