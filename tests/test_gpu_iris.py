"""IRIS on the device (iris.hip): the coder's bytes equal the host coder's and the
restatement of tests/iris.py at every size and image of the host tests and at
the shapes where the kernels' steps meet; rendered frames decode to the pixels
of the TARGA_RAW file of the same frame, with BW, RGB and dither; frames in
flight beside a PNG frame write their solo files; the coder's time is reported;
the shim; sizes outside the format are refused before any launch."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import iris as I
from conftest import PKG, ROOT, scene_path

pytestmark = pytest.mark.gpu

S04 = scene_path("04_very-simple-standin.rrscene")
MODES = {"BW": 1, "RGB": 3, "RGBA": 4}
CHUNK = 256  # bytes a workgroup of k_iris_size takes of its row-plane per step (iris.hpp kIrisChunk)
IMAGES = {**I.images(), **I.device_images(CHUNK)}
WANT = {}  # (name, c) -> the restatement's file, computed once


def _want(name, c):
    if (name, c) not in WANT:
        WANT[(name, c)] = I.encode(IMAGES[name], c)
    return WANT[(name, c)]


def _device_file(ctx, rr, img, c, depth=8):
    """One rr_debug_encode_device call into a buffer above the all-literal bound."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    out = np.zeros(I.HEADER + I.body_bound(w, h, c) + 64, np.uint8)
    n = ctypes.c_uint64()
    rc = rr.lib().rr_debug_encode_device(ctx.handle, b"IRIS", depth, c, img.ctypes.data_as(ctypes.c_void_p), 0, w, h, 0,
                                         ctypes.c_float(1.0), 90, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                         out.size, ctypes.byref(n))
    assert rc == 0, rr.lib().rr_last_error(ctx.handle)
    assert n.value <= out.size - 64, "a file above the all-literal bound"
    return out[:n.value].tobytes()


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} samples differ, first at {bad[0]}"


def _pil(data, w, h, c):
    im = Image.open(io.BytesIO(data))
    assert im.size == (w, h) and im.mode == I.PIL_MODE[c], (im.size, im.mode)
    return np.asarray(im).reshape(h, w, c)


def test_chunk_is_the_kernels(rr):
    with open(os.path.join(ROOT, PKG, "csrc", "iris.hpp")) as f:
        assert f"constexpr int kIrisChunk = {CHUNK};" in f.read()


@pytest.mark.parametrize("mode", ["BW", "RGB", "RGBA"])
def test_device_equals_host_and_restatement(ctx, rr, tmp_path, mode):
    c = MODES[mode]
    for name, img in IMAGES.items():
        dev = _device_file(ctx, rr, img, c)
        want = _want(name, c)
        assert dev == want, (name, len(dev), len(want), "device file differs from the restatement")
        rr.encode_image_mode(img, str(tmp_path / "h"), "IRIS", 90, mode)
        assert dev == (tmp_path / "h.rgb").read_bytes(), (name, "device file differs from the host coder's")
    # the strict reader and PIL on the device's own bytes at the step shapes
    for name in ("across steps", "tall 9x700", "random 257x2"):
        img = IMAGES[name]
        h, w = img.shape[:2]
        dev = _device_file(ctx, rr, img, c)
        _same(I.read(dev)[0], I.expected(img, c), name)
        _same(_pil(dev, w, h, c), I.expected(img, c), ("PIL", name))
    # encode_device (two calls: the length, then the bytes) gives the same file, and depth 0 is 8
    img = IMAGES["across steps"]
    assert ctx.encode_device("IRIS", img, 0, mode) == _want("across steps", c)
    if mode == "RGBA":
        assert ctx.encode_device("IRIS", img, 8, 0) == _want("across steps", 4)  # no mode: RGBA
    # the same image after another: the same bytes
    assert _device_file(ctx, rr, IMAGES["random 300x17"], c) == _want("random 300x17", c)


def _render_file(ctx, s, frame, p, tmp_path, name, fmt):
    ctx.render_frame(s, frame, p, str(tmp_path / name), fmt, 90)
    return (tmp_path / (name + rr_ext(fmt))).read_bytes()


def rr_ext(fmt):
    return {"IRIS": ".rgb", "TARGA": ".tga", "TARGA_RAW": ".tga", "PNG": ".png"}[fmt]


@pytest.mark.parametrize("dither", [0.0, 1.0])
@pytest.mark.parametrize("mode", [0, "BW", "RGB"])
def test_rendered_frames(ctx, rr, tmp_path, mode, dither):
    c = {0: 4, "BW": 1, "RGB": 3}[mode]
    w, h = 250, 141
    p = rr.default_params(spp=4, width=w, height=h)
    s = ctx.load_scene(S04)
    ctx.set_dither(dither)
    ctx.set_color_mode(mode)
    ctx.set_png_depth(16)  # an IRIS file is 8 bits a channel whatever the depth
    try:
        data = _render_file(ctx, s, 3, p, tmp_path, "a", "IRIS")
        raw = _render_file(ctx, s, 3, p, tmp_path, "a", "TARGA_RAW")
        px = _pil(data, w, h, c)
        assert len(np.unique(px)) > 16
        _same(px, _pil(raw, w, h, c), "IRIS against TARGA_RAW")
        got, info = I.read(data)
        assert info["channels"] == c
        _same(got, px, "the strict reader against PIL")
        if c == 4:
            assert np.all(px[..., 3] == 255)
        # and the file is the restatement's of the frame's 8-bit image
        rgba8 = ctx.render_to_memory(s, 3, p)[1]
        assert data == I.encode(rgba8, c)
    finally:
        ctx.set_dither(0.0)
        ctx.set_color_mode(0)
        ctx.set_png_depth(0)
        s.close()


def test_dither_changes_the_file(ctx, rr, tmp_path):
    """The file is coded after the view pass: the dithered frame's differs."""
    p = rr.default_params(spp=4, width=160, height=90)
    s = ctx.load_scene(S04)
    try:
        plain = _render_file(ctx, s, 3, p, tmp_path, "p", "IRIS")
        ctx.set_dither(1.0)
        dithered = _render_file(ctx, s, 3, p, tmp_path, "d", "IRIS")
        assert dithered != plain
        assert not np.array_equal(I.read(dithered)[0], I.read(plain)[0])
    finally:
        ctx.set_dither(0.0)
        s.close()


def test_frames_in_flight_and_beside_png(ctx, rr, tmp_path):
    p = rr.default_params(spp=4, width=160, height=90)
    s = ctx.load_scene(S04)
    ctx.set_device_png(True)
    try:
        solo = {f: _render_file(ctx, s, f, p, tmp_path, f"solo{f}", "IRIS") for f in (3, 4, 5)}
        assert len(set(solo.values())) == 3
        png4 = _render_file(ctx, s, 4, p, tmp_path, "solo4", "PNG")
        # three frames in flight
        tickets = [ctx.submit_frame(s, f, p, str(tmp_path / f"fl{f}"), "IRIS", 90) for f in (3, 4, 5)]
        for t in tickets:
            ctx.complete_frame(t)
        for f in (3, 4, 5):
            assert (tmp_path / f"fl{f}.rgb").read_bytes() == solo[f], f
        # three IRIS frames around a device PNG frame, in flight together
        order = ((3, "IRIS"), (4, "PNG"), (4, "IRIS"), (5, "IRIS"))
        tickets = []
        for i, (f, fmt) in enumerate(order[:3]):
            tickets.append(ctx.submit_frame(s, f, p, str(tmp_path / f"mix{i}"), fmt, 90))
        ctx.complete_frame(tickets[0])
        tickets.append(ctx.submit_frame(s, 5, p, str(tmp_path / "mix3"), "IRIS", 90))
        for t in tickets[1:]:
            ctx.complete_frame(t)
        for i, (f, fmt) in enumerate(order):
            want = solo[f] if fmt == "IRIS" else png4
            assert (tmp_path / f"mix{i}{rr_ext(fmt)}").read_bytes() == want, (i, f, fmt)
        # and one after the other, beside TARGA frames of the same slot buffers
        for k, (f, fmt) in enumerate(((4, "PNG"), (3, "IRIS"), (3, "TARGA"), (5, "IRIS"))):
            ctx.render_frame(s, f, p, str(tmp_path / f"seq{k}"), fmt, 90)
        assert (tmp_path / "seq0.png").read_bytes() == png4
        assert (tmp_path / "seq1.rgb").read_bytes() == solo[3] and (tmp_path / "seq3.rgb").read_bytes() == solo[5]
    finally:
        ctx.set_device_png(False)
        s.close()


def test_coder_time_is_reported(ctx, rr, tmp_path):
    p = rr.default_params(spp=2, width=160, height=90, flags=rr.native.RR_FLAG_PROFILE_KERNELS)
    s = ctx.load_scene(S04)
    try:
        _, st = ctx.render_frame(s, 3, p, str(tmp_path / "t"), "IRIS", 90)
        assert st.kernel_launches[rr.native.RR_K_PNG] == 1 and st.kernel_ms[rr.native.RR_K_PNG] > 0.0
        assert st.output_bytes == (tmp_path / "t.rgb").stat().st_size
    finally:
        s.close()


def test_shim_writes_rgb(rr, tmp_path):
    out_fmt = str(tmp_path / "######")
    env = dict(os.environ, RR_WIDTH="64", RR_HEIGHT="36", RR_SPP="2")
    argv = [rr.SHIM_PATH, S04.replace(".rrscene", ".blend"), "--background", "--python", "script.py", "--",
            "--render-output", out_fmt, "--render-format", "IRIS", "--render-frame", "12"]
    res = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"Saved: '{tmp_path}/000012.rgb'" in res.stdout
    px, info = I.read((tmp_path / "000012.rgb").read_bytes())
    assert px.shape == (36, 64, 4) and info["channels"] == 4 and len(np.unique(px[..., :3])) > 4


def test_sizes_outside_the_format_are_refused(ctx, rr, tmp_path):
    """RR_EINVAL before any launch: the image is not read (it is one pixel)."""
    tiny = np.zeros((1, 1, 4), np.uint8)
    n = ctypes.c_uint64()
    L = rr.lib()
    ptr = tiny.ctypes.data_as(ctypes.c_void_p)
    for mode in (0, 1, 3, 4):
        for w, h in ((65536, 1), (1, 65536), (65535, 65535), (32768, 65535)):
            rc = L.rr_debug_encode_device(ctx.handle, b"IRIS", 8, mode, ptr, 0, w, h, 0, ctypes.c_float(1.0), 90, None, 0,
                                          ctypes.byref(n))
            assert rc == rr.native.RR_EINVAL, (mode, w, h)
    # the bound counts the channels: 65535 x 9000 is inside it with three and outside with four
    rc = L.rr_debug_encode_device(ctx.handle, b"IRIS", 8, 4, ptr, 0, 65535, 9000, 0, ctypes.c_float(1.0), 90, None, 0,
                                  ctypes.byref(n))
    assert rc == rr.native.RR_EINVAL
    # 8 bits a channel and no other depth; no float image
    for depth, isf in ((16, 0), (32, 0), (8, 1), (0, 1)):
        rc = L.rr_debug_encode_device(ctx.handle, b"IRIS", depth, 4, ptr, isf, 1, 1, 0, ctypes.c_float(1.0), 90, None, 0,
                                      ctypes.byref(n))
        assert rc == rr.native.RR_EINVAL, (depth, isf)
    # a frame of such a size is refused when it is submitted, and the context goes on
    s = ctx.load_scene(S04)
    try:
        with pytest.raises(rr.RRError) as e:
            ctx.submit_frame(s, 3, rr.default_params(spp=1, width=65536, height=1), str(tmp_path / "big"), "IRIS", 90)
        assert e.value.code == rr.native.RR_EINVAL and "IRIS" in str(e.value)
        assert not (tmp_path / "big.rgb").exists()
        assert _device_file(ctx, rr, tiny, 4) == I.encode(tiny, 4)
    finally:
        s.close()
