"""WEBP on the device (webp.hip): the coder's bytes equal the host coder's and the
restatement of tests/webp.py in every colour mode at the shapes where the
kernels' steps, the copy limit and the codes' forms meet, and PIL (libwebp)
decodes the device's own bytes to the pixels; rendered frames decode to the
pixels of the TARGA_RAW file of the same frame, with BW, RGB and dither; a
quality below 100 is flagged and changes no byte; frames in flight beside a PNG
frame write their solo files; the coder's time is reported; the shim; sizes
outside the format are refused before any launch."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import webp as W
from conftest import PKG, ROOT, scene_path

pytestmark = pytest.mark.gpu

S04 = scene_path("04_very-simple-standin.rrscene")
MODES = {"BW": 1, "RGB": 3, "RGBA": 4}
CHUNK = 256  # pixels a workgroup takes of its row per step (webp.hpp kWebpChunk)
IMAGES = W.device_images(CHUNK)
WANT = {}  # (name, c) -> (the restatement's file, its info), computed once


def _want(name, c):
    if (name, c) not in WANT:
        info = {}
        WANT[(name, c)] = (W.encode(IMAGES[name], c, info), info)
    return WANT[(name, c)]


def _device_file(ctx, rr, img, c, depth=8, quality=100):
    """One rr_debug_encode_device call into a buffer above the all-literal bound."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    out = np.zeros(W.file_bound(w, h) + 64, np.uint8)
    n = ctypes.c_uint64()
    rc = rr.lib().rr_debug_encode_device(ctx.handle, b"WEBP", depth, c, img.ctypes.data_as(ctypes.c_void_p), 0, w, h, 0,
                                         ctypes.c_float(1.0), quality,
                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), out.size, ctypes.byref(n))
    assert rc == 0, rr.lib().rr_last_error(ctx.handle)
    assert n.value <= out.size - 64, "a file above the all-literal bound"
    return out[:n.value].tobytes()


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} samples differ, first at {bad[0]}"


def _pil(data, w, h, c):
    im = Image.open(io.BytesIO(data))
    assert im.format == "WEBP" and im.size == (w, h) and im.mode == W.PIL_MODE[c], (im.size, im.mode)
    return np.asarray(im)


def test_chunk_is_the_kernels(rr):
    with open(os.path.join(ROOT, PKG, "csrc", "webp.hpp")) as f:
        assert f"constexpr int kWebpChunk = {CHUNK};" in f.read()


def test_images_are_the_named_ones():
    """The cases the shapes are there for, stated on the restatement's tokens and codes."""
    n = W.MIN_RUN
    copies = lambda row: [v for kind, v in row if kind == "copy"]  # noqa: E731
    toks = _want("stretches", 4)[1]["tokens"]
    want = [[m] if m >= n else [] for m in (2, 3)] + [[4096] + ([m - 4096] if m - 4096 >= n else [])
                                                      for m in (4096, 4097, 4098, 4099)]
    assert [copies(r) for r in toks[:6]] == want
    # a stretch to the row's last pixel, and the next row goes on with the same residual: a literal first
    assert toks[6][-1] == ("copy", 4) and toks[7][0][0] == "lit" and toks[7][1] == ("copy", 3)
    assert toks[7][0][1] == toks[6][-2][1]
    # 16383 pixels equal their left neighbour: four copies
    assert _want("flat row 16384", 4)[1]["tokens"] == [[("lit", 0), ("copy", 4096), ("copy", 4096), ("copy", 4096),
                                                         ("copy", 4095)]]
    forms = lambda name, c=4: [f["simple"] for f in _want(name, c)[1]["codes"]]  # noqa: E731
    assert forms("one colour 3x4") == [1, 2, 2, 1, 0]          # every code simple, no distance symbol
    assert forms("one colour 40x9")[1:] == [2, 2, 2, 1]        # the distance code: one symbol
    assert forms("two values 50x40") == [None, 2, 2, 2, 0]      # exactly two used symbols in red, blue and alpha
    assert forms("noise 64x64") == [None, None, None, None, 0]
    fib = _want("fibonacci 70x64", 4)[1]["codes"][0]
    assert fib["depth"] > 15 and fib["max_len"] == 15           # the unlimited tree is too deep: the repair works
    red = _want("uniform red 64x64", 4)[1]["codes"][1]
    assert red["cl_used"] == 1 and red["max_len"] == 8          # one used code length: it takes no bits


@pytest.mark.parametrize("mode", ["BW", "RGB", "RGBA"])
def test_device_equals_host_and_restatement(ctx, rr, tmp_path, mode):
    c = MODES[mode]
    for name, img in IMAGES.items():
        h, w = img.shape[:2]
        dev = _device_file(ctx, rr, img, c)
        want = _want(name, c)[0]
        assert dev == want, (name, len(dev), len(want), "device file differs from the restatement")
        rr.encode_image_mode(img, str(tmp_path / "h"), "WEBP", 100, mode)
        assert dev == (tmp_path / "h.webp").read_bytes(), (name, "device file differs from the host coder's")
        # PIL on the device's own bytes
        _same(_pil(dev, w, h, c), W.pil_expected(img, c), ("PIL", name))
    # the strict reader on the device's own bytes at the step shapes
    for name in ("across steps", "sparse 257x3", "one colour 40x9"):
        img = IMAGES[name]
        px, info = W.read(_device_file(ctx, rr, img, c))
        _same(px, W.expected(img, c), name)
        assert info["alpha"] == (1 if c == 4 else 0)
    # encode_device (two calls: the length, then the bytes) gives the same file, and depth 0 is 8
    img = IMAGES["across steps"]
    assert ctx.encode_device("WEBP", img, 0, mode, quality=100) == _want("across steps", c)[0]
    if mode == "RGBA":
        assert ctx.encode_device("WEBP", img, 8, 0, quality=100) == _want("across steps", 4)[0]  # no mode: RGBA
    # the same image after another: the same bytes
    assert _device_file(ctx, rr, IMAGES["noise 64x64"], c) == _want("noise 64x64", c)[0]
    assert _device_file(ctx, rr, IMAGES["one colour 3x4"], c) == _want("one colour 3x4", c)[0]
    assert _device_file(ctx, rr, IMAGES["noise 64x64"], c) == _want("noise 64x64", c)[0]


def test_quality_is_flagged_not_honoured(ctx, rr, tmp_path):
    img = IMAGES["across steps"]
    q100 = _device_file(ctx, rr, img, 4, quality=100)
    assert ctx.last_warning() == ""
    q90 = _device_file(ctx, rr, img, 4, quality=90)
    assert q90 == q100
    w = ctx.last_warning()
    assert "WEBP" in w and "90" in w and "lossy WEBP is not built" in w
    # a rendered frame: written, flagged, the same bytes
    p = rr.default_params(spp=2, width=96, height=54)
    s = ctx.load_scene(S04)
    try:
        ctx.render_frame(s, 3, p, str(tmp_path / "a"), "WEBP", 100)
        assert ctx.last_warning() == ""
        ctx.render_frame(s, 3, p, str(tmp_path / "b"), "WEBP", 75)
        assert "75" in ctx.last_warning() and "lossy WEBP is not built" in ctx.last_warning()
        assert (tmp_path / "a.webp").read_bytes() == (tmp_path / "b.webp").read_bytes()
        ctx.render_frame(s, 3, p, str(tmp_path / "c"), "TARGA", 75)
        assert ctx.last_warning() == ""
    finally:
        s.close()


def _render_file(ctx, s, frame, p, tmp_path, name, fmt):
    ctx.render_frame(s, frame, p, str(tmp_path / name), fmt, 100)
    return (tmp_path / (name + rr_ext(fmt))).read_bytes()


def rr_ext(fmt):
    return {"WEBP": ".webp", "TARGA": ".tga", "TARGA_RAW": ".tga", "PNG": ".png"}[fmt]


@pytest.mark.parametrize("dither", [0.0, 1.0])
@pytest.mark.parametrize("mode", [0, "BW", "RGB"])
def test_rendered_frames(ctx, rr, tmp_path, mode, dither):
    c = {0: 4, "BW": 1, "RGB": 3}[mode]
    w, h = 250, 141
    p = rr.default_params(spp=4, width=w, height=h)
    s = ctx.load_scene(S04)
    ctx.set_dither(dither)
    ctx.set_color_mode(mode)
    ctx.set_png_depth(16)  # a WEBP file is 8 bits a channel whatever the depth
    try:
        data = _render_file(ctx, s, 3, p, tmp_path, "a", "WEBP")
        raw = _render_file(ctx, s, 3, p, tmp_path, "a", "TARGA_RAW")
        px = _pil(data, w, h, c)
        assert len(np.unique(px)) > 16
        tga = np.asarray(Image.open(io.BytesIO(raw)))
        if c == 1:
            assert tga.shape == (h, w)
            tga = np.repeat(tga[..., None], 3, axis=2)  # BW: the grey code in R, G and B
        _same(px, tga, "WEBP against TARGA_RAW")
        if c == 4:
            assert np.all(px[..., 3] == 255)
        # and the file is the restatement's of the frame's 8-bit image
        rgba8 = ctx.render_to_memory(s, 3, p)[1]
        assert data == W.encode(rgba8, c)
    finally:
        ctx.set_dither(0.0)
        ctx.set_color_mode(0)
        ctx.set_png_depth(0)
        s.close()


def test_frames_in_flight_and_beside_png(ctx, rr, tmp_path):
    p = rr.default_params(spp=4, width=160, height=90)
    s = ctx.load_scene(S04)
    ctx.set_device_png(True)
    try:
        solo = {f: _render_file(ctx, s, f, p, tmp_path, f"solo{f}", "WEBP") for f in (3, 4, 5)}
        assert len(set(solo.values())) == 3
        png4 = _render_file(ctx, s, 4, p, tmp_path, "solo4", "PNG")
        # three frames in flight
        tickets = [ctx.submit_frame(s, f, p, str(tmp_path / f"fl{f}"), "WEBP", 100) for f in (3, 4, 5)]
        for t in tickets:
            ctx.complete_frame(t)
        for f in (3, 4, 5):
            assert (tmp_path / f"fl{f}.webp").read_bytes() == solo[f], f
        # three WEBP frames around a device PNG frame, in flight together
        order = ((3, "WEBP"), (4, "PNG"), (4, "WEBP"), (5, "WEBP"))
        tickets = []
        for i, (f, fmt) in enumerate(order[:3]):
            tickets.append(ctx.submit_frame(s, f, p, str(tmp_path / f"mix{i}"), fmt, 100))
        ctx.complete_frame(tickets[0])
        tickets.append(ctx.submit_frame(s, 5, p, str(tmp_path / "mix3"), "WEBP", 100))
        for t in tickets[1:]:
            ctx.complete_frame(t)
        for i, (f, fmt) in enumerate(order):
            want = solo[f] if fmt == "WEBP" else png4
            assert (tmp_path / f"mix{i}{rr_ext(fmt)}").read_bytes() == want, (i, f, fmt)
        # and one after the other, beside TARGA frames of the same slot buffers
        for k, (f, fmt) in enumerate(((4, "PNG"), (3, "WEBP"), (3, "TARGA"), (5, "WEBP"))):
            ctx.render_frame(s, f, p, str(tmp_path / f"seq{k}"), fmt, 100)
        assert (tmp_path / "seq0.png").read_bytes() == png4
        assert (tmp_path / "seq1.webp").read_bytes() == solo[3] and (tmp_path / "seq3.webp").read_bytes() == solo[5]
    finally:
        ctx.set_device_png(False)
        s.close()


def test_coder_time_is_reported(ctx, rr, tmp_path):
    p = rr.default_params(spp=2, width=160, height=90, flags=rr.native.RR_FLAG_PROFILE_KERNELS)
    s = ctx.load_scene(S04)
    try:
        _, st = ctx.render_frame(s, 3, p, str(tmp_path / "t"), "WEBP", 100)
        assert st.kernel_launches[rr.native.RR_K_PNG] == 1 and st.kernel_ms[rr.native.RR_K_PNG] > 0.0
        assert st.output_bytes == (tmp_path / "t.webp").stat().st_size
    finally:
        s.close()


def test_shim_writes_webp(rr, tmp_path):
    out_fmt = str(tmp_path / "######")
    env = dict(os.environ, RR_WIDTH="64", RR_HEIGHT="36", RR_SPP="2")
    argv = [rr.SHIM_PATH, S04.replace(".rrscene", ".blend"), "--background", "--python", "script.py", "--",
            "--render-output", out_fmt, "--render-format", "WEBP", "--render-frame", "12"]
    res = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"Saved: '{tmp_path}/000012.webp'" in res.stdout
    px, info = W.read((tmp_path / "000012.webp").read_bytes())
    assert px.shape == (36, 64, 4) and info["alpha"] == 1 and len(np.unique(px[..., :3])) > 4
    _same(_pil((tmp_path / "000012.webp").read_bytes(), 64, 36, 4), px, "PIL against the strict reader")


def test_sizes_outside_the_format_are_refused(ctx, rr, tmp_path):
    """RR_EINVAL before any launch: the image is not read (it is one pixel)."""
    tiny = np.zeros((1, 1, 4), np.uint8)
    n = ctypes.c_uint64()
    L = rr.lib()
    ptr = tiny.ctypes.data_as(ctypes.c_void_p)
    for mode in (0, 1, 3, 4):
        for w, h in ((16385, 1), (1, 16385), (16385, 16385), (65536, 2)):
            rc = L.rr_debug_encode_device(ctx.handle, b"WEBP", 8, mode, ptr, 0, w, h, 0, ctypes.c_float(1.0), 100, None,
                                          0, ctypes.byref(n))
            assert rc == rr.native.RR_EINVAL, (mode, w, h)
    # 8 bits a channel and no other depth; no float image
    for depth, isf in ((16, 0), (32, 0), (8, 1), (0, 1)):
        rc = L.rr_debug_encode_device(ctx.handle, b"WEBP", depth, 4, ptr, isf, 1, 1, 0, ctypes.c_float(1.0), 100, None,
                                      0, ctypes.byref(n))
        assert rc == rr.native.RR_EINVAL, (depth, isf)
    # a frame of such a size is refused when it is submitted, and the context goes on
    s = ctx.load_scene(S04)
    try:
        with pytest.raises(rr.RRError) as e:
            ctx.submit_frame(s, 3, rr.default_params(spp=1, width=16385, height=1), str(tmp_path / "big"), "WEBP", 100)
        assert e.value.code == rr.native.RR_EINVAL and "WEBP" in str(e.value)
        assert not (tmp_path / "big.webp").exists()
        assert _device_file(ctx, rr, tiny, 4) == W.encode(tiny, 4)
    finally:
        s.close()
