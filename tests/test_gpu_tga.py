"""TARGA and TARGA_RAW on the device (tga.hip): the packer's bytes equal the
host coder's and the restatement of tests/tga.py at every shape where it can go
wrong; rendered frames decode to the 8-bit image, with BW and with dither;
frames in flight and frames beside PNG frames write their solo files; the shim;
sizes outside the format are refused before any launch."""
import ctypes
import io
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

import tga as T
from conftest import scene_path

pytestmark = pytest.mark.gpu

S04 = scene_path("04_very-simple-standin.rrscene")
MODES = {"BW": 1, "RGB": 3, "RGBA": 4}
CHUNK = 256  # pixels a workgroup of k_tga_size takes of its row per step (tga.hpp kTgaChunk)
IMAGES = {**T.images(), **T.device_images(CHUNK)}


def _device_file(ctx, rr, fmt, img, c):
    """One rr_debug_encode_device call into a buffer above the all-literal bound."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    out = np.zeros(T.HEADER + h * T.row_bound(w, c) + 64, np.uint8)
    n = ctypes.c_uint64()
    rc = rr.lib().rr_debug_encode_device(ctx.handle, fmt.encode(), 8, c, img.ctypes.data_as(ctypes.c_void_p), 0, w, h,
                                         0, ctypes.c_float(1.0), 90, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                         out.size, ctypes.byref(n))
    assert rc == 0, rr.lib().rr_last_error(ctx.handle)
    assert n.value <= out.size - 64, "a file above the all-literal bound"
    return out[:n.value].tobytes()


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} samples differ, first at {bad[0]}"


def test_chunk_is_the_kernels(rr):
    from conftest import ROOT, PKG
    with open(os.path.join(ROOT, PKG, "csrc", "tga.hpp")) as f:
        assert f"constexpr int kTgaChunk = {CHUNK};" in f.read()


@pytest.mark.parametrize("fmt", ["TARGA", "TARGA_RAW"])
@pytest.mark.parametrize("mode", ["BW", "RGB", "RGBA"])
def test_device_equals_host_and_restatement(ctx, rr, tmp_path, mode, fmt):
    c, rle = MODES[mode], fmt == "TARGA"
    for name, img in IMAGES.items():
        dev = _device_file(ctx, rr, fmt, img, c)
        want = T.encode(img, c, rle)
        assert dev == want, (name, len(dev), len(want), "device file differs from the restatement")
        rr.encode_image_mode(img, str(tmp_path / "h"), fmt, 90, mode)
        assert dev == (tmp_path / "h.tga").read_bytes(), (name, "device file differs from the host coder's")
    # encode_device (two calls: the length, then the bytes) gives the same file, and depth 0 is 8
    img = IMAGES["across chunks"]
    assert ctx.encode_device(fmt, img, 0, mode) == T.encode(img, c, rle)


def _render_file(ctx, s, frame, p, tmp_path, name, fmt):
    ctx.render_frame(s, frame, p, str(tmp_path / name), fmt, 90)
    return (tmp_path / (name + ".tga")).read_bytes()


@pytest.mark.parametrize("dither", [0.0, 1.0])
@pytest.mark.parametrize("mode", [0, "BW", "RGB"])
def test_rendered_frames(ctx, rr, tmp_path, mode, dither):
    c = {0: 4, "BW": 1, "RGB": 3}[mode]
    p = rr.default_params(spp=4, width=250, height=141)
    s = ctx.load_scene(S04)
    ctx.set_dither(dither)
    ctx.set_color_mode(mode)
    ctx.set_png_depth(16)  # a TARGA file is 8 bits a channel whatever the depth
    try:
        rgba8 = ctx.render_to_memory(s, 3, p)[1]
        assert len(np.unique(rgba8[..., :3])) > 16 and np.all(rgba8[..., 3] == 255)
        want = T.expected(rgba8, c)
        for fmt in ("TARGA", "TARGA_RAW"):
            data = _render_file(ctx, s, 3, p, tmp_path, "a" + fmt, fmt)
            assert data == T.encode(rgba8, c, fmt == "TARGA"), fmt
            px, info = T.read(data)
            assert info["channels"] == c and info["rle"] == (fmt == "TARGA")
            _same(px, want, fmt)
            im = Image.open(io.BytesIO(data))
            assert im.mode == T.PIL_MODE[c] and im.size == (250, 141)
            _same(np.asarray(im).reshape(141, 250, c), want, ("PIL", fmt))
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
        plain = _render_file(ctx, s, 3, p, tmp_path, "p", "TARGA_RAW")
        ctx.set_dither(2.0)
        assert _render_file(ctx, s, 3, p, tmp_path, "d", "TARGA_RAW") != plain
    finally:
        ctx.set_dither(0.0)
        s.close()


def test_frames_in_flight_and_beside_png(ctx, rr, tmp_path):
    p = rr.default_params(spp=4, width=160, height=90)
    s = ctx.load_scene(S04)
    ctx.set_device_png(True)
    try:
        solo = {f: _render_file(ctx, s, f, p, tmp_path, f"solo{f}", "TARGA") for f in (3, 4, 5)}
        assert len(set(solo.values())) == 3
        ctx.render_frame(s, 4, p, str(tmp_path / "solo4"), "PNG", 90)
        png4 = (tmp_path / "solo4.png").read_bytes()
        # three frames in flight
        tickets = [ctx.submit_frame(s, f, p, str(tmp_path / f"fl{f}"), "TARGA", 90) for f in (3, 4, 5)]
        for t in tickets:
            ctx.complete_frame(t)
        for f in (3, 4, 5):
            assert (tmp_path / f"fl{f}.tga").read_bytes() == solo[f], f
        # a TARGA frame before and after a device PNG frame, in flight together, then one after the other
        tickets = [ctx.submit_frame(s, f, p, str(tmp_path / f"mix{f}"), fmt, 90)
                   for f, fmt in ((3, "TARGA"), (4, "PNG"), (5, "TARGA"))]
        for t in tickets:
            ctx.complete_frame(t)
        assert (tmp_path / "mix3.tga").read_bytes() == solo[3]
        assert (tmp_path / "mix4.png").read_bytes() == png4
        assert (tmp_path / "mix5.tga").read_bytes() == solo[5]
        for k, (f, fmt) in enumerate(((4, "PNG"), (3, "TARGA"), (4, "PNG"), (5, "TARGA_RAW"), (5, "TARGA"))):
            ctx.render_frame(s, f, p, str(tmp_path / f"seq{k}"), fmt, 90)
        assert (tmp_path / "seq0.png").read_bytes() == png4 and (tmp_path / "seq2.png").read_bytes() == png4
        assert (tmp_path / "seq1.tga").read_bytes() == solo[3] and (tmp_path / "seq4.tga").read_bytes() == solo[5]
        _same(T.read((tmp_path / "seq3.tga").read_bytes())[0], T.read(solo[5])[0], "raw after PNG")
    finally:
        ctx.set_device_png(False)
        s.close()


def test_coder_time_is_reported(ctx, rr, tmp_path):
    p = rr.default_params(spp=2, width=160, height=90, flags=rr.native.RR_FLAG_PROFILE_KERNELS)
    s = ctx.load_scene(S04)
    try:
        _, st = ctx.render_frame(s, 3, p, str(tmp_path / "t"), "TARGA", 90)
        assert st.kernel_launches[rr.native.RR_K_PNG] == 1 and st.kernel_ms[rr.native.RR_K_PNG] > 0.0
        assert st.output_bytes == (tmp_path / "t.tga").stat().st_size
    finally:
        s.close()


def test_shim_writes_tga(rr, tmp_path):
    out_fmt = str(tmp_path / "######")
    env = dict(os.environ, RR_WIDTH="64", RR_HEIGHT="36", RR_SPP="2")
    for fmt in ("TARGA", "TARGA_RAW"):
        argv = [rr.SHIM_PATH, S04.replace(".rrscene", ".blend"), "--background", "--python", "script.py", "--",
                "--render-output", out_fmt, "--render-format", fmt, "--render-frame", "12"]
        res = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        assert f"Saved: '{tmp_path}/000012.tga'" in res.stdout
        px, info = T.read((tmp_path / "000012.tga").read_bytes())
        assert px.shape == (36, 64, 4) and info["rle"] == (fmt == "TARGA")
    bad = subprocess.run(argv[:-3] + ["TIFF", "--render-frame", "12"], capture_output=True, text=True, env=env,
                         timeout=60)
    assert bad.returncode == 1 and "unsupported output format 'TIFF'" in bad.stdout


def test_sizes_outside_the_format_are_refused(ctx, rr):
    """RR_EINVAL before any launch: the image is not read (it is one pixel)."""
    tiny = np.zeros((1, 1, 4), np.uint8)
    n = ctypes.c_uint64()
    L = rr.lib()
    for fmt in (b"TARGA", b"TARGA_RAW"):
        for mode in (0, 1, 3, 4):
            for w, h in ((65536, 1), (1, 65536), (65535, 65535)):
                rc = L.rr_debug_encode_device(ctx.handle, fmt, 8, mode, tiny.ctypes.data_as(ctypes.c_void_p), 0, w, h, 0,
                                              ctypes.c_float(1.0), 90, None, 0, ctypes.byref(n))
                assert rc == rr.native.RR_EINVAL, (fmt, mode, w, h)
        # 8 bits a channel and no other depth; no float image
        for depth, isf in ((16, 0), (32, 0), (8, 1), (0, 1)):
            rc = L.rr_debug_encode_device(ctx.handle, fmt, depth, 4, tiny.ctypes.data_as(ctypes.c_void_p), isf, 1, 1, 0,
                                          ctypes.c_float(1.0), 90, None, 0, ctypes.byref(n))
            assert rc == rr.native.RR_EINVAL, (fmt, depth, isf)
