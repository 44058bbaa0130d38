"""HDR on the device (hdr.hip): the coder's bytes equal the restatement of
tests/hdr.py and the host coder's at every shape where it can go wrong;
rendered frames hold the quads of the FLOAT OPEN_EXR file's values, in RGB and
BW, whatever the view settings; frames in flight and frames beside JPEG and PNG
frames write their solo files; the shim; refusals before any launch."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import color_modes as M
import exr32_reader as X
import hdr as H
from conftest import PKG, ROOT, scene_path

pytestmark = pytest.mark.gpu

F32 = np.float32
S04 = scene_path("04_very-simple-standin.rrscene")
MODES = {"BW": 1, "RGB": 3, "RGBA": 3}
CHUNK = 256  # bytes a workgroup of k_hdr_size takes of its plane per step (hdr.hpp kHdrChunk)
IMAGES = {**H.images(), **H.device_images(CHUNK)}
WANT = {}  # (name, c) -> the restatement's file, computed once


def _want(name, c):
    if (name, c) not in WANT:
        WANT[(name, c)] = H.encode(IMAGES[name], c)
    return WANT[(name, c)]


def test_chunk_is_the_kernels(rr):
    with open(os.path.join(ROOT, PKG, "csrc", "hdr.hpp")) as f:
        assert f"constexpr int kHdrChunk = {CHUNK};" in f.read()


@pytest.mark.parametrize("mode", ["BW", "RGB", "RGBA"])
def test_device_equals_restatement_and_host(ctx, rr, mode):
    c = MODES[mode]
    for name, img in IMAGES.items():
        dev = ctx.encode_device("HDR", img, 0, mode)
        assert dev == _want(name, c), (name, len(dev), len(_want(name, c)), "device file differs from the restatement")
        assert dev == rr.hdr_host(img, mode), (name, "device file differs from the host coder's")
        H.read(dev)
    img = IMAGES["across steps"]
    assert ctx.encode_device("HDR", img, 32, mode) == _want("across steps", c)  # depth 32 is depth 0
    if mode == "RGB":
        assert ctx.encode_device("HDR", img, 0, 0) == _want("across steps", 3)  # no mode: RGB


@pytest.mark.parametrize("w", [32767, 32768])
def test_widest_coded_and_first_flat_row(ctx, rr, w):
    img = H.shape_image(w, 2, seed=w)
    dev = ctx.encode_device("HDR", img, 0, "RGB")
    assert dev == H.encode(img, 3)
    assert dev == rr.hdr_host(img, "RGB")
    assert H.read(dev)[1]["flat"] == (w == 32768)


def test_special_values_and_twice(ctx, rr):
    img = H.special_row()
    for mode in ("RGB", "BW"):
        dev = ctx.encode_device("HDR", img, 0, mode)
        assert dev == rr.hdr_host(img, mode), mode
        assert dev == H.encode(img, MODES[mode]), mode
        assert ctx.encode_device("HDR", img[:, :7], 0, mode) == rr.hdr_host(img[:, :7], mode)  # a flat row
    # random float bits: every branch of the rule beside every other
    bits = np.random.default_rng(4).integers(0, 1 << 32, (3, 1000, 4), dtype=np.uint64).astype(np.uint32)
    rnd = bits.view(F32)
    first = ctx.encode_device("HDR", rnd, 0, "RGB")
    assert first == rr.hdr_host(rnd, "RGB")
    with np.errstate(all="ignore"):
        assert ctx.encode_device("HDR", rnd, 0, "BW") == rr.hdr_host(rnd, "BW") == H.encode(rnd, 1)
    # the same image twice: the same bytes
    a = ctx.encode_device("HDR", IMAGES["across steps"], 0, "RGB")
    assert ctx.encode_device("HDR", rnd, 0, "RGB") == first
    assert ctx.encode_device("HDR", IMAGES["across steps"], 0, "RGB") == a


def _render(ctx, s, frame, p, tmp_path, name, fmt, ext):
    ctx.render_frame(s, frame, p, str(tmp_path / name), fmt, 90)
    return (tmp_path / (name + ext)).read_bytes()


def test_rendered_frame_holds_the_exr_values(ctx, rr, tmp_path):
    p = rr.default_params(spp=4, width=250, height=141)
    s = ctx.load_scene(S04)
    ctx.set_exr_depth(32)
    try:
        hdr = _render(ctx, s, 3, p, tmp_path, "a", "HDR", ".hdr")
        px = X.read_exr32(_render(ctx, s, 3, p, tmp_path, "a", "OPEN_EXR", ".exr"))[0]  # (H, W, 4) bits, R G B A
        means = np.ascontiguousarray(px).view(F32)
        assert means.shape == (141, 250, 4) and len(np.unique(means[..., :3])) > 1000
        assert hdr == H.encode(means, 3)
        q, info = H.read(hdr)
        assert not info["flat"] and q.shape == (141, 250, 4) and len(np.unique(q[..., 3])) > 1
        # BW: the quads of the EXR's Y in all three channels
        ctx.set_color_mode("BW")
        hdr_bw = _render(ctx, s, 3, p, tmp_path, "b", "HDR", ".hdr")
        words, einfo = M.read_exr(_render(ctx, s, 3, p, tmp_path, "b", "OPEN_EXR", ".exr"))
        assert words.shape == (141, 250, 1) and words.dtype == np.uint32
        y = np.ascontiguousarray(words[..., 0]).view(F32)
        assert hdr_bw == H.encode(np.stack([y, y, y], axis=-1), 3)
        assert hdr_bw == H.encode(means, 1)  # which is the luma of the RGB file's means
        qb = H.read(hdr_bw)[0]
        assert np.array_equal(qb[..., 0], qb[..., 1]) and np.array_equal(qb[..., 0], qb[..., 2])
        ctx.set_color_mode("RGBA")  # no alpha: RGB
        assert _render(ctx, s, 3, p, tmp_path, "c", "HDR", ".hdr") == hdr
        # scene-linear: view settings, depths and dither do not reach the file
        ctx.set_color_mode(0)
        ctx.set_look("High Contrast")
        ctx.set_display_gamma(2.2)
        ctx.set_dither(1.0)
        ctx.set_png_depth(16)
        ctx.set_exr_depth(16)
        assert _render(ctx, s, 3, p, tmp_path, "d", "HDR", ".hdr") == hdr
    finally:
        ctx.set_color_mode(0)
        ctx.set_look(None)
        ctx.set_display_gamma(0.0)
        ctx.set_dither(0.0)
        ctx.set_png_depth(0)
        ctx.set_exr_depth(0)
        s.close()


def test_frames_in_flight_and_beside_jpeg_and_png(ctx, rr, tmp_path):
    p = rr.default_params(spp=4, width=160, height=90)
    s = ctx.load_scene(S04)
    ctx.set_device_png(True)
    try:
        solo = {f: _render(ctx, s, f, p, tmp_path, f"solo{f}", "HDR", ".hdr") for f in (3, 4, 5)}
        assert len(set(solo.values())) == 3
        png4 = _render(ctx, s, 4, p, tmp_path, "solo4", "PNG", ".png")
        jpg3 = _render(ctx, s, 3, p, tmp_path, "solo3", "JPEG", ".jpg")
        tickets = [ctx.submit_frame(s, f, p, str(tmp_path / f"fl{f}"), "HDR", 90) for f in (3, 4, 5)]
        for t in tickets:
            ctx.complete_frame(t)
        for f in (3, 4, 5):
            assert (tmp_path / f"fl{f}.hdr").read_bytes() == solo[f], f
        for k, order in enumerate((((3, "JPEG"), (4, "HDR"), (4, "PNG")), ((5, "HDR"), (3, "JPEG"), (3, "HDR")),
                                   ((4, "PNG"), (5, "HDR"), (4, "HDR")))):
            tickets = [ctx.submit_frame(s, f, p, str(tmp_path / f"mix{k}_{i}"), fmt, 90)
                       for i, (f, fmt) in enumerate(order)]
            for t in tickets:
                ctx.complete_frame(t)
            for i, (f, fmt) in enumerate(order):
                ext = {"HDR": ".hdr", "PNG": ".png", "JPEG": ".jpg"}[fmt]
                want = solo[f] if fmt == "HDR" else png4 if fmt == "PNG" else jpg3
                assert (tmp_path / f"mix{k}_{i}{ext}").read_bytes() == want, (k, i, f, fmt)
    finally:
        ctx.set_device_png(False)
        s.close()


def test_coder_time_is_reported(ctx, rr, tmp_path):
    p = rr.default_params(spp=2, width=160, height=90, flags=rr.native.RR_FLAG_PROFILE_KERNELS)
    s = ctx.load_scene(S04)
    try:
        _, st = ctx.render_frame(s, 3, p, str(tmp_path / "t"), "HDR", 90)
        assert st.kernel_launches[rr.native.RR_K_PNG] == 1 and st.kernel_ms[rr.native.RR_K_PNG] > 0.0
        assert st.output_bytes == (tmp_path / "t.hdr").stat().st_size
    finally:
        s.close()


def test_shim_writes_hdr(rr, tmp_path):
    out_fmt = str(tmp_path / "######")
    env = dict(os.environ, RR_WIDTH="64", RR_HEIGHT="36", RR_SPP="2")
    argv = [rr.SHIM_PATH, S04.replace(".rrscene", ".blend"), "--background", "--python", "script.py", "--",
            "--render-output", out_fmt, "--render-format", "HDR", "--render-frame", "12"]
    res = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"Saved: '{tmp_path}/000012.hdr'" in res.stdout
    q, info = H.read((tmp_path / "000012.hdr").read_bytes())
    assert q.shape == (36, 64, 4) and not info["flat"] and q[..., 3].max() > 0


def test_refusals_before_any_launch(ctx, rr):
    """RR_EINVAL before any launch: the image is not read (it is one pixel)."""
    tiny = np.zeros((1, 1, 4), F32)
    n = ctypes.c_uint64()
    L = rr.lib()
    ptr = tiny.ctypes.data_as(ctypes.c_void_p)

    def call(depth, mode, is_float, w, h):
        return L.rr_debug_encode_device(ctx.handle, b"HDR", depth, mode, ptr, is_float, w, h, 0, ctypes.c_float(1.0), 90,
                                        None, 0, ctypes.byref(n))

    for depth, isf in ((0, 0), (32, 0), (8, 0), (8, 1), (16, 1)):  # a uint8 image; depths 8 and 16
        assert call(depth, 3, isf, 1, 1) == rr.native.RR_EINVAL, (depth, isf)
    for mode in (0, 1, 3, 4):
        for w, h in ((32768, 16384), (32767, 16400), (1 << 29, 1), (1, 1 << 29)):  # a body bound of 2 GB and more
            assert call(0, mode, 1, w, h) == rr.native.RR_EINVAL, (mode, w, h)
    assert call(0, 3, 1, 1, 1) == 0 and n.value == len(H.header(1, 1)) + 4
    with pytest.raises(rr.RRError) as e:
        ctx.encode_device("HDR", np.zeros((2, 2, 4), np.uint8))
    assert e.value.code == rr.native.RR_EINVAL
    with pytest.raises(rr.RRError) as e:
        ctx.encode_device("HDR", np.zeros((2, 2, 4), F32), 16)
    assert e.value.code == rr.native.RR_EINVAL
