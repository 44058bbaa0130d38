"""The render region (rr_set_region): a region's pixels are, bit for bit, the pixels the same
frame has when rendered whole by the same build, on the tile path and on the split path.

The yardstick is the full frame: each pixel's samples are keyed on the pixel's full-frame
coordinates, so nothing the region code computes enters the comparison, and the tolerance is 0.
The film comes from FLOAT OPEN_EXR files, which hold the means sum * inv_spp bit for bit.
Scene: the 04_very-simple stand-in at 70 x 45 (neither side a multiple of the 8 x 8 tile),
4 samples, frame 3; each path renders it whole once."""
import json
import os
import subprocess

import numpy as np
import pytest

import exr32_reader as X32
import png16_reader as P16
import reduce as R
import tga as T
from conftest import scene_path

pytestmark = pytest.mark.gpu

S04 = scene_path("04_very-simple-standin.rrscene")
W, H, SPP, FRAME = 70, 45, 4, 3
REGIONS = {
    "aligned": (8, 8, 24, 16),
    "unaligned": (3, 5, 61, 44),
    "pixel": (13, 7, 14, 8),
    "row": (0, 44, 70, 45),
    "column": (69, 0, 70, 45),
    "ragged-corner": (60, 40, 70, 45),
    "whole": (0, 0, 70, 45),
}
UNALIGNED = REGIONS["unaligned"]
# 41 samples: 41 * (1 / 41) is not 1 in float32, so an alpha made by rescaling a sample count would show;
# the tile path then also runs sliced (two sample groups) and folds
PATHS = ("tiles", "split", "split-2-chunks", "tiles-41", "split-41")
EXT = {"JPEG": ".jpg", "PNG": ".png", "OPEN_EXR": ".exr", "TARGA_RAW": ".tga", "WEBP": ".webp"}


@pytest.fixture(scope="module")
def mctx(rr):
    c = rr.RenderContext(0)
    yield c
    c.close()


@pytest.fixture
def rctx(mctx):
    yield mctx
    mctx.set_region(None, from_scene=False)
    mctx.set_device_png(False)
    mctx.set_exr_depth(0)
    mctx.set_png_depth(0)
    mctx.set_color_mode(0)


@pytest.fixture(scope="module")
def s04(mctx):
    s = mctx.load_scene(S04)
    yield s
    s.close()


def _params(rr, path="tiles"):
    if path == "tiles":
        return rr.default_params(width=W, height=H, spp=SPP)
    if path == "tiles-41":
        return rr.default_params(width=W, height=H, spp=41)
    if path == "split-41":
        return rr.default_params(width=W, height=H, spp=41, flags=rr.native.RR_FLAG_WAVEFRONT)
    if path == "split":
        return rr.default_params(width=W, height=H, spp=SPP, flags=rr.native.RR_FLAG_WAVEFRONT)
    return rr.default_params(width=W, height=H, spp=8, spp_per_chunk=4, flags=rr.native.RR_FLAG_WAVEFRONT)


def _file(base, fmt):
    with open(str(base) + EXT[fmt], "rb") as f:
        return f.read()


def _render(ctx, scene, p, d, name, fmt, quality=90):
    ctx.render_frame(scene, FRAME, p, str(d / name), fmt, quality)
    return _file(d / name, fmt)


def _words(exr):
    return X32.read_exr32(exr)[0]  # (H, W, 4) uint32: R, G, B, A bit patterns


@pytest.fixture(scope="module")
def full(mctx, rr, s04, tmp_path_factory):
    """Per path, the words of the whole frame's FLOAT OPEN_EXR file, rendered once."""
    d = tmp_path_factory.mktemp("full")
    mctx.set_region(None, from_scene=False)
    mctx.set_exr_depth(32)
    out = {}
    for path in PATHS:
        out[path] = _words(_render(mctx, s04, _params(rr, path), d, path, "OPEN_EXR"))
        assert out[path].shape == (H, W, 4)
        assert np.all(out[path][..., 3] == 0x3F800000)  # a rendered frame's A is 1.0
    mctx.set_exr_depth(0)
    # both paths compute the same frame (the existing parity tests pin it to the oracle)
    assert np.array_equal(out["tiles"], out["split"]) and np.array_equal(out["tiles-41"], out["split-41"])
    return out


# ------------------------------------------------------ 1: bit-exact window ---
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(REGIONS))
def test_cropped_region_is_the_full_frames_window(rctx, rr, s04, full, tmp_path, name, path):
    x0, y0, x1, y1 = REGIONS[name]
    rctx.set_exr_depth(32)
    rctx.set_region(REGIONS[name], crop=True)
    got = _words(_render(rctx, s04, _params(rr, path), tmp_path, "c", "OPEN_EXR"))
    assert got.shape == (y1 - y0, x1 - x0, 4)
    assert np.array_equal(got, full[path][y0:y1, x0:x1])


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(REGIONS))
def test_uncropped_region_is_the_full_frame_inside_and_zero_outside(rctx, rr, s04, full, tmp_path, name, path):
    x0, y0, x1, y1 = REGIONS[name]
    rctx.set_exr_depth(32)
    rctx.set_region(REGIONS[name], crop=False)
    got = _words(_render(rctx, s04, _params(rr, path), tmp_path, "u", "OPEN_EXR"))
    want = np.zeros_like(full[path])
    want[y0:y1, x0:x1] = full[path][y0:y1, x0:x1]  # A = 1.0 inside, every channel 0 outside
    assert got.shape == (H, W, 4)
    assert np.array_equal(got, want)


# ----------------------------------------------------------------- 2: union ---
@pytest.mark.parametrize("path", ("tiles", "split", "tiles-41", "split-41"))
def test_two_halves_add_up_to_the_full_frame(rctx, rr, s04, full, tmp_path, path):
    rctx.set_exr_depth(32)
    halves = []
    for i, region in enumerate(((0, 0, 35, 45), (35, 0, 70, 45))):
        rctx.set_region(region, crop=False)
        halves.append(_words(_render(rctx, s04, _params(rr, path), tmp_path, f"h{i}", "OPEN_EXR")).view(np.float32))
    assert np.array_equal((halves[0] + halves[1]).view(np.uint32), full[path])


# ---------------------------------------------------------- 3: other coders ---
def _decode(fmt, data):
    if fmt == "TARGA_RAW":
        return T.read(data)[0]
    if fmt == "PNG16":
        return P16.read_png16(data)[0]
    from PIL import Image
    import io
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))


@pytest.mark.parametrize("fmt", ("TARGA_RAW", "PNG", "PNG16"))
def test_cropped_files_decode_to_the_window_of_the_full_frames_file(rctx, rr, s04, tmp_path, fmt):
    x0, y0, x1, y1 = UNALIGNED
    rctx.set_device_png(True)
    rctx.set_png_depth(16 if fmt == "PNG16" else 8)
    name = "PNG" if fmt == "PNG16" else fmt
    p = _params(rr)
    whole = _decode(fmt, _render(rctx, s04, p, tmp_path, "whole", name))
    rctx.set_region(UNALIGNED, crop=True)
    part = _decode(fmt, _render(rctx, s04, p, tmp_path, "part", name))
    assert whole.shape[:2] == (H, W) and part.shape[:2] == (y1 - y0, x1 - x0)
    assert np.array_equal(part, whole[y0:y1, x0:x1])


def test_cropped_jpeg_is_the_coders_file_of_the_cropped_image(rctx, rr, s04, tmp_path):
    x0, y0, x1, y1 = UNALIGNED
    p = _params(rr)
    _, whole8, _ = rctx.render_to_memory(s04, FRAME, p)
    rctx.set_region(UNALIGNED, crop=True)
    film, part8, st = rctx.render_to_memory(s04, FRAME, p)
    assert part8.shape == (y1 - y0, x1 - x0, 4) and film.shape == part8.shape
    assert np.array_equal(part8, whole8[y0:y1, x0:x1])
    assert (st.width, st.height) == (W, H)
    data = _render(rctx, s04, p, tmp_path, "j", "JPEG", 85)
    assert data == rctx.encode_device("JPEG", part8, quality=85)


def test_uncropped_rgba_targa_has_alpha_only_inside(rctx, rr, s04, tmp_path):
    x0, y0, x1, y1 = UNALIGNED
    p = _params(rr)
    rctx.set_color_mode("RGBA")
    whole = T.read(_render(rctx, s04, p, tmp_path, "w", "TARGA_RAW"))[0]
    rctx.set_region(UNALIGNED, crop=False)
    got = T.read(_render(rctx, s04, p, tmp_path, "u", "TARGA_RAW"))[0]
    want = np.zeros_like(whole)
    want[y0:y1, x0:x1] = whole[y0:y1, x0:x1]
    assert got.shape == (H, W, 4) and np.all(whole[..., 3] == 255)
    assert np.array_equal(got, want)  # alpha 255 inside, 0 outside; RGB 0 outside


def test_uncropped_16_bit_png_is_transparent_black_outside(rctx, rr, s04, tmp_path):
    x0, y0, x1, y1 = UNALIGNED
    rctx.set_png_depth(16)
    p = rr.default_params(width=W, height=H, spp=41)
    whole = P16.read_png16(_render(rctx, s04, p, tmp_path, "w", "PNG"))[0]
    rctx.set_region(UNALIGNED, crop=False)
    got = P16.read_png16(_render(rctx, s04, p, tmp_path, "u", "PNG"))[0]
    want = np.zeros_like(whole)
    want[y0:y1, x0:x1] = whole[y0:y1, x0:x1]
    assert got.shape == (H, W, 4) and np.all(whole[..., 3] == 65535)
    assert np.array_equal(got, want)  # A 65535 inside, (0, 0, 0, 0) outside


def test_uncropped_film_in_memory_has_alpha_only_inside(rctx, rr, s04):
    x0, y0, x1, y1 = UNALIGNED
    p = rr.default_params(width=W, height=H, spp=41)
    whole, _, _ = rctx.render_to_memory(s04, FRAME, p)
    rctx.set_region(UNALIGNED, crop=False)
    film, _, _ = rctx.render_to_memory(s04, FRAME, p)
    want = np.zeros_like(whole)
    want[y0:y1, x0:x1] = whole[y0:y1, x0:x1]
    assert np.all(whole[..., 3] == 1.0) and np.array_equal(film.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------- 4: whole-frame region ---
@pytest.mark.parametrize("crop", (False, True))
def test_a_region_of_the_whole_frame_writes_the_no_region_bytes(rctx, rr, s04, tmp_path, crop):
    rctx.set_device_png(True)
    p = _params(rr)
    fmts = ("JPEG", "PNG", "OPEN_EXR", "WEBP")
    plain = {f: _render(rctx, s04, p, tmp_path, "plain", f, 100) for f in fmts}
    rctx.set_region((-5, -5, W + 9, H + 1), crop=crop)  # reaches beyond the frame: clamped to all of it
    for f in fmts:
        assert _render(rctx, s04, p, tmp_path, "region", f, 100) == plain[f], f


# ----------------------------------------------------------- 5: with reduce ---
def test_reduce_applies_to_the_cropped_film(rctx, rr, s04, full, tmp_path):
    x0, y0, x1, y1 = UNALIGNED
    rctx.set_exr_depth(32)
    rctx.set_region(UNALIGNED, crop=True)
    rctx.render_frame_outputs(s04, FRAME, _params(rr), [(tmp_path / "r2", "OPEN_EXR", 90, 2)])
    got = _words(_file(tmp_path / "r2", "OPEN_EXR"))
    # spp 4: inv_spp 0.25 commutes with the float32 sums of the reduction (test_gpu_multi_output)
    window = np.ascontiguousarray(full["tiles"][y0:y1, x0:x1]).view(np.float32)
    want = R.reduce(window, 2)
    assert got.shape == want.shape == ((y1 - y0 + 1) // 2, (x1 - x0 + 1) // 2, 4)
    assert np.array_equal(got[..., :3], want.view(np.uint32)[..., :3])
    assert np.all(got[..., 3] == 0x3F800000)


# ------------------------------------------------------ 6: frames in flight ---
def test_two_frames_in_flight_keep_their_own_regions(rctx, rr, s04, tmp_path):
    rctx.set_exr_depth(32)
    p = _params(rr)
    a, b = REGIONS["aligned"], UNALIGNED
    solo = {}
    for name, region in (("a", a), ("b", b)):
        rctx.set_region(region, crop=True)
        solo[name] = _render(rctx, s04, p, tmp_path, "solo_" + name, "OPEN_EXR")
    rctx.set_region(a, crop=True)
    ta = rctx.submit_frame(s04, FRAME, p, str(tmp_path / "fa"), "OPEN_EXR")
    rctx.set_region(b, crop=True)  # read at submit: the frame in flight keeps its own
    tb = rctx.submit_frame(s04, FRAME, p, str(tmp_path / "fb"), "OPEN_EXR")
    rctx.set_region(None)
    rctx.complete_frame(ta)
    rctx.complete_frame(tb)
    assert _file(tmp_path / "fa", "OPEN_EXR") == solo["a"]
    assert _file(tmp_path / "fb", "OPEN_EXR") == solo["b"]


# ------------------------------------------------------------- 7: refusals ---
def test_refusals_and_clamping(rctx, rr, s04, tmp_path):
    p = _params(rr)
    for bad in ((10, 10, 10, 20), (10, 10, 20, 10), (20, 5, 10, 9), (5, 20, 9, 10)):
        with pytest.raises(rr.RRError) as e:
            rctx.set_region(bad, crop=True)
        assert e.value.code == rr.native.RR_EINVAL
    assert rctx.region_resolution(s04, p) == (W, H)  # a refused value changed nothing
    rctx.set_region((70, 0, 90, 45), crop=True)  # nothing of it inside the frame
    for call in (lambda: rctx.render_frame(s04, FRAME, p, str(tmp_path / "e"), "JPEG", 90),
                 lambda: rctx.render_to_memory(s04, FRAME, p), lambda: rctx.region_resolution(s04, p)):
        with pytest.raises(rr.RRError) as e:
            call()
        assert e.value.code == rr.native.RR_EINVAL
        assert "(70, 0, 90, 45)" in str(e.value) and "70 x 45" in str(e.value)
    assert not list(tmp_path.iterdir())
    rctx.set_region((60, 40, 500, 400), crop=True)  # beyond the frame: clamped, not refused
    assert rctx.region_resolution(s04, p) == (10, 5)
    rctx.set_exr_depth(32)
    assert _words(_render(rctx, s04, p, tmp_path, "k", "OPEN_EXR")).shape == (5, 10, 4)
    rctx.set_region((60, 40, 500, 400), crop=False)
    assert rctx.region_resolution(s04, p) == (W, H)
    rctx.set_region(None)
    assert rctx.region_resolution(s04, p) == (W, H)


def test_stats_describe_what_ran(rctx, rr, s04):
    x0, y0, x1, y1 = UNALIGNED
    rctx.set_region(UNALIGNED, crop=True)
    _, _, split = rctx.render_to_memory(s04, FRAME, _params(rr, "split"))
    _, _, tiles = rctx.render_to_memory(s04, FRAME, _params(rr, "tiles"))
    assert split.camera_rays == (x1 - x0) * (y1 - y0) * SPP  # the split path traces the region's pixels alone
    # the tile path runs the 8 x 8 tiles that meet the region, partial tiles whole: columns 0 .. 63, rows 0 .. 47
    # cut at the frame's 45
    assert tiles.camera_rays == 64 * 45 * SPP
    rctx.set_region(REGIONS["aligned"], crop=True)
    _, _, tiles = rctx.render_to_memory(s04, FRAME, _params(rr, "tiles"))
    assert tiles.camera_rays == 16 * 8 * SPP
    rctx.set_region(REGIONS["pixel"], crop=False)
    _, _, tiles = rctx.render_to_memory(s04, FRAME, _params(rr, "tiles"))
    assert tiles.camera_rays == 64 * SPP


# --------------------------------------------------- the scene's own border ---
def test_scene_border_gives_the_region_only_after_the_opt_in(rctx, rr, full, tmp_path):
    """JSON -> RenderDesc -> region: min / max and the y flip, crop, and the opt-in."""
    doc = json.load(open(S04))
    doc["render"]["border"] = {"min_x": 0.1, "max_x": 0.5, "min_y": 0.0, "max_y": 0.2, "crop": True}
    path = tmp_path / "bordered.rrscene"
    path.write_text(json.dumps(doc))
    scene = rctx.load_scene(str(path))
    try:
        p = _params(rr)
        rctx.set_exr_depth(32)
        assert rctx.region_resolution(scene, p) == (W, H)  # not asked for: the scene renders whole
        assert np.array_equal(_words(_render(rctx, scene, p, tmp_path, "whole", "OPEN_EXR")), full["tiles"])
        rctx.set_region_from_scene(True)
        # x 7 .. 35; the bottom fifth: int(0.2 * 45) = 9 rows from the bottom, rows 36 .. 45 from the top
        assert rctx.region_resolution(scene, p) == (28, 9)
        got = _words(_render(rctx, scene, p, tmp_path, "part", "OPEN_EXR"))
        assert np.array_equal(got, full["tiles"][36:45, 7:35])
    finally:
        scene.close()


# ----------------------------------------------------------------- 8: shim ---
def test_shim_crops_to_the_region_of_the_environment(rr, full, tmp_path):
    x0, y0, x1, y1 = UNALIGNED
    env = {k: v for k, v in os.environ.items() if k != "RR_REGION"}
    env.update(RR_WIDTH=str(W), RR_HEIGHT=str(H), RR_SPP=str(SPP), RR_EXR_DEPTH="32", RR_REGION="3,5,61,44,1")
    argv = [rr.SHIM_PATH, S04.replace(".rrscene", ".blend"), "--background", "--python", "script.py", "--",
            "--render-output", str(tmp_path / "######"), "--render-format", "OPEN_EXR", "--render-frame", str(FRAME)]
    res = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    got = _words((tmp_path / f"{FRAME:06d}.exr").read_bytes())
    assert np.array_equal(got, full["tiles"][y0:y1, x0:x1])
    bad = subprocess.run(argv, capture_output=True, text=True, env=dict(env, RR_REGION="3,5,61"), timeout=60)
    assert bad.returncode != 0 and "RR_REGION='3,5,61'" in bad.stdout


# -------------------------------------------------------- 9: k_film_window ---
@pytest.mark.parametrize("crop", (False, True))
@pytest.mark.parametrize("w", (1, 63, 64, 65, 257))
def test_film_window_kernel_against_a_numpy_slice(mctx, w, crop):
    h = 5
    rng = np.random.default_rng(w)
    img = rng.standard_normal((h, w, 4)).astype(np.float32)
    img[0, 0] = (np.inf, -0.0, np.float32(1e-42), 7.0)  # bits, not values: infinities, zeros' signs, subnormals
    for region in {(0, 0, w, h), (w // 2, 1, w, h - 1), (0, 2, max(1, w - 1), 3), (w - 1, h - 1, w, h)}:
        x0, y0, x1, y1 = region
        got = mctx.film_window(img, region, crop, alpha_sum=4.0)
        inside = img[y0:y1, x0:x1].copy()
        inside[..., 3] = 4.0
        want = inside
        if not crop:
            want = np.zeros_like(img)
            want[y0:y1, x0:x1] = inside
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), region
