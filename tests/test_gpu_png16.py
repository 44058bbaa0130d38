"""The device 16-bit PNG path (png16.hip: mean, exposure, clamp, view transform,
quantize16, Sub filter over 8-byte pixels in front of deflate.hip's stages,
one zlib stream) writes files that the strict reader of tests/png16_reader.py
decodes to exactly the samples its numpy float32 restatement of the front end
gives, deterministically; the Filmic view agrees with the 8-bit path within
the two rounding rules; rendered frames of both render paths take it when the
resolved depth is 16, and 8-bit PNG frames keep their bytes."""
import io
import json
import os
import zlib

import numpy as np
import pytest
from PIL import Image

import png16_reader as P
from conftest import scene_path
from oracle import host_oracle as HO

pytestmark = pytest.mark.gpu

S04 = scene_path("04_very-simple-standin.rrscene")
S01 = scene_path("01_simple-animation.rrscene")
VIEWS = {"standard": 0, "raw": 1}


@pytest.fixture(scope="module")
def table(rr):
    return rr.native.srgb16_table()


def _decode(data, w, h):
    px, info = P.read_png16(data)  # raises on any deviation from the layout
    assert px.shape == (h, w, 4) and np.all(info["filters"] == 1)
    assert np.all(px[..., 3] == 65535)
    return px, info


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} samples differ, first at {bad[0]}: " \
                          f"{got[tuple(bad[0])]:#06x} != {want[tuple(bad[0])]:#06x}"


@pytest.mark.parametrize("view", sorted(VIEWS))
@pytest.mark.parametrize("w,h", P.SIZES)
def test_device_png16_round_trip(ctx, table, w, h, view):
    for kind in P.KINDS:
        img = P.make_image(kind, w, h, seed=w * 7 + h)
        scale = 1.0 if kind == "ramp" else 1.25
        data = ctx.png16_device(img, VIEWS[view], scale)
        px, info = _decode(data, w, h)
        want = P.front_end(img, VIEWS[view], scale, table)
        print(f"{kind} {view} {w}x{h}: file {len(data)} bytes, raw {len(info['raw'])}, "
              f"zlib level 1 {len(zlib.compress(info['raw'], 1))}")
        _same(px, want, f"{kind} {view} {w}x{h}")
        assert info["raw"] == P.filtered_bytes(want)
        if kind == "ramp" and view == "raw" and 3 * w * h >= 65536:
            assert len(np.unique(px[..., :3])) == 65536  # every 16-bit code went through
        im = Image.open(io.BytesIO(data))
        assert im.size == (w, h) and im.mode == "RGBA"
        assert ctx.png16_device(img, VIEWS[view], scale) == data, f"{kind} {w}x{h}: same image, other bytes"


def test_device_png16_flat_1080p(ctx, table):
    """A flat frame: Huffman codes alone cannot go below one bit a byte."""
    img = P.make_image("flat", 1920, 1080)
    data = ctx.png16_device(img, 0, 1.0)
    px, info = _decode(data, 1920, 1080)
    _same(px, P.front_end(img, 0, 1.0, table), "flat 1920x1080")
    raw = (8 * 1920 + 1) * 1080
    print(f"flat 1920x1080: file {len(data)} bytes, raw {raw}, ratio {len(data) / raw:.5f}")
    assert len(data) < 0.02 * raw


def test_sizes_outside_the_plan_are_refused(ctx, rr):
    """W above 2^19 (band positions in 32-bit counters): RR_EINVAL, no other route."""
    with pytest.raises(rr.native.RRError) as e:
        ctx.png16_device(np.zeros((1, (1 << 19) + 1, 4), np.float32))
    assert e.value.code == rr.native.RR_EINVAL
    ctx.set_ocio_config(None)
    with pytest.raises(rr.native.RRError) as e:  # Filmic needs the context's LUTs
        ctx.png16_device(np.zeros((2, 3, 4), np.float32), 2)
    assert e.value.code == rr.native.RR_EINVAL
    with pytest.raises(rr.native.RRError) as e:
        ctx.set_png_depth(12)
    assert e.value.code == rr.native.RR_EINVAL
    px, _ = _decode(ctx.png16_device(np.zeros((2, 3, 4), np.float32)), 3, 2)  # the context still works
    assert not px[..., :3].any()


def test_filmic_agrees_with_the_8_bit_path(ctx, rr, tmp_path):
    """Both paths quantise the same float d of the Filmic chain: c8 = floor(255 d
    + 0.5) and c16 = floor(65535 d + 0.5) give |255 d - c8| <= 0.5 and |65535 d
    - c16| <= 0.5, so |c16 / 257 - c8| <= 0.5 + 0.5 / 257 = 0.5 + 1 / 514."""
    HO.write_synthetic_filmic_luts(str(tmp_path), n3=33, n1=4096)
    ctx.set_ocio_config(str(tmp_path))
    s = ctx.load_scene(S01)
    try:
        p = rr.default_params(width=96, height=54, spp=8)
        film, rgba, st = ctx.render_to_memory(s, 30, p)
        assert st.view_transform == rr.native.RR_VIEW_FILMIC and st.view_transform_substituted == 0
        scale = float(ctx.frame_state(s, 30, p).render_floats[2])
        ctx.set_png_depth(16)
        _, st = ctx.render_frame(s, 30, p, str(tmp_path / "f"), "PNG", 0)
        data = (tmp_path / "f.png").read_bytes()
        assert st.output_bytes == len(data) and st.view_transform == rr.native.RR_VIEW_FILMIC
        px, _ = _decode(data, 96, 54)
        assert ctx.png16_device(film, 2, scale) == data  # the debug entry is the frame's coder
        # and on a synthetic image that spans the chain's range, against the 8-bit chain's oracle
        from oracle import oracle as O
        O.set_filmic(HO.load_filmic_luts(str(tmp_path)))
        rng = np.random.default_rng(3)
        img = np.zeros((64, 128, 4), np.float32)
        img[..., :3] = np.exp2(rng.uniform(-14, 5, (64, 128, 3))).astype(np.float32)
        img[0, :8, :3] = 0.0
        px2, _ = _decode(ctx.png16_device(img, 2, 1.0), 128, 64)
        c8 = O.filmic(img[..., :3].reshape(-1, 3)).reshape(64, 128, 3)
        for name, c16, ref in (("frame", px, rgba), ("synthetic", px2, c8)):
            err = np.abs(c16[..., :3].astype(np.float64) / 257.0 - ref[..., :3].astype(np.float64))
            print(f"filmic {name}: max |c16 / 257 - c8| = {err.max():.6f} (bound {0.5 + 1 / 514:.6f}), "
                  f"{len(np.unique(c16[..., :3]))} distinct 16-bit codes")
            assert err.max() <= 0.5 + 1 / 514
    finally:
        from oracle import oracle as O
        O.set_filmic(None)
        ctx.set_png_depth(0)
        ctx.set_ocio_config(None)
        s.close()


@pytest.mark.parametrize("path", ["tiles", "wavefront"])
def test_rendered_frame_png16(ctx, rr, table, tmp_path, path):
    """04vs, 250 x 141, 4 spp, on k_tiles and on the split path: the file's
    samples are the restatement applied to render_to_memory's film; the 8-bit
    PNG of the same frame is byte-identical with the setting at 0 or 8."""
    flags = rr.native.RR_FLAG_WAVEFRONT if path == "wavefront" else 0
    s = ctx.load_scene(S04)
    try:
        p = rr.default_params(spp=4, width=250, height=141, flags=flags)
        film, rgba, st0 = ctx.render_to_memory(s, 9, p)
        assert (st0.tile_slices > 0) == (path == "tiles")
        state = ctx.frame_state(s, 9, p)
        view, scale = int(state.render_ints[5]), float(state.render_floats[2])
        assert view == 0
        files = {}
        for dev in (False, True):
            ctx.set_device_png(dev)
            for depth in (None, 0, 8):  # None: no call yet made for this file
                if depth is not None:
                    ctx.set_png_depth(depth)
                ctx.render_frame(s, 9, p, str(tmp_path / "f8"), "PNG", 0)
                files[dev, depth] = (tmp_path / "f8.png").read_bytes()
            assert files[dev, None] == files[dev, 0] == files[dev, 8]
            im = Image.open(io.BytesIO(files[dev, 8]))
            assert im.mode == "RGBA" and np.array_equal(np.asarray(im), rgba)
            ctx.set_png_depth(16)  # 16 bits: the device coder, whatever rr_set_device_png says
            _, st = ctx.render_frame(s, 9, p, str(tmp_path / "f16"), "PNG", 0)
            data = (tmp_path / "f16.png").read_bytes()
            files[dev, 16] = data
            assert st.output_bytes == len(data)
            ctx.set_png_depth(0)
        assert files[False, 16] == files[True, 16]
        data = files[True, 16]
        px, info = _decode(data, 250, 141)
        want = P.front_end(film, view, scale, table)
        _same(px, want, f"04vs {path}")
        ref = P.write_png16(want, 1)
        print(f"04vs {path}: device {len(data)} bytes, zlib level 1 {len(ref)} bytes, ratio {len(data) / len(ref):.4f}")
        assert len(data) <= 1.25 * len(ref)  # the bound DESIGN §8 applies to the PNG and EXR coders
        idat = data[8 + 25 + 8:-12 - 4]
        assert zlib.decompress(idat) == info["raw"]
        im = Image.open(io.BytesIO(data))
        assert im.size == (250, 141) and im.mode == "RGBA"
        top = np.asarray(im.convert("RGBA")).astype(int)  # PIL keeps the top 8 bits
        assert np.max(np.abs(top - (px >> 8).astype(int))) <= 1
        assert np.max(np.abs((px[..., :3] / 257.0) - rgba[..., :3])) <= 1.0  # the 8-bit table differs by < 1/2 code
    finally:
        ctx.set_device_png(False)
        ctx.set_png_depth(0)
        s.close()


def test_scene_depth_and_environment(rr, tmp_path, monkeypatch, table):
    """render.color_depth = 16 selects the path when the context says 0; the
    context's 8 overrides it; RR_PNG_DEPTH sets the context's default."""
    with open(S04) as f:
        j = json.load(f)
    j["render"]["color_depth"] = 16
    (tmp_path / "s16.rrscene").write_text(json.dumps(j))
    p = rr.default_params(spp=2, width=64, height=36)

    def depth_of(c, scene_file, name):
        s = c.load_scene(scene_file)
        try:
            c.render_frame(s, 3, p, str(tmp_path / name), "PNG", 0)
        finally:
            s.close()
        return (tmp_path / (name + ".png")).read_bytes()[24]

    monkeypatch.delenv("RR_PNG_DEPTH", raising=False)
    with rr.RenderContext(0) as c:
        assert depth_of(c, S04, "a") == 8  # nothing set: the 8-bit file, and the same bytes once 0 or 8 is set
        for d in (0, 8):
            c.set_png_depth(d)
            assert depth_of(c, S04, "a%d" % d) == 8
            assert (tmp_path / ("a%d.png" % d)).read_bytes() == (tmp_path / "a.png").read_bytes()
        c.set_png_depth(0)
        assert depth_of(c, str(tmp_path / "s16.rrscene"), "b") == 16
        _decode((tmp_path / "b.png").read_bytes(), 64, 36)
        c.set_png_depth(8)
        assert depth_of(c, str(tmp_path / "s16.rrscene"), "c") == 8
    monkeypatch.setenv("RR_PNG_DEPTH", "16")
    with rr.RenderContext(0) as c:
        assert depth_of(c, S04, "d") == 16
    monkeypatch.setenv("RR_PNG_DEPTH", "12")
    with pytest.raises(rr.native.RRError) as e:
        rr.RenderContext(0)
    assert e.value.code == rr.native.RR_EINVAL
    monkeypatch.delenv("RR_PNG_DEPTH")
    with rr.RenderContext(0, png_depth=16) as c:
        assert depth_of(c, S04, "e") == 16


def test_frames_in_flight_keep_their_own_png16_buffers(ctx, rr, table, tmp_path):
    """Three 16-bit frames pending together, then 16-bit, 8-bit device PNG and EXR mixed."""
    s = ctx.load_scene(S04)
    try:
        p = rr.default_params(spp=4, width=250, height=141)
        frames = [3, 4, 5]
        scale = float(ctx.frame_state(s, 3, p).render_floats[2])
        want = {f: P.front_end(ctx.render_to_memory(s, f, p)[0], 0, scale, table) for f in frames}
        rgba4 = ctx.render_to_memory(s, 4, p)[1]
        assert not np.array_equal(want[3], want[5])
        ctx.set_png_depth(16)
        tickets = [ctx.submit_frame(s, f, p, str(tmp_path / f"f{f}"), "PNG") for f in frames]
        for t in tickets:
            ctx.complete_frame(t)
        for f in frames:
            _same(_decode((tmp_path / f"f{f}.png").read_bytes(), 250, 141)[0], want[f], f"frame {f}")
        ctx.set_device_png(True)
        t3 = ctx.submit_frame(s, 3, p, str(tmp_path / "a"), "PNG")
        ctx.set_png_depth(8)  # frames in flight keep their choice
        t4 = ctx.submit_frame(s, 4, p, str(tmp_path / "b"), "PNG")
        t5 = ctx.submit_frame(s, 5, p, str(tmp_path / "c"), "OPEN_EXR")
        for t in (t3, t4, t5):
            ctx.complete_frame(t)
        _same(_decode((tmp_path / "a.png").read_bytes(), 250, 141)[0], want[3], "mixed frame 3")
        assert np.array_equal(np.asarray(Image.open(tmp_path / "b.png").convert("RGBA")), rgba4)
        assert (tmp_path / "c.exr").stat().st_size > 0
    finally:
        ctx.set_device_png(False)
        ctx.set_png_depth(0)
        s.close()


def test_backend_runner_png16_job(rr, table, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    job = rr.BlenderJob.load_from_file(os.path.join(root, "jobs", "04_very-simple_demo_10f-1w.toml"))
    job = rr.BlenderJob.from_dict({**job.to_dict(), "output_directory_path": str(tmp_path / "out"),
                                   "output_file_format": "PNG"})
    p = rr.default_params(width=64, height=36, spp=2)
    runner = rr.BackendRunner(root, params=p, png_depth=16)
    try:
        runner.render_frames(job, [1, 2, 3])
        assert sorted(os.listdir(tmp_path / "out")) == ["000001.png", "000002.png", "000003.png"]
        s = runner._scenes[next(iter(runner._scenes))]
        for f in (1, 2, 3):
            scale = float(runner.ctx.frame_state(s, f, p).render_floats[2])
            want = P.front_end(runner.ctx.render_to_memory(s, f, p)[0], 0, scale, table)
            _same(_decode((tmp_path / "out" / f"{f:06d}.png").read_bytes(), 64, 36)[0], want, f"job frame {f}")
    finally:
        runner.close()
