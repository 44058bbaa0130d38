"""The device OPEN_EXR path (exr.hip: half conversion, plane split, byte
reorder and predictor in front of deflate.hip's stages, every 16-row chunk
a zlib stream of its own with a raw fallback) writes files that the strict
reader of tests/exr_reader.py decodes to exactly float16(clip(film)),
deterministically, within size conditions that only working matches over the
plane distance meet; rendered frames of both render paths take it for the
format "OPEN_EXR"; frames in flight, of mixed formats too, do not share its
buffers."""
import os
import zlib

import numpy as np
import pytest
from PIL import Image

import exr_reader as X
from conftest import scene_path

pytestmark = pytest.mark.gpu


def _decode(data, w, h):
    px, header, sizes, modes = X.read_exr(data)  # raises on any deviation from the layout
    assert px.shape == (h, w, 4)
    assert header["dataWindow"] == header["displayWindow"] == (0, 0, w - 1, h - 1)
    assert [c["name"] for c in header["channels"]] == ["A", "B", "G", "R"]
    assert all(c["pixelType"] == 1 for c in header["channels"])
    assert header["compression"] == 3 and header["lineOrder"] == 0
    assert header["pixelAspectRatio"] == 1.0 and header["screenWindowWidth"] == 1.0
    for k, s in enumerate(sizes):  # the raw rule: no chunk larger than its pixels
        assert s <= 8 * w * min(16, h - 16 * k)
    return px, sizes, modes


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} halfs differ, first at {bad[0]}: " \
                          f"{got[tuple(bad[0])]:#06x} != {want[tuple(bad[0])]:#06x}"


@pytest.mark.parametrize("w,h", X.SIZES)
def test_device_exr_round_trip(ctx, w, h):
    for kind in X.KINDS:
        img = X.make_image(kind, w, h, seed=w * 7 + h)
        data = ctx.exr_device(img)
        px, sizes, modes = _decode(data, w, h)
        print(f"{kind} {w}x{h}: file {len(data)} bytes, raw {8 * w * h}, ratio {len(data) / (8 * w * h):.4f}, "
              f"{modes.count('raw')} of {len(modes)} chunks raw")
        _same(px, X.expected_halfs(img), f"{kind} {w}x{h}")
        assert ctx.exr_device(img) == data, f"{kind} {w}x{h}: same image, other bytes"


def test_device_exr_1080p(ctx):
    img = X.make_image("grey", 1920, 1080, seed=1)
    data = ctx.exr_device(img)
    px, sizes, modes = _decode(data, 1920, 1080)
    print(f"grey 1920x1080: file {len(data)} bytes, ratio {len(data) / (8 * 1920 * 1080):.4f}")
    _same(px, X.expected_halfs(img), "grey 1920x1080")


def test_incompressible_chunks_are_raw(ctx):
    """Uniformly random half bit patterns: zlib at its best level cannot shrink a
    band (the precondition), so no coder could have done better than raw."""
    w, h = 256, 64
    img = X.make_image("bits", w, h, seed=5)
    want = X.expected_halfs(img)
    for y in range(0, h, 16):
        raw = X.chunk_bytes(want[y:y + 16])
        assert len(zlib.compress(X.preprocess(raw), 9)) >= len(raw)
    data = ctx.exr_device(img)
    px, sizes, modes = _decode(data, w, h)
    assert modes == ["raw"] * 4 and sizes == [8 * w * 16] * 4
    _same(px, want, "bits 256x64")


def test_flat_frame_needs_matches(ctx):
    """Huffman codes alone cannot go below one bit a byte (0.125 of raw)."""
    img = X.make_image("flat", 1920, 1080)
    data = ctx.exr_device(img)
    px, _, modes = _decode(data, 1920, 1080)
    _same(px, X.expected_halfs(img), "flat 1920x1080")
    raw = 8 * 1920 * 1080
    print(f"flat 1920x1080: file {len(data)} bytes, raw {raw}, ratio {len(data) / raw:.5f}")
    assert len(data) < 0.02 * raw


def test_grey_pixels_take_the_plane_distance(ctx):
    """R = G = B: the G and R planes repeat the B plane W bytes back."""
    w, h = 333, 257
    grey = ctx.exr_device(X.make_image("grey", w, h, seed=9))
    noise = ctx.exr_device(X.make_image("noise", w, h, seed=9))
    _decode(grey, w, h)
    _decode(noise, w, h)
    print(f"333x257: grey {len(grey)} bytes, independent channels {len(noise)} bytes")
    assert len(grey) < len(noise)


def _scene(ctx, which):
    return ctx.load_scene(scene_path("04_very-simple-standin.rrscene" if which == "04vs"
                                     else "02_physics-standin.rrscene"))


def _film_halfs(film):
    assert np.all(film[..., 3] == 1.0)
    return X.expected_halfs(film)


@pytest.mark.parametrize("which,frame", [("04vs", 9), ("02", 90)])
def test_rendered_frame_exr(ctx, rr, tmp_path, which, frame):
    """Tile path (04vs) and split path (02): the file decodes to the halfs of the
    film render_to_memory returns for the frame, and is at most 1.25 times the
    reference writer's zlib level 1 file of the same pixels (the bound DESIGN §8
    applies to the PNG coder)."""
    s = _scene(ctx, which)
    try:
        p = rr.default_params(spp=4, width=250, height=141)
        film, _, _ = ctx.render_to_memory(s, frame, p)
        _, stats = ctx.render_frame(s, frame, p, str(tmp_path / "f"), "OPEN_EXR", 0)  # the quality is ignored
        data = (tmp_path / "f.exr").read_bytes()
        assert stats.output_bytes == len(data)
        px, _, modes = _decode(data, 250, 141)
        want = _film_halfs(film)
        _same(px, want, f"{which} frame {frame}")
        ref = X.write_exr(want, 1)
        print(f"{which} frame {frame}: device {len(data)} bytes, zlib level 1 {len(ref)} bytes, "
              f"ratio {len(data) / len(ref):.4f}, {modes.count('raw')} of {len(modes)} chunks raw")
        assert len(data) <= 1.25 * len(ref)
    finally:
        s.close()


def test_frames_in_flight_keep_their_own_exr_buffers(ctx, rr, tmp_path):
    s = _scene(ctx, "04vs")
    try:
        p = rr.default_params(spp=4, width=250, height=141)
        frames = [3, 4, 5]
        want = {f: _film_halfs(ctx.render_to_memory(s, f, p)[0]) for f in frames}
        assert not np.array_equal(want[3], want[5])
        tickets = [ctx.submit_frame(s, f, p, str(tmp_path / f"f{f}"), "OPEN_EXR") for f in frames]
        for t in tickets:
            ctx.complete_frame(t)
        for f in frames:
            px, _, _ = _decode((tmp_path / f"f{f}.exr").read_bytes(), 250, 141)
            _same(px, want[f], f"frame {f}")
    finally:
        s.close()


def test_mixed_formats_in_flight(ctx, rr, tmp_path):
    """A device-PNG frame, an EXR frame and a JPEG frame pending together in one context."""
    s = _scene(ctx, "04vs")
    try:
        p = rr.default_params(spp=4, width=250, height=141)
        film4 = ctx.render_to_memory(s, 4, p)[0]
        rgba3 = ctx.render_to_memory(s, 3, p)[1]
        ctx.render_frame(s, 5, p, str(tmp_path / "serial"), "JPEG", 90)
        ctx.set_device_png(True)
        tickets = [ctx.submit_frame(s, 3, p, str(tmp_path / "a"), "PNG"),
                   ctx.submit_frame(s, 4, p, str(tmp_path / "b"), "OPEN_EXR"),
                   ctx.submit_frame(s, 5, p, str(tmp_path / "c"), "JPEG", 90)]
        for t in tickets:
            ctx.complete_frame(t)
        assert np.array_equal(np.asarray(Image.open(tmp_path / "a.png").convert("RGBA")), rgba3)
        px, _, _ = _decode((tmp_path / "b.exr").read_bytes(), 250, 141)
        _same(px, _film_halfs(film4), "frame 4")
        assert (tmp_path / "c.jpg").read_bytes() == (tmp_path / "serial.jpg").read_bytes()
    finally:
        ctx.set_device_png(False)
        s.close()


def test_sizes_outside_the_plan_are_refused(ctx, rr):
    """W above 2^19 (band positions in 32-bit counters): RR_EINVAL, no other route."""
    w = (1 << 19) + 1
    with pytest.raises(rr.native.RRError) as e:
        ctx.exr_device(np.zeros((1, w, 4), np.float32))
    assert e.value.code == rr.native.RR_EINVAL
    px, _, _ = _decode(ctx.exr_device(np.zeros((2, 3, 4), np.float32)), 3, 2)  # the context still works
    assert not px.any()


def test_backend_runner_open_exr_job(ctx, rr, tmp_path):
    """A job that asks for OPEN_EXR renders through BackendRunner to .exr files
    that decode to the film's halfs."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    job = rr.BlenderJob.load_from_file(os.path.join(root, "jobs", "04_very-simple_demo_10f-1w.toml"))
    job = rr.BlenderJob.from_dict({**job.to_dict(), "output_directory_path": str(tmp_path / "out"),
                                   "output_file_format": "OPEN_EXR"})
    p = rr.default_params(width=64, height=36, spp=2)
    runner = rr.BackendRunner(root, params=p)
    try:
        runner.render_frames(job, [1, 2, 3])
        assert sorted(os.listdir(tmp_path / "out")) == ["000001.exr", "000002.exr", "000003.exr"]
        s = runner._scenes[next(iter(runner._scenes))]
        for f in (1, 2, 3):
            want = _film_halfs(runner.ctx.render_to_memory(s, f, p)[0])
            px, _, _ = _decode((tmp_path / "out" / f"{f:06d}.exr").read_bytes(), 64, 36)
            _same(px, want, f"job frame {f}")
    finally:
        runner.close()
