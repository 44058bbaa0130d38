"""The device OPEN_EXR path with FLOAT channels (exr.hip ExrFloatFront: plane
split, byte reorder and predictor over 4-byte samples in front of deflate.hip's
stages, every 16-row chunk a zlib stream of its own with a raw fallback) writes
files that the strict reader of tests/exr32_reader.py decodes to the film's
floats bit for bit, deterministically, within size conditions that only
working matches over the sample and plane distances meet; rr_set_exr_depth, a
scene's render.exr_depth and BackendRunner(exr_depth=) select it for
"OPEN_EXR" frames of both render paths, HALF files keep their bytes, and
frames in flight, of mixed formats too, do not share its buffers."""
import json
import os
import zlib

import numpy as np
import pytest

import exr32_reader as F
import exr_reader as X
import png16_reader as P
from conftest import scene_path

pytestmark = pytest.mark.gpu

S04 = scene_path("04_very-simple-standin.rrscene")
S02 = scene_path("02_physics-standin.rrscene")
W_MAX = 1 << 18  # exr32_plan: a band's 256 W bytes at 16 bits each stay below 2^30, as exr_plan's 128 W at 2^19


def _decode(data, w, h):
    px, header, sizes, modes = F.read_exr32(data)  # raises on any deviation from the layout
    assert px.shape == (h, w, 4) and px.dtype == np.uint32
    assert header["dataWindow"] == header["displayWindow"] == (0, 0, w - 1, h - 1)
    assert [c["name"] for c in header["channels"]] == ["A", "B", "G", "R"]
    assert all(c["pixelType"] == 2 for c in header["channels"])
    assert header["compression"] == 3 and header["lineOrder"] == 0
    for k, s in enumerate(sizes):  # the raw rule: no chunk larger than its pixels
        assert s <= 16 * w * min(16, h - 16 * k)
    return px, sizes, modes


def _same(got, want, what):
    assert got.dtype == want.dtype == np.uint32
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} floats differ, first at {bad[0]}: " \
                          f"{got[tuple(bad[0])]:#010x} != {want[tuple(bad[0])]:#010x}"


@pytest.mark.parametrize("w,h", F.SIZES)
def test_device_exr32_round_trip(ctx, w, h):
    for kind in F.KINDS:
        img = F.make_image(kind, w, h, seed=w * 7 + h)
        data = ctx.exr32_device(img)
        px, sizes, modes = _decode(data, w, h)
        print(f"{kind} {w}x{h}: file {len(data)} bytes, raw {16 * w * h}, ratio {len(data) / (16 * w * h):.4f}, "
              f"{modes.count('raw')} of {len(modes)} chunks raw")
        _same(px, F.bits(img), f"{kind} {w}x{h}")
        assert ctx.exr32_device(img) == data, f"{kind} {w}x{h}: same image, other bytes"


def test_values_half_cannot_hold_survive(ctx):
    """Above 65504, float subnormals, infinities: the FLOAT file has them, the
    HALF file of the same image has clamped or flushed them."""
    img = F.make_image("values32", 40, 20, seed=2)
    want = F.bits(img)
    mag = want & 0x7FFFFFFF
    big = np.isfinite(img) & (np.abs(img) > 65504)
    sub = (mag > 0) & (mag < 0x00800000)
    assert big.any() and sub.any() and np.isinf(img).any()
    px, _, _ = _decode(ctx.exr32_device(img), 40, 20)
    _same(px, want, "values32 40x20")
    half = X.read_exr(ctx.exr_device(img))[0].view(np.float16).astype(np.float32)
    assert np.all(np.abs(half[big]) == 65504) and np.all(half[sub] == 0)  # what the HALF path does to them


def test_incompressible_chunks_are_raw(ctx):
    """Uniformly random 32-bit patterns: zlib at its best level cannot shrink a
    band (the precondition), so no coder could have done better than raw."""
    w, h = 128, 64
    img = F.make_image("bits32", w, h, seed=5)
    want = F.bits(img)
    for y in range(0, h, 16):
        raw = F.chunk_bytes(want[y:y + 16])
        assert len(zlib.compress(X.preprocess(raw), 9)) >= len(raw)
    data = ctx.exr32_device(img)
    px, sizes, modes = _decode(data, w, h)
    assert modes == ["raw"] * 4 and sizes == [16 * w * 16] * 4
    _same(px, want, "bits32 128x64")


def test_flat_frame_needs_matches(ctx):
    """Huffman codes alone cannot go below one bit a byte (0.125 of raw)."""
    img = F.make_image("flat", 1920, 1080)
    data = ctx.exr32_device(img)
    px, _, modes = _decode(data, 1920, 1080)
    _same(px, F.bits(img), "flat 1920x1080")
    raw = 16 * 1920 * 1080
    print(f"flat 1920x1080: file {len(data)} bytes, raw {raw}, ratio {len(data) / raw:.5f}")
    assert len(data) < 0.02 * raw


def test_grey_pixels_take_the_plane_distance(ctx):
    """R = G = B: the G and R planes repeat the B plane 2W bytes back."""
    w, h = 333, 257
    grey = ctx.exr32_device(F.make_image("grey", w, h, seed=9))
    noise = ctx.exr32_device(F.make_image("noise", w, h, seed=9))
    _decode(grey, w, h)
    _decode(noise, w, h)
    print(f"333x257: grey {len(grey)} bytes, independent channels {len(noise)} bytes")
    assert len(grey) < len(noise)


def _film_bits(film):
    assert np.all(film[..., 3] == 1.0)
    return F.bits(film)


@pytest.mark.parametrize("which,frame", [("04vs", 9), ("02", 90)])
def test_rendered_frame_exr32(ctx, rr, tmp_path, which, frame):
    """Tile path (04vs) and split path (02): the file decodes to the bits of the
    film render_to_memory returns for the frame, and is at most 1.25 times the
    reference writer's zlib level 1 file of the same floats (the bound DESIGN §8
    applies to every front end of the deflate coder)."""
    s = ctx.load_scene(S04 if which == "04vs" else S02)
    try:
        p = rr.default_params(spp=4, width=250, height=141)
        film, _, st0 = ctx.render_to_memory(s, frame, p)
        assert (st0.tile_slices > 0) == (which == "04vs")
        ctx.set_exr_depth(32)
        _, stats = ctx.render_frame(s, frame, p, str(tmp_path / "f"), "OPEN_EXR", 0)  # the quality is ignored
        data = (tmp_path / "f.exr").read_bytes()
        assert stats.output_bytes == len(data)
        px, _, modes = _decode(data, 250, 141)
        want = _film_bits(film)
        _same(px, want, f"{which} frame {frame}")
        ref = F.write_exr32(want, 1)
        print(f"{which} frame {frame}: device {len(data)} bytes, zlib level 1 {len(ref)} bytes, "
              f"ratio {len(data) / len(ref):.4f}, {modes.count('raw')} of {len(modes)} chunks raw")
        assert len(data) <= 1.25 * len(ref)
    finally:
        ctx.set_exr_depth(0)
        s.close()


def test_scene_depth_and_environment(rr, tmp_path, monkeypatch):
    """render.exr_depth = 32 selects the path when the context says 0; the
    context's 16 overrides it; RR_EXR_DEPTH sets the context's default."""
    with open(S04) as f:
        j = json.load(f)
    j["render"]["exr_depth"] = 32
    (tmp_path / "s32.rrscene").write_text(json.dumps(j))
    s32 = str(tmp_path / "s32.rrscene")
    p = rr.default_params(spp=2, width=64, height=36)

    def type_of(c, scene_file, name):
        s = c.load_scene(scene_file)
        try:
            c.render_frame(s, 3, p, str(tmp_path / name), "OPEN_EXR", 0)
        finally:
            s.close()
        data = (tmp_path / (name + ".exr")).read_bytes()
        try:
            _decode(data, 64, 36)
            return 32
        except F.ExrError:
            X.read_exr(data)
            return 16

    monkeypatch.delenv("RR_EXR_DEPTH", raising=False)
    with rr.RenderContext(0) as c:
        assert type_of(c, S04, "a") == 16  # nothing set: the HALF file, and the same bytes once 0 or 16 is set
        for d in (0, 16):
            c.set_exr_depth(d)
            assert type_of(c, S04, "a%d" % d) == 16
            assert (tmp_path / ("a%d.exr" % d)).read_bytes() == (tmp_path / "a.exr").read_bytes()
        c.set_exr_depth(0)
        assert type_of(c, s32, "b") == 32
        c.set_exr_depth(16)
        assert type_of(c, s32, "c") == 16
        assert (tmp_path / "c.exr").read_bytes() == (tmp_path / "a.exr").read_bytes()
        c.set_exr_depth(32)
        assert type_of(c, S04, "d") == 32
        assert (tmp_path / "d.exr").read_bytes() == (tmp_path / "b.exr").read_bytes()
        for bad in (8, 24, -1, 64):
            with pytest.raises(rr.native.RRError) as e:
                c.set_exr_depth(bad)
            assert e.value.code == rr.native.RR_EINVAL
        assert type_of(c, S04, "d2") == 32  # a refused value changes nothing
    monkeypatch.setenv("RR_EXR_DEPTH", "32")
    with rr.RenderContext(0) as c:
        assert type_of(c, S04, "e") == 32
    monkeypatch.setenv("RR_EXR_DEPTH", "24")
    with pytest.raises(rr.native.RRError) as e:
        rr.RenderContext(0)
    assert e.value.code == rr.native.RR_EINVAL
    monkeypatch.delenv("RR_EXR_DEPTH")
    with rr.RenderContext(0, exr_depth=32) as c:
        assert type_of(c, S04, "g") == 32


def test_mixed_frames_in_flight_keep_their_own_buffers(ctx, rr, tmp_path):
    """A HALF frame, a FLOAT frame and a 16-bit PNG frame pending together: each
    decodes to its own frame; frames in flight keep the depth they were
    submitted with."""
    s = ctx.load_scene(S04)
    try:
        p = rr.default_params(spp=4, width=250, height=141)
        films = {f: ctx.render_to_memory(s, f, p)[0] for f in (3, 4, 5)}
        assert not np.array_equal(films[3], films[5])
        scale = float(ctx.frame_state(s, 5, p).render_floats[2])
        ctx.set_png_depth(16)
        t3 = ctx.submit_frame(s, 3, p, str(tmp_path / "a"), "OPEN_EXR")
        ctx.set_exr_depth(32)
        t4 = ctx.submit_frame(s, 4, p, str(tmp_path / "b"), "OPEN_EXR")
        ctx.set_exr_depth(16)  # frames in flight keep their choice
        t5 = ctx.submit_frame(s, 5, p, str(tmp_path / "c"), "PNG")
        for t in (t3, t4, t5):
            ctx.complete_frame(t)
        half = X.read_exr((tmp_path / "a.exr").read_bytes())[0]
        assert np.array_equal(half, X.expected_halfs(films[3]))
        _same(_decode((tmp_path / "b.exr").read_bytes(), 250, 141)[0], _film_bits(films[4]), "frame 4")
        px16, _ = P.read_png16((tmp_path / "c.png").read_bytes())
        assert np.array_equal(px16, P.front_end(films[5], 0, scale, rr.native.srgb16_table()))
        # three FLOAT frames together
        ctx.set_exr_depth(32)
        tickets = [ctx.submit_frame(s, f, p, str(tmp_path / f"f{f}"), "OPEN_EXR") for f in (3, 4, 5)]
        for t in tickets:
            ctx.complete_frame(t)
        for f in (3, 4, 5):
            _same(_decode((tmp_path / f"f{f}.exr").read_bytes(), 250, 141)[0], _film_bits(films[f]), f"frame {f}")
    finally:
        ctx.set_exr_depth(0)
        ctx.set_png_depth(0)
        s.close()


def test_half_files_keep_their_bytes_across_the_switch(ctx, rr, tmp_path):
    """After set_exr_depth(32) and back to 0, exr_device and rendered
    "OPEN_EXR" files are byte-identical to those made before."""
    s = ctx.load_scene(S04)
    try:
        p = rr.default_params(spp=4, width=250, height=141)
        img = X.make_image("gradient", 333, 257, seed=4)
        before = ctx.exr_device(img)
        ctx.render_frame(s, 9, p, str(tmp_path / "before"), "OPEN_EXR", 0)
        ctx.set_exr_depth(32)
        assert ctx.exr_device(img) == before  # the inspection call is HALF whatever the depth
        full = ctx.exr32_device(img)
        _decode(full, 333, 257)
        ctx.render_frame(s, 9, p, str(tmp_path / "full"), "OPEN_EXR", 0)
        _decode((tmp_path / "full.exr").read_bytes(), 250, 141)
        ctx.set_exr_depth(0)
        assert ctx.exr_device(img) == before
        ctx.render_frame(s, 9, p, str(tmp_path / "after"), "OPEN_EXR", 0)
        assert (tmp_path / "after.exr").read_bytes() == (tmp_path / "before.exr").read_bytes()
        X.read_exr((tmp_path / "after.exr").read_bytes())
    finally:
        ctx.set_exr_depth(0)
        s.close()


def test_sizes_outside_the_plan_are_refused(ctx, rr):
    """W above 2^18 (band positions and bit offsets in 32-bit counters, a band
    of twice the HALF path's bytes): RR_EINVAL, no other route."""
    with pytest.raises(rr.native.RRError) as e:
        ctx.exr32_device(np.zeros((1, W_MAX + 1, 4), np.float32))
    assert e.value.code == rr.native.RR_EINVAL
    px, _, _ = _decode(ctx.exr32_device(np.zeros((2, 3, 4), np.float32)), 3, 2)  # the context still works
    assert not px.any()


def test_backend_runner_exr32_job(rr, tmp_path):
    """BackendRunner(exr_depth=32): an OPEN_EXR job renders to .exr files that
    decode to the film's floats."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    job = rr.BlenderJob.load_from_file(os.path.join(root, "jobs", "04_very-simple_demo_10f-1w.toml"))
    job = rr.BlenderJob.from_dict({**job.to_dict(), "output_directory_path": str(tmp_path / "out"),
                                   "output_file_format": "OPEN_EXR"})
    p = rr.default_params(width=64, height=36, spp=2)
    runner = rr.BackendRunner(root, params=p, exr_depth=32)
    try:
        runner.render_frames(job, [1, 2, 3])
        assert sorted(os.listdir(tmp_path / "out")) == ["000001.exr", "000002.exr", "000003.exr"]
        s = runner._scenes[next(iter(runner._scenes))]
        for f in (1, 2, 3):
            want = _film_bits(runner.ctx.render_to_memory(s, f, p)[0])
            px, _, _ = _decode((tmp_path / "out" / f"{f:06d}.exr").read_bytes(), 64, 36)
            _same(px, want, f"job frame {f}")
    finally:
        runner.close()
