"""OPEN_EXR with FLOAT channels, the parts that need no GPU: the strict reader of
tests/exr32_reader.py round-trips its reference writer over the device
encoder's case list and rejects damaged files and HALF files (as exr_reader
rejects FLOAT ones); the C ABI exports the new entries without an ABI bump;
scenes carry render.exr_depth; the runner passes the depth on; the exporter
leaves the committed projects' scenes as they are."""
import json
import os
import struct
import types
import zlib

import numpy as np
import pytest

import exr32_reader as F
import exr_reader as X
from conftest import ROOT, scene_path


@pytest.mark.parametrize("w,h", F.SIZES + [(128, 64)])
def test_reader_round_trips_reference_writer(w, h):
    for kind in F.KINDS:
        px = F.bits(F.make_image(kind, w, h, seed=w * 7 + h))
        assert px.dtype == np.uint32 and px.shape == (h, w, 4)
        data = F.write_exr32(px)
        back, header, sizes, modes = F.read_exr32(data)
        assert np.array_equal(back, px), kind
        assert header["dataWindow"] == (0, 0, w - 1, h - 1)
        assert all(c["pixelType"] == 2 for c in header["channels"])
        assert len(sizes) == (h + 15) // 16 and all(s <= 16 * w * min(16, h) for s in sizes)
        if kind == "flat" and w * h >= 512:
            assert set(modes) == {"zip"}
        if kind == "bits32" and (w, h) == (128, 64):
            assert set(modes) == {"raw"}


def test_image_kinds_hold_what_they_promise():
    b = F.bits(F.make_image("bits32", 128, 64, seed=5))
    mag = b & 0x7FFFFFFF
    assert not np.any(mag > 0x7F800000)  # no NaN
    assert np.any((mag > 0) & (mag < 0x00800000)) and len(np.unique(b >> 24)) == 256  # subnormals; every top byte
    v = F.make_image("values32", 16, 16, seed=1)
    mag = F.bits(v) & 0x7FFFFFFF
    assert np.any(np.isinf(v)) and np.any(np.abs(v) == np.finfo(np.float32).max)
    assert np.any((mag > 0) & (mag < 0x00800000)) and np.any(np.isfinite(v) & (np.abs(v) > 65504))
    assert not np.any(np.isnan(v))


def test_float_layout_is_the_documented_one():
    """One pixel: A, B, G, R as little-endian floats; after the reorder the
    first half alternates bytes 0 and 2 of consecutive samples, the second
    bytes 1 and 3."""
    px = np.array([[[0x04030201, 0x14131211, 0x24232221, 0x34333231]]], np.uint32)  # R G B A
    raw = F.chunk_bytes(px)
    assert raw == bytes([0x31, 0x32, 0x33, 0x34, 0x21, 0x22, 0x23, 0x24, 0x11, 0x12, 0x13, 0x14, 1, 2, 3, 4])
    t = np.frombuffer(X.preprocess(raw), np.uint8).astype(int)
    undone = np.cumsum(np.concatenate([t[:1], t[1:] - 128])) & 0xFF
    assert list(undone) == [0x31, 0x33, 0x21, 0x23, 0x11, 0x13, 1, 3, 0x32, 0x34, 0x22, 0x24, 0x12, 0x14, 2, 4]
    assert X.unprocess(X.preprocess(raw)) == raw


def _two_chunk_file():
    px = F.bits(F.make_image("gradient", 40, 20, seed=3))
    data = F.write_exr32(px)
    _, _, sizes, modes = F.read_exr32(data)
    assert modes == ["zip", "zip"]
    return data, len(F.header_bytes(40, 20)), sizes


def test_reader_rejects_damaged_files():
    data, table, sizes = _two_chunk_file()
    with pytest.raises(F.ExrError):  # truncated
        F.read_exr32(data[:-1])
    with pytest.raises(F.ExrError):
        F.read_exr32(data[:table + 12])
    with pytest.raises(F.ExrError, match="after the last chunk"):
        F.read_exr32(data + b"\0")
    bad = bytearray(data)  # the second offset is off by one
    struct.pack_into("<Q", bad, table + 8, struct.unpack_from("<Q", data, table + 8)[0] + 1)
    with pytest.raises(F.ExrError, match="offset table"):
        F.read_exr32(bytes(bad))
    bad = bytearray(data)  # the first chunk's Adler-32
    end = table + 16 + 8 + sizes[0]
    bad[end - 1] ^= 1
    with pytest.raises(F.ExrError, match="chunk 0"):
        F.read_exr32(bytes(bad))
    # an attribute too many, and one missing
    extra = data[:table - 1] + X._attr("owner", "float", struct.pack("<f", 1.0)) + b"\0"
    with pytest.raises(F.ExrError, match="attributes"):
        F.read_exr32(extra + data[table:])
    head = F.header_bytes(40, 20)
    cut = head.index(b"lineOrder\0")
    with pytest.raises(F.ExrError, match="attributes"):
        F.read_exr32(head[:cut] + head[cut + len(X._attr("lineOrder", "lineOrder", b"\0")):] + data[table:])


def _replace_first_chunk(data, table, sizes, body):
    """The two-chunk file with `body` as its first chunk, offsets mended."""
    at = table + 16
    second = at + 8 + len(body)
    return (data[:table] + struct.pack("<QQ", at, second) + struct.pack("<ii", 0, len(body)) + body
            + data[at + 8 + sizes[0]:])


def test_reader_requires_exact_chunks():
    data, table, sizes = _two_chunk_file()
    n = 16 * 40 * 16
    F.read_exr32(_replace_first_chunk(data, table, sizes, data[table + 24:table + 24 + sizes[0]]))  # the helper itself
    with pytest.raises(F.ExrError, match="inflates to 100"):
        F.read_exr32(_replace_first_chunk(data, table, sizes, zlib.compress(b"\0" * 100, 1)))
    with pytest.raises(F.ExrError, match=f"{n} uncompressed"):  # larger than its scanlines
        F.read_exr32(_replace_first_chunk(data, table, sizes, b"\0" * (n + 1)))
    z = data[table + 24:table + 24 + sizes[0]]
    with pytest.raises(F.ExrError, match="one complete zlib stream"):  # a stream and a byte
        F.read_exr32(_replace_first_chunk(data, table, sizes, z + b"\0"))
    with pytest.raises(F.ExrError, match="one complete zlib stream"):  # a stream cut short
        F.read_exr32(_replace_first_chunk(data, table, sizes, z[:-5]))


def test_readers_reject_the_other_channel_type():
    half = X.write_exr(X.expected_halfs(X.make_image("gradient", 40, 20, seed=3)))
    X.read_exr(half)
    with pytest.raises(F.ExrError, match="pixelType 1"):
        F.read_exr32(half)
    full = F.write_exr32(F.bits(F.make_image("gradient", 40, 20, seed=3)))
    with pytest.raises(X.ExrError, match="channel"):
        X.read_exr(full)


def test_new_entries_exported_without_abi_bump(rr):
    lib = rr.native.lib()
    header = open(os.path.join(ROOT, "include", "rr.h")).read()
    for name in ("rr_set_exr_depth", "rr_debug_exr32_device"):
        assert name in rr.native.EXPORTS and hasattr(lib, name) and name + "(" in header
    assert lib.rr_abi_version() == 8 and "#define RR_ABI_VERSION 8" in header
    assert lib.rr_set_exr_depth(None, 32) == rr.native.RR_EINVAL  # NULL ctx
    assert lib.rr_set_exr_depth(None, 0) == rr.native.RR_EINVAL


def _scene_with(tmp_path, depth):
    with open(scene_path("04_very-simple-standin.rrscene")) as f:
        j = json.load(f)
    assert "exr_depth" not in j["render"]  # the committed scenes stay HALF
    if depth is not None:
        j["render"]["exr_depth"] = depth
    p = tmp_path / f"exr_depth{depth}.rrscene"
    p.write_text(json.dumps(j))
    return str(p)


def test_scene_exr_depth_parses(rr, tmp_path):
    for depth in (None, 16, 32):
        rr.Scene(_scene_with(tmp_path, depth)).close()
    for depth in (8, 0, 24, 16.5):
        with pytest.raises(rr.native.RRError) as e:
            rr.Scene(_scene_with(tmp_path, depth))
        assert e.value.code == rr.native.RR_EINVAL and "exr_depth" in str(e.value)


class _Ctx:
    """Stand-in for RenderContext: records what the runner asks for."""

    def __init__(self):
        self.calls = []

    def set_exr_depth(self, depth):
        self.calls.append(("exr_depth", depth))

    def set_png_depth(self, depth):
        self.calls.append(("depth", depth))

    def set_device_png(self, on):
        self.calls.append(("device_png", on))

    def load_scene(self, path):
        return types.SimpleNamespace(close=lambda: None)

    def render_frame(self, scene, f, params, out, fmt, q):
        self.calls.append((f, out, fmt))
        now = 0.0
        t = types.SimpleNamespace(loaded_at=now, started_rendering_at=now, finished_rendering_at=now,
                                  file_saving_started_at=now, file_saving_finished_at=now)
        return t, types.SimpleNamespace(spp=1)

    def close(self):
        pass


def test_runner_passes_the_exr_depth_through(rr, tmp_path):
    job = rr.BlenderJob.load_from_file(os.path.join(ROOT, "jobs", "04_very-simple_demo_10f-1w.toml"))
    job = rr.BlenderJob.from_dict({**job.to_dict(), "output_directory_path": str(tmp_path / "out"),
                                   "output_file_format": "OPEN_EXR"})
    ctx = _Ctx()
    runner = rr.BackendRunner(ROOT, ctx=ctx, exr_depth=32)
    runner.render_frame(job, 3)
    assert ctx.calls == [("exr_depth", 32), (3, str(tmp_path / "out" / "000003"), "OPEN_EXR")]
    ctx = _Ctx()
    rr.BackendRunner(ROOT, ctx=ctx)  # the default leaves the context's setting alone
    assert ctx.calls == []
    ctx = _Ctx()
    rr.BackendRunner(ROOT, ctx=ctx, exr_depth=0)
    assert ctx.calls == []


@pytest.mark.parametrize("blend", ["01_simple-animation/01_simple-animation.blend",
                                   "04_very-simple/04_very-simple-standin.blend"])
def test_exporter_writes_no_exr_depth_for_the_committed_projects(rr, blend):
    """The committed .blend projects do not carry R_IMF_CHAN_DEPTH_32: their
    exports have no exr_depth (16 is what its absence means), so they still
    equal the committed scenes."""
    import argparse
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import blend_export
    args = argparse.Namespace(samples=128, max_bounces=12, clamp_indirect=10.0, seed=0)
    out = blend_export.export(os.path.join(ROOT, "blender-projects", blend), args)
    assert "exr_depth" not in out["render"]
