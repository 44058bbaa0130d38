"""OPEN_EXR output, the parts that need no GPU: the strict reader of
tests/exr_reader.py round-trips its reference writer over the device encoder's
case list and rejects damaged files; the C ABI exports the debug entry without
an ABI bump; file naming and the runner accept the format."""
import os
import struct
import types
import zlib

import numpy as np
import pytest

import exr_reader as X
from conftest import ROOT


@pytest.mark.parametrize("w,h", X.SIZES + [(256, 64)])
def test_reader_round_trips_reference_writer(w, h):
    for kind in X.KINDS:
        px = X.expected_halfs(X.make_image(kind, w, h, seed=w * 7 + h))
        data = X.write_exr(px)
        back, header, sizes, modes = X.read_exr(data)
        assert np.array_equal(back, px), kind
        assert header["dataWindow"] == (0, 0, w - 1, h - 1)
        assert len(sizes) == (h + 15) // 16 and all(s <= 8 * w * min(16, h) for s in sizes)
        if kind == "flat" and w * h >= 512:
            assert set(modes) == {"zip"}
        if kind == "bits" and (w, h) == (256, 64):
            assert set(modes) == {"raw"}


def test_reader_round_trips_1080p():
    px = X.expected_halfs(X.make_image("grey", 1920, 1080, seed=1))
    back, _, sizes, _ = X.read_exr(X.write_exr(px))
    assert np.array_equal(back, px) and len(sizes) == 68


def test_preprocess_is_the_documented_transform():
    raw = bytes([1, 2, 3, 4, 5, 250])
    # even-indexed bytes 1 3 5, odd-indexed 2 4 250; differences + 128
    assert X.preprocess(raw) == bytes([1, 130, 130, (2 - 5 + 128) & 255, 130, (250 - 4 + 128) & 255])
    assert X.unprocess(X.preprocess(raw)) == raw


def _two_chunk_file():
    px = X.expected_halfs(X.make_image("gradient", 40, 20, seed=3))
    data = X.write_exr(px)
    _, _, sizes, modes = X.read_exr(data)
    assert modes == ["zip", "zip"]
    table = len(X.header_bytes(40, 20))
    return data, table, sizes


def test_reader_rejects_damaged_files():
    data, table, sizes = _two_chunk_file()
    with pytest.raises(X.ExrError):  # truncated
        X.read_exr(data[:-1])
    with pytest.raises(X.ExrError):
        X.read_exr(data[:table + 12])
    with pytest.raises(X.ExrError):  # bytes after the last chunk
        X.read_exr(data + b"\0")
    bad = bytearray(data)  # the second offset is off by one
    struct.pack_into("<Q", bad, table + 8, struct.unpack_from("<Q", data, table + 8)[0] + 1)
    with pytest.raises(X.ExrError, match="offset table"):
        X.read_exr(bytes(bad))
    bad = bytearray(data)  # the first chunk's Adler-32
    end = table + 16 + 8 + sizes[0]
    bad[end - 1] ^= 1
    with pytest.raises(X.ExrError, match="chunk 0"):
        X.read_exr(bytes(bad))
    bad = bytearray(data)  # the second chunk claims scanline 17
    struct.pack_into("<i", bad, end, 17)
    with pytest.raises(X.ExrError, match="scanline"):
        X.read_exr(bytes(bad))
    with pytest.raises(X.ExrError, match="magic"):
        X.read_exr(b"\x89PNG" + data[4:])
    with pytest.raises(X.ExrError, match="version"):
        X.read_exr(data[:4] + bytes([2, 2, 0, 0]) + data[8:])


def test_reader_requires_the_inflated_length():
    data, table, sizes = _two_chunk_file()
    at = table + 16
    short = zlib.compress(b"\0" * 100, 1)
    bad = data[:at] + struct.pack("<ii", 0, len(short)) + short
    rest = data[at + 8 + sizes[0]:]
    second = at + 8 + len(short)
    bad = bad[:table] + struct.pack("<QQ", at, second) + bad[table + 16:] + rest
    with pytest.raises(X.ExrError, match="inflates to 100"):
        X.read_exr(bad)


def test_debug_entry_exported_without_abi_bump(rr):
    assert "rr_debug_exr_device" in rr.native.EXPORTS
    lib = rr.native.lib()
    assert hasattr(lib, "rr_debug_exr_device")
    assert lib.rr_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "rr.h")).read()
    assert "rr_debug_exr_device(" in header and "#define RR_ABI_VERSION 8" in header


class _Ctx:
    """Stand-in for RenderContext: records what the runner asks for."""

    def __init__(self):
        self.calls = []

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


def test_naming_and_runner_accept_open_exr(rr, tmp_path):
    assert rr.naming.output_file_path("/out", "frame-####", 12, "OPEN_EXR") == "/out/frame-0012.exr"
    job = rr.BlenderJob.load_from_file(os.path.join(ROOT, "jobs", "04_very-simple_demo_10f-1w.toml"))
    job = rr.BlenderJob.from_dict({**job.to_dict(), "output_directory_path": str(tmp_path / "out"),
                                   "output_file_format": "OPEN_EXR"})
    assert all(p.endswith(".exr") for p in rr.naming.job_output_files(job, str(tmp_path / "out")))
    ctx = _Ctx()
    runner = rr.BackendRunner(ROOT, ctx=ctx)
    runner.render_frame(job, 3)
    assert ctx.calls == [(3, str(tmp_path / "out" / "000003"), "OPEN_EXR")]
    with pytest.raises(rr.runner.RenderError):
        bad = rr.BlenderJob.from_dict({**job.to_dict(), "output_file_format": "TIFF"})
        runner.render_frame(bad, 3)
