"""16-bit PNG output, the parts that need no GPU: the strict reader of
tests/png16_reader.py round-trips its reference writer (all five filter types)
and rejects damaged files; PIL opens what the writer makes; the front end's
restatement follows its rounding rules; the C ABI exports the new entries
without an ABI bump; scenes carry render.color_depth; the runner passes the
depth on."""
import io
import json
import os
import struct
import types
import zlib

import numpy as np
import pytest
from PIL import Image

import png16_reader as P
from conftest import ROOT, scene_path


def _pixels(kind, w, h, view=1):
    return P.front_end(P.make_image(kind, w, h, seed=w * 7 + h), 1)


@pytest.mark.parametrize("w,h", P.SIZES[:-1] + [(40, 20)])
def test_reader_round_trips_reference_writer(w, h):
    for kind in P.KINDS:
        px = _pixels(kind, w, h)
        assert px.dtype == np.uint16 and px.shape == (h, w, 4) and np.all(px[..., 3] == 65535)
        data = P.write_png16(px)
        back, info = P.read_png16(data)
        assert np.array_equal(back, px), kind
        assert (info["width"], info["height"]) == (w, h) and np.all(info["filters"] == 1)
        assert info["raw"] == P.filtered_bytes(px)
        im = Image.open(io.BytesIO(data))  # a third-party reader takes the file
        assert im.size == (w, h) and im.mode == "RGBA", (im.size, im.mode)
        im.load()


def test_reader_round_trips_wide_and_large():
    px = _pixels("ramp", 4096, 17)
    assert len(np.unique(px[..., :3])) == 65536  # the ramp holds every 16-bit code
    back, _ = P.read_png16(P.write_png16(px))
    assert np.array_equal(back, px)
    px = P.front_end(P.make_image("flat", 1920, 1080), 1)
    back, _ = P.read_png16(P.write_png16(px))
    assert np.array_equal(back, px)


def test_reader_undoes_all_five_filters():
    px = _pixels("noise", 37, 11)
    kinds = [0, 1, 2, 3, 4, 4, 3, 2, 1, 0, 4]
    data = P.write_png16(px, types=kinds)
    back, info = P.read_png16(data)
    assert list(info["filters"]) == kinds and np.array_equal(back, px)
    im = Image.open(io.BytesIO(data))
    assert im.size == (37, 11) and im.mode == "RGBA"
    # PIL reduces 16-bit RGBA to 8 bits on load: it vouches for the top byte only
    top = np.asarray(im.convert("RGBA"))
    assert np.max(np.abs(top.astype(int) - (px >> 8).astype(int))) <= 1


def test_sub_filter_is_the_documented_transform():
    px = np.array([[[0x0102, 0x0304, 0x0506, 0xFFFF], [0x0103, 0x0300, 0x0606, 0xFFFF]]], np.uint16)
    want = bytes([1, 1, 2, 3, 4, 5, 6, 255, 255, 0, 1, 0, 252, 1, 0, 0, 0])
    assert P.filtered_bytes(px) == want
    img, kinds = P.unfilter(want, 2, 1)
    assert list(kinds) == [1] and img.tobytes() == P.image_bytes(px).tobytes()


def test_reader_rejects_damaged_files():
    px = _pixels("gradient", 40, 20)
    data = P.write_png16(px)
    P.read_png16(data)
    for cut in (1, 4, 12, 13, len(data) - 8, len(data) - 40):
        with pytest.raises(P.Png16Error):  # truncated
            P.read_png16(data[:-cut])
    with pytest.raises(P.Png16Error, match="after IEND"):
        P.read_png16(data + b"\0")
    with pytest.raises(P.Png16Error, match="signature"):
        P.read_png16(b"\x88" + data[1:])
    bad = bytearray(data)
    bad[8 + 8 + 8] = 8  # bit depth 8, CRC left alone
    with pytest.raises(P.Png16Error, match="CRC"):
        P.read_png16(bytes(bad))
    raw = P.filtered_bytes(px)

    def with_idat(z, depth=16, colour=6, lace=0):
        h, w = px.shape[:2]
        return P.SIGNATURE + P._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, lace)) + \
            P._chunk(b"IDAT", z) + P._chunk(b"IEND", b"")

    P.read_png16(with_idat(zlib.compress(raw, 1)))
    for kw in ({"depth": 8}, {"colour": 2}, {"lace": 1}):
        with pytest.raises(P.Png16Error, match="IHDR"):
            P.read_png16(with_idat(zlib.compress(raw, 1), **kw))
    z = zlib.compress(raw, 1)
    with pytest.raises(P.Png16Error, match="zlib"):  # Adler-32
        P.read_png16(with_idat(z[:-1] + bytes([z[-1] ^ 1])))
    with pytest.raises(P.Png16Error, match="truncated"):
        P.read_png16(with_idat(z[:-5]))
    with pytest.raises(P.Png16Error, match="after the zlib stream"):
        P.read_png16(with_idat(z + b"\0"))
    with pytest.raises(P.Png16Error, match="inflates to"):
        P.read_png16(with_idat(zlib.compress(raw[:-1], 1)))
    with pytest.raises(P.Png16Error, match="filter type"):
        P.read_png16(with_idat(zlib.compress(bytes([5]) + raw[1:], 1)))
    two = P.SIGNATURE + P._chunk(b"IHDR", struct.pack(">IIBBBBB", 40, 20, 16, 6, 0, 0, 0)) + \
        P._chunk(b"IDAT", z[:100]) + P._chunk(b"IDAT", z[100:]) + P._chunk(b"IEND", b"")
    with pytest.raises(P.Png16Error, match="chunks"):  # the renderer writes one IDAT
        P.read_png16(two)


def test_quantize16_rule():
    v = np.array([-1.0, -0.0, 0.0, 1e-9, 0.5 / 65535 * 0.99, 0.5 / 65535 * 1.01, 0.5, 1.0 - 2 ** -24, 1.0, 7.0],
                 np.float32)
    assert list(P.quantize16(v)) == [0, 0, 0, 0, 0, 1, 32768, 65535, 65535, 65535]
    k = np.arange(65536)
    assert np.array_equal(P.quantize16((k / 65535.0).astype(np.float32)), k)


def test_new_entries_exported_without_abi_bump(rr):
    lib = rr.native.lib()
    header = open(os.path.join(ROOT, "include", "rr.h")).read()
    for name in ("rr_set_png_depth", "rr_debug_png16_device", "rr_debug_srgb16_table"):
        assert name in rr.native.EXPORTS and hasattr(lib, name) and name + "(" in header
    assert lib.rr_abi_version() == 8 and "#define RR_ABI_VERSION 8" in header
    assert "render-timing-script.py:83-92" in header.split("rr_set_png_depth(")[0].rsplit("/*", 1)[1]
    assert lib.rr_set_png_depth(None, 16) == rr.native.RR_EINVAL  # NULL ctx


def test_srgb16_table_and_its_read(rr):
    t = rr.native.srgb16_table()
    n = len(t) - 1
    assert t.dtype == np.float32 and n & (n - 1) == 0 and n >= 16384
    want = (1.055 * (np.arange(n + 1) / n) ** (1 / 2.4) - 0.055).astype(np.float32)
    assert np.max(np.abs(t - want)) <= 2 ** -23 and t[n] == 1.0  # pow implementations may differ in the last bit
    # over a ramp of every multiple of 2^-12 and the knee's neighbourhood: within
    # one code of the exact curve rounded, and monotone
    x = np.unique(np.concatenate([np.arange(4097) / 4096.0, np.linspace(0.003, 0.0033, 3001)])).astype(np.float32)
    q = P.quantize16(P.srgb_oetf16(x, t)).astype(int)
    xd = x.astype(np.float64)
    exact = np.where(xd <= 0.0031308, 12.92 * xd, 1.055 * xd ** (1 / 2.4) - 0.055)
    assert np.max(np.abs(q - np.rint(65535 * exact))) <= 1 and np.all(np.diff(q) >= 0)
    assert q[0] == 0 and q[-1] == 65535


def _scene_with(tmp_path, depth):
    with open(scene_path("04_very-simple-standin.rrscene")) as f:
        j = json.load(f)
    assert "color_depth" not in j["render"]  # the committed scenes stay at 8
    if depth is not None:
        j["render"]["color_depth"] = depth
    p = tmp_path / f"depth{depth}.rrscene"
    p.write_text(json.dumps(j))
    return str(p)


def test_scene_color_depth_parses(rr, tmp_path):
    for depth in (None, 8, 16):
        rr.Scene(_scene_with(tmp_path, depth)).close()
    for depth in (12, 0, 32, 16.5):
        with pytest.raises(rr.native.RRError) as e:
            rr.Scene(_scene_with(tmp_path, depth))
        assert e.value.code == rr.native.RR_EINVAL and "color_depth" in str(e.value)


class _Ctx:
    """Stand-in for RenderContext: records what the runner asks for."""

    def __init__(self):
        self.calls = []

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


def test_runner_passes_the_depth_through(rr, tmp_path):
    job = rr.BlenderJob.load_from_file(os.path.join(ROOT, "jobs", "04_very-simple_demo_10f-1w.toml"))
    job = rr.BlenderJob.from_dict({**job.to_dict(), "output_directory_path": str(tmp_path / "out"),
                                   "output_file_format": "PNG"})
    ctx = _Ctx()
    runner = rr.BackendRunner(ROOT, ctx=ctx, png_depth=16)
    runner.render_frame(job, 3)
    assert ctx.calls == [("depth", 16), (3, str(tmp_path / "out" / "000003"), "PNG")]
    ctx = _Ctx()
    rr.BackendRunner(ROOT, ctx=ctx)  # the default leaves the context's setting alone
    assert ctx.calls == []


def test_exporter_writes_color_depth_only_when_16(rr):
    """The committed .blend projects are 8-bit PNG: their exports carry no
    color_depth (8 is what its absence means), so they still equal the
    committed scenes; the exporter reads ImageFormatData.depth."""
    import argparse
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import blend_export
    args = argparse.Namespace(samples=128, max_bounces=12, clamp_indirect=10.0, seed=0)
    out = blend_export.export(os.path.join(ROOT, "blender-projects", "04_very-simple",
                                           "04_very-simple-standin.blend"), args)
    assert "color_depth" not in out["render"]
