"""Colour modes (rr_set_color_mode), the parts that need no GPU: scenes carry
render.color_mode; the values of the setter; the exporter's --color-mode; the
grey rule on every code; the host encoders' BW / RGB / RGBA files; the readers
of tests/color_modes.py reject what they should."""
import argparse
import ctypes
import io
import json
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

import color_modes as M
import png16_reader as P
from conftest import ROOT, scene_path

S01 = scene_path("01_simple-animation.rrscene")
S04 = scene_path("04_very-simple-standin.rrscene")
BLENDS = {S01: os.path.join(ROOT, "blender-projects", "01_simple-animation", "01_simple-animation.blend"),
          S04: os.path.join(ROOT, "blender-projects", "04_very-simple", "04_very-simple-standin.blend")}


def _scene_with(tmp_path, name, **render):
    with open(S04) as f:
        j = json.load(f)
    j["render"].update(render)
    p = tmp_path / name
    p.write_text(json.dumps(j))
    return str(p)


# ------------------------------------------------------------ the setting --
@pytest.mark.parametrize("mode", ["BW", "RGB", "RGBA"])
def test_scene_field_is_accepted(rr, tmp_path, mode):
    rr.Scene(_scene_with(tmp_path, "s.rrscene", color_mode=mode)).close()


@pytest.mark.parametrize("bad", ["bw", "GREY", "", "RGBAA", 3, None])
def test_scene_field_is_rejected(rr, tmp_path, bad):
    with pytest.raises(rr.RRError) as e:
        rr.Scene(_scene_with(tmp_path, "s.rrscene", color_mode=bad))
    assert "color_mode" in str(e.value)


def test_committed_scenes_carry_no_field():
    for s in (S01, S04):
        with open(s) as f:
            assert "color_mode" not in json.load(f)["render"]


def test_values_and_exports(rr):
    n = rr.native
    assert (n.RR_COLOR_SCENE, n.RR_COLOR_BW, n.RR_COLOR_RGB, n.RR_COLOR_RGBA) == (0, 1, 3, 4)
    assert (M.BW, M.RGB, M.RGBA) == (n.RR_COLOR_BW, n.RR_COLOR_RGB, n.RR_COLOR_RGBA)
    with open(os.path.join(ROOT, "include", "rr.h")) as f:
        header = f.read()
    for name, v in (("SCENE", 0), ("BW", 1), ("RGB", 3), ("RGBA", 4)):
        assert re.search(rf"#define RR_COLOR_{name} {v}\b", header), name
    for sym in ("rr_set_color_mode", "rr_encode_image_mode", "rr_debug_encode_device"):
        assert sym in n.EXPORTS and hasattr(rr.lib(), sym)
    assert rr.lib().rr_abi_version() == n.RR_ABI_VERSION
    assert [n.color_mode_value(m) for m in ("", None, 0, "BW", "RGB", "RGBA", 4)] == [0, 0, 0, 1, 3, 4, 4]
    with pytest.raises(ValueError):
        n.color_mode_value("GREY")
    # NULL ctx: RR_EINVAL, with a valid and with an invalid value
    assert rr.lib().rr_set_color_mode(None, 1) == n.RR_EINVAL
    assert rr.lib().rr_set_color_mode(None, 2) == n.RR_EINVAL


class _Ctx:
    def __init__(self):
        self.calls = []

    def set_color_mode(self, mode):
        self.calls.append(("color_mode", mode))


def test_runner_passes_the_mode_through(rr):
    c = _Ctx()
    rr.BackendRunner(ROOT, ctx=c, color_mode="BW")
    assert c.calls == [("color_mode", "BW")]
    c = _Ctx()
    rr.BackendRunner(ROOT, ctx=c)
    assert c.calls == []


# --------------------------------------------------------------- exporter --
def _export(blend, **kw):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from blend_export import export
    args = argparse.Namespace(samples=128, max_bounces=12, clamp_indirect=10.0, seed=0, **kw)
    return json.loads(json.dumps(export(blend, args)))


def test_exporter_keep_and_project():
    with open(S01) as f:
        committed = json.load(f)
    assert _export(BLENDS[S01]) == committed  # no attribute: keep
    assert _export(BLENDS[S01], color_mode="keep") == committed
    for s, blend in BLENDS.items():
        assert "color_mode" not in _export(blend, color_mode="keep")["render"]
        proj = _export(blend, color_mode="project")
        assert proj["render"]["color_mode"] == "RGB"  # ImageFormatData.planes = 24 in both projects
        del proj["render"]["color_mode"]
        assert proj == _export(blend, color_mode="keep")


def test_exported_field_loads(rr, tmp_path):
    proj = _export(BLENDS[S01], color_mode="project")
    p = tmp_path / "p.rrscene"
    p.write_text(json.dumps(proj))
    rr.Scene(str(p)).close()


# ---------------------------------------------------------- the grey rule --
def test_grey8_is_the_identity_on_greys():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(M.grey8(np.stack([v, v, v], -1)), v)


def test_grey8_primaries_and_weights():
    px = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 0, 0], [255, 255, 255]], np.uint8)
    # 255 * 0.2126 = 54.2, 255 * 0.7152 = 182.4, 255 * 0.0722 = 18.4, 255 * 0.9278 = 236.6
    assert list(M.grey8(px)) == [54, 182, 18, 237, 0, 255]


def test_grey16_on_every_code_and_the_primaries():
    """r = g = b = k / 65535 quantises to k or a neighbour: the float32 sum of
    the three rounded products is within two ulps of the value (2^-22 near 1,
    a quarter of the half code quantize16 rounds over), so it moves a code
    only next to a rounding tie, and by one. Monotone over all 65,536 codes."""
    k = np.arange(65536)
    v = (k / 65535.0).astype(np.float32)
    q = P.quantize16(M.luma(v, v, v)).astype(np.int64)
    assert np.max(np.abs(q - P.quantize16(v).astype(np.int64))) <= 1
    assert q[0] == 0 and q[65535] >= 65534 and np.all(np.diff(q) >= 0)
    one, zero = np.float32(1), np.float32(0)
    prim = [int(P.quantize16(M.luma(*c))) for c in ((one, zero, zero), (zero, one, zero), (zero, zero, one))]
    assert prim == [13933, 46871, 4732]  # round(65535 * w)
    assert int(P.quantize16(M.luma(one, one, one))) in (65534, 65535)


# -------------------------------------------------------- host PNG files --
@pytest.mark.parametrize("mode,pil,c", [("BW", "L", 1), ("RGB", "RGB", 3), ("RGBA", "RGBA", 4), (0, "RGBA", 4)])
@pytest.mark.parametrize("w,h", [(1, 1), (3, 17), (67, 45)])
def test_host_png_modes(rr, tmp_path, mode, pil, c, w, h):
    for kind in M.KINDS:
        img = M.rgba8_image(kind, w, h, seed=w + h)
        n = rr.encode_image_mode(img, str(tmp_path / "f"), "PNG", 90, mode)
        data = (tmp_path / "f.png").read_bytes()
        assert len(data) == n
        px, info = M.read_png(data)
        want = M.expected_png8(img, c)
        assert info["depth"] == 8 and info["colour_type"] == M.COLOUR_TYPE[c]
        assert np.array_equal(px, want), kind
        im = Image.open(io.BytesIO(data))
        assert im.mode == pil and im.size == (w, h)
        assert np.array_equal(np.asarray(im).reshape(h, w, c), want)


def test_mode_zero_is_rr_encode_image(rr, tmp_path):
    img = M.rgba8_image("gradient", 67, 45)
    for fmt, ext, modes in (("PNG", ".png", (0, "RGBA")), ("JPEG", ".jpg", (0, "RGB", "RGBA"))):
        rr.encode_image(img, str(tmp_path / "a"), fmt, 90)
        for m in modes:
            rr.encode_image_mode(img, str(tmp_path / "b"), fmt, 90, m)
            assert (tmp_path / ("a" + ext)).read_bytes() == (tmp_path / ("b" + ext)).read_bytes(), (fmt, m)
    with pytest.raises(rr.RRError) as e:
        rr.encode_image_mode(img, str(tmp_path / "c"), "PNG", 90, 2)
    assert e.value.code == rr.native.RR_EINVAL


# ------------------------------------------------------- host JPEG files --


def _jpeg_structure(data):
    """Marker segments in front of the scan: [(marker, body)]."""
    assert data[:2] == b"\xff\xd8"
    at, out = 2, []
    while True:
        assert data[at] == 0xFF
        m = data[at + 1]
        n, = struct.unpack_from(">H", data, at + 2)
        out.append((m, data[at + 4:at + 2 + n]))
        at += 2 + n
        if m == 0xDA:
            return out, data[at:]


@pytest.mark.parametrize("w,h", [(1, 1), (7, 9), (8, 8), (17, 33), (250, 141)])
def test_host_jpeg_bw_structure(rr, tmp_path, w, h):
    img = M.smooth_image(w, h)
    rr.encode_image_mode(img, str(tmp_path / "f"), "JPEG", 90, "BW")
    data = (tmp_path / "f.jpg").read_bytes()
    segs, scan = _jpeg_structure(data)
    assert [m for m, _ in segs] == [0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xDD, 0xDA]
    sof = segs[2][1]
    assert sof == struct.pack(">BHHB", 8, h, w, 1) + bytes([1, 0x11, 0])
    assert segs[1][1][0] == 0 and [s[1][0] for s in segs[3:5]] == [0x00, 0x10]  # luma DQT, luma DC + AC DHT
    assert segs[5][1] == struct.pack(">H", (w + 7) // 8)  # one restart interval an MCU row
    assert segs[6][1] == bytes([1, 1, 0x00, 0, 63, 0])
    rst = re.findall(rb"\xff[\xd0-\xd7]", scan)
    rows = (h + 7) // 8
    assert [r[1] for r in rst] == [0xD0 + (k & 7) for k in range(rows - 1)] and scan[-2:] == b"\xff\xd9"
    im = Image.open(io.BytesIO(data))
    assert im.format == "JPEG" and im.mode == "L" and im.size == (w, h)
    im.load()


def _shortfalls(rr, img, tmp_path):
    """(host BW PSNR, PIL L PSNR, host RGB PSNR, PIL RGB PSNR) at quality 90.
    PIL's RGB encode with 4:2:0 subsampling, as the host encoder's."""
    grey = M.grey8(img)
    rr.encode_image_mode(img, str(tmp_path / "g"), "JPEG", 90, "BW")
    rr.encode_image_mode(img, str(tmp_path / "c"), "JPEG", 90, "RGB")
    ours_l = np.asarray(Image.open(tmp_path / "g.jpg"))
    ours_c = np.asarray(Image.open(tmp_path / "c.jpg").convert("RGB"))
    b = io.BytesIO()
    Image.fromarray(grey, "L").save(b, "JPEG", quality=90)
    pil_l = np.asarray(Image.open(io.BytesIO(b.getvalue())))
    b = io.BytesIO()
    Image.fromarray(img[..., :3].copy(), "RGB").save(b, "JPEG", quality=90, subsampling=2)
    pil_c = np.asarray(Image.open(io.BytesIO(b.getvalue())).convert("RGB"))
    return M.psnr(ours_l, grey), M.psnr(pil_l, grey), M.psnr(ours_c, img[..., :3]), M.psnr(pil_c, img[..., :3])


def test_host_jpeg_bw_fidelity(rr, tmp_path):
    """Every kind is above the 35 dB floor of test_jpeg_encoder_quality90, and on
    no kind is the BW file further below PIL's own L encode at quality 90 than
    the three-component encoder strays from PIL's RGB encode.

    The reading, as a decision: "the three-component encoder's shortfall on the
    same image kinds" is taken as one figure, the largest |PIL RGB - host RGB|
    over the kinds, and every kind's BW shortfall is held against it. The two
    host encoders share fdct_quant, and both differ from libjpeg by the
    rounding of single coefficients (float DCT and a multiply by 1/q here, an
    integer DCT and a division there), which moves a file's PSNR by hundredths
    of a dB in either direction: the three-component figures below go from
    -0.057 to +0.015. That spread is the noise of the comparison itself,
    measured on the encoder that was there before, not on the one under test;
    a bound tighter than it would test the libjpeg build.
    Measured (dB; BW, PIL L | RGB, PIL RGB), 250x141:
      smooth   53.573 53.579 | 45.569 45.512
      flat     99     99     | 52.902 52.902
      grey     36.417 36.427 | 36.419 36.427
      gradient 51.928 51.916 | 34.676 34.692
      noise    36.337 36.337 | 12.657 12.655
    largest BW shortfall 0.010 (grey); three-component |difference| 0.057."""
    short_l, diff_c = {}, {}
    for kind in ["smooth"] + M.KINDS:
        img = M.smooth_image(250, 141) if kind == "smooth" else M.rgba8_image(kind, 250, 141)
        ours_l, pil_l, ours_c, pil_c = _shortfalls(rr, img, tmp_path)
        print(f"{kind}: BW {ours_l:.3f} dB (PIL L {pil_l:.3f}), RGB {ours_c:.3f} dB (PIL RGB {pil_c:.3f})")
        assert ours_l > 35.0, kind
        short_l[kind] = pil_l - ours_l
        diff_c[kind] = abs(pil_c - ours_c)
    noise = max(diff_c.values())
    print(f"largest BW shortfall {max(short_l.values()):.4f} dB, three-component |difference| {noise:.4f} dB")
    for kind, s in short_l.items():
        assert s <= noise, (kind, s, noise)


# -------------------------------------------------------------- readers ---
def test_png_reader_rejects_damage():
    img = np.arange(3 * 5 * 1, dtype=np.uint8).reshape(3, 5, 1)
    raw = M.png_front_bytes(img, 8)

    def png(colour, depth, body, w=5, h=3):
        return P.SIGNATURE + P._chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, 0)) + \
            P._chunk(b"IDAT", body) + P._chunk(b"IEND", b"")

    good = png(0, 8, zlib.compress(raw, 1))
    px, info = M.read_png(good)
    assert np.array_equal(px, img) and info["channels"] == 1
    for bad in (png(2, 8, zlib.compress(raw, 1)), png(0, 16, zlib.compress(raw, 1)), png(3, 8, zlib.compress(raw, 1)),
                png(0, 8, zlib.compress(raw, 1) + b"\0"), png(0, 8, zlib.compress(raw + b"\0", 1)),
                png(0, 8, zlib.compress(raw, 1)[:-1] + b"\0"), good[:-1], good + b"\0"):
        with pytest.raises(M.FormatError):
            M.read_png(bad)
    for c, depth in ((3, 8), (4, 8), (1, 16), (3, 16), (4, 16)):
        s = (np.arange(4 * 7 * c).reshape(4, 7, c) * 2621 % (1 << depth)).astype(np.uint16 if depth == 16 else np.uint8)
        back, info = M.read_png(png(M.COLOUR_TYPE[c], depth, zlib.compress(M.png_front_bytes(s, depth), 1), 7, 4))
        assert np.array_equal(back, s) and back.dtype == s.dtype


def test_exr_restatement_shapes():
    img = M.float_image("noise", 5, 3, seed=2)
    for c in (1, 3, 4):
        assert M.expected_exr(img, c, True).shape == (3, 5, c) and M.expected_exr(img, c, True).dtype == np.uint32
        assert M.expected_exr(img, c, False).dtype == np.uint16
    assert np.all(M.expected_exr(img, 4, True)[..., 0] == 0x3F800000)
    assert np.array_equal(M.exr_means(img, 3)[..., ::-1], img[..., :3])
