"""Several files from one rendered frame (rr_frame_submit_outputs), with reduced proxies.

A file of a multi-output frame is compared byte for byte with the file a single-output submit
of the same frame and settings writes, and a proxy with what rr_debug_encode_device makes of
the film reduced by tests/reduce.py. The film comes from the frame's own factor-1 OPEN_EXR
file with FLOAT channels, which holds the means sum * inv_spp bit for bit; the frames here
take 4 samples, so inv_spp is 0.25 and scaling commutes with the float32 sums of the
reduction: reduce(means) is reduce(sums) * inv_spp exactly."""
import json
import os
import subprocess

import numpy as np
import pytest

import exr32_reader as X32
import reduce as R
import tga as T
from conftest import scene_path

pytestmark = pytest.mark.gpu

S04 = scene_path("04_very-simple-standin.rrscene")
EXT = {"JPEG": ".jpg", "PNG": ".png", "OPEN_EXR": ".exr", "TARGA": ".tga", "TARGA_RAW": ".tga", "HDR": ".hdr",
       "IRIS": ".rgb", "WEBP": ".webp"}
WEBP_RANGE = "image size outside the WEBP format's range (16384 x 16384, a payload bound below 2 GB)"


@pytest.fixture(scope="module")
def mctx(rr):
    """A context of this module's own: its settings change here, and the frames-in-flight test
    compares it with a fresh one."""
    c = rr.RenderContext(0)
    yield c
    c.close()


@pytest.fixture
def octx(mctx):
    yield mctx
    mctx.set_device_png(False)
    mctx.set_exr_depth(0)
    mctx.set_exr_codec("")
    mctx.set_extra_outputs(None)


@pytest.fixture(scope="module")
def s04(mctx):
    s = mctx.load_scene(S04)
    yield s
    s.close()


def _params(rr, w=64, h=48, **kw):
    return rr.default_params(width=w, height=h, spp=4, **kw)


def _file(base, fmt):
    with open(str(base) + EXT[fmt], "rb") as f:
        return f.read()


def _single(ctx, scene, frame, p, d, name, fmt, quality=90, reduce=1):
    """The file of a single-output submit of the frame."""
    ctx.render_frame_outputs(scene, frame, p, [(d / name, fmt, quality, reduce)])
    return _file(d / name, fmt)


def _means(exr32_bytes):
    px, header, _, _ = X32.read_exr32(exr32_bytes)
    return px.view(np.float32)


def _dims(fmt, data):
    """(width, height) from the file's own header."""
    if fmt == "JPEG":
        at = data.index(b"\xff\xc0")
        return int.from_bytes(data[at + 7:at + 9], "big"), int.from_bytes(data[at + 5:at + 7], "big")
    if fmt == "WEBP":
        assert data[12:16] == b"VP8L" and data[20] == 0x2F
        bits = int.from_bytes(data[21:25], "little")
        return (bits & 0x3FFF) + 1, ((bits >> 14) & 0x3FFF) + 1
    if fmt == "HDR":
        line = data[:data.index(b"\n", data.index(b"\n\n") + 2)].split(b"\n")[-1].split()
        return int(line[3]), int(line[1])
    raise AssertionError(fmt)


def _expected_proxy(ctx, scene, frame, p, means, fmt, k, quality=90):
    """rr_debug_encode_device of the reduced film: through the view pass for an 8-bit format."""
    red = R.reduce(means, k)
    if fmt == "HDR":
        return ctx.encode_device("HDR", red)
    st = ctx.frame_state(scene, frame, p)
    img8 = ctx.view_device(red, int(st.render_ints[5]), float(st.render_floats[2]))
    return ctx.encode_device(fmt, img8, quality=quality)


# ---------------------------------------------------------------- identity ---
def test_outputs_at_factor_one_are_the_single_output_files(octx, rr, s04, tmp_path):
    octx.set_device_png(True)
    p = _params(rr)
    fmts = ["OPEN_EXR", "JPEG", "PNG", "TARGA"]
    _, st = octx.render_frame_outputs(s04, 30, p, [(tmp_path / f"m{i}", f, 90, 1) for i, f in enumerate(fmts)])
    for i, f in enumerate(fmts):
        data = _file(tmp_path / f"m{i}", f)
        assert data == _single(octx, s04, 30, p, tmp_path, f"s{i}", f), f
        octx.render_frame(s04, 30, p, str(tmp_path / f"r{i}"), f, 90)  # and rr_render_frame's
        assert data == _file(tmp_path / f"r{i}", f), f
    octx.render_frame_outputs(s04, 30, p, [(tmp_path / f"m{i}", f, 90, 1) for i, f in enumerate(fmts)])
    assert st.output_bytes == len(_file(tmp_path / "m0", "OPEN_EXR"))
    assert [octx.last_output_bytes(i) for i in range(4)] == [len(_file(tmp_path / f"m{i}", f)) for i, f in enumerate(fmts)]
    with pytest.raises(rr.RRError) as e:
        octx.last_output_bytes(4)
    assert e.value.code == rr.native.RR_EINVAL


def test_host_coded_png_is_an_output_at_any_factor(octx, rr, s04, tmp_path):
    """Without rr_set_device_png the 8-bit PNG comes from the host coder: the (reduced) 8-bit image
    goes back to the host for it."""
    from PIL import Image
    p = _params(rr, 67, 45)
    octx.render_frame_outputs(s04, 30, p, [(tmp_path / "a", "PNG", 90, 1), (tmp_path / "b", "PNG", 90, 4),
                                           (tmp_path / "c", "TARGA", 90, 4)])
    assert _file(tmp_path / "a", "PNG") == _single(octx, s04, 30, p, tmp_path, "sa", "PNG")
    assert _file(tmp_path / "b", "PNG") == _single(octx, s04, 30, p, tmp_path, "sb", "PNG", reduce=4)
    b = np.asarray(Image.open(tmp_path / "b.png").convert("RGBA"))
    c, _ = T.read((tmp_path / "c.tga").read_bytes())
    assert b.shape == (12, 17, 4) and np.array_equal(b, c)  # one reduced 8-bit image behind both


# ----------------------------------------------------------------- proxies ---
def test_proxies_are_the_coders_files_of_the_reduced_film(octx, rr, s04, tmp_path):
    octx.set_exr_depth(32)
    p = _params(rr, 67, 45)
    outs = [(tmp_path / "m", "OPEN_EXR", 90, 1), (tmp_path / "j", "JPEG", 90, 4), (tmp_path / "w", "WEBP", 100, 4),
            (tmp_path / "h", "HDR", 90, 4)]
    octx.render_frame_outputs(s04, 30, p, outs)
    assert octx.last_warning() == ""
    means = _means(_file(tmp_path / "m", "OPEN_EXR"))
    assert means.shape == (45, 67, 4) and float(means[..., :3].max()) > 0.0
    for base, fmt, q, k in outs[1:]:
        data = _file(base, fmt)
        assert _dims(fmt, data) == (17, 12), fmt
        assert data == _expected_proxy(octx, s04, 30, p, means, fmt, k, q), fmt


def test_split_path_film_is_what_the_coders_read(octx, rr, s04, tmp_path):
    octx.set_exr_depth(32)
    p = _params(rr, flags=rr.native.RR_FLAG_WAVEFRONT)
    _, st = octx.render_frame_outputs(s04, 30, p, [(tmp_path / "m", "OPEN_EXR", 90, 1), (tmp_path / "j", "JPEG", 90, 2)])
    assert st.tile_slices == 0  # not k_tiles
    means = _means(_file(tmp_path / "m", "OPEN_EXR"))
    data = _file(tmp_path / "j", "JPEG")
    assert _dims("JPEG", data) == (32, 24)
    assert data == _expected_proxy(octx, s04, 30, p, means, "JPEG", 2)
    assert _file(tmp_path / "m", "OPEN_EXR") == _single(octx, s04, 30, p, tmp_path, "sm", "OPEN_EXR")
    assert data == _single(octx, s04, 30, p, tmp_path, "sj", "JPEG", reduce=2)


# -------------------------------------------------------- frames in flight ---
def test_three_frames_in_flight_with_three_outputs_each(octx, rr, s04, tmp_path):
    octx.set_device_png(True)
    p = _params(rr)
    plan = {3: [("OPEN_EXR", 90, 1), ("JPEG", 90, 1), ("TARGA", 90, 1)],
            4: [("PNG", 90, 1), ("HDR", 90, 2), ("WEBP", 100, 1)],
            5: [("JPEG", 70, 4), ("IRIS", 90, 1), ("OPEN_EXR", 90, 2)]}
    tickets = [octx.submit_frame_outputs(s04, f, p, [(tmp_path / f"f{f}_{i}", fmt, q, k)
                                                     for i, (fmt, q, k) in enumerate(outs)])
               for f, outs in plan.items()]
    with pytest.raises(rr.RRError) as e:  # the fourth is one too many
        octx.submit_frame_outputs(s04, 6, p, [(tmp_path / "x", "JPEG", 90, 1)])
    assert e.value.code == rr.native.RR_EBUSY
    for t in tickets:
        octx.complete_frame(t)
    for f, outs in plan.items():
        for i, (fmt, q, k) in enumerate(outs):
            assert _file(tmp_path / f"f{f}_{i}", fmt) == _single(octx, s04, f, p, tmp_path, f"s{f}_{i}", fmt, q, k), (f, fmt)
    assert not (tmp_path / "x.jpg").exists()
    # nothing of those frames stays behind: a plain frame equals a fresh context's
    octx.set_device_png(False)
    octx.render_frame(s04, 7, p, str(tmp_path / "after"), "JPEG", 90)
    with rr.RenderContext(0) as fresh:
        s = fresh.load_scene(S04)
        try:
            fresh.render_frame(s, 7, p, str(tmp_path / "fresh"), "JPEG", 90)
        finally:
            s.close()
    assert _file(tmp_path / "after", "JPEG") == _file(tmp_path / "fresh", "JPEG")


def test_two_jpeg_outputs_of_different_quality(octx, rr, s04, tmp_path):
    """Accepted: the context keeps the transform's table of every quality."""
    p = _params(rr)
    octx.render_frame_outputs(s04, 30, p, [(tmp_path / "a", "JPEG", 90, 1), (tmp_path / "b", "JPEG", 50, 1),
                                           (tmp_path / "c", "JPEG", 90, 2), (tmp_path / "d", "JPEG", 50, 2)])
    a, b = _file(tmp_path / "a", "JPEG"), _file(tmp_path / "b", "JPEG")
    assert a != b and len(b) < len(a)
    assert a == _single(octx, s04, 30, p, tmp_path, "sa", "JPEG", 90)
    assert b == _single(octx, s04, 30, p, tmp_path, "sb", "JPEG", 50)
    assert _file(tmp_path / "c", "JPEG") == _single(octx, s04, 30, p, tmp_path, "sc", "JPEG", 90, 2)
    assert _file(tmp_path / "d", "JPEG") == _single(octx, s04, 30, p, tmp_path, "sd", "JPEG", 50, 2)


# ---------------------------------------------------------------- refusals ---
def test_refusals_come_before_any_file(octx, rr, s04, tmp_path):
    p = _params(rr)
    d = tmp_path / "out"
    d.mkdir()
    EINVAL, ENOTSUP = rr.native.RR_EINVAL, rr.native.RR_ENOTSUP

    def refused(outs, code, text, params=p):
        with pytest.raises(rr.RRError) as e:
            octx.render_frame_outputs(s04, 30, params, outs)
        assert e.value.code == code and text in str(e.value), (outs, str(e.value))

    ok = (d / "a", "JPEG", 90, 1)
    refused([], EINVAL, "1 .. 4 files, not 0")
    refused([(d / f"a{i}", "JPEG", 90, 1) for i in range(5)], EINVAL, "1 .. 4 files, not 5")
    for k in (0, 3, 16, -1):
        refused([ok, (d / "b", "PNG", 90, k)], EINVAL, "reduce must be 1, 2, 4 or 8")
    refused([ok, (d / "b", "PNG", 90, 1), (d / "a", "JPEG", 50, 2)], EINVAL, str(d / "a.jpg"))
    refused([(d / "t", "TARGA", 90, 1), (d / "t", "TARGA_RAW", 90, 1)], EINVAL, str(d / "t.tga"))
    with pytest.raises(rr.RRError) as single:
        octx.submit_frame(s04, 30, p, str(d / "a"), "TIFF", 90)
    assert single.value.code == ENOTSUP
    refused([ok, (d / "b", "TIFF", 90, 1)], ENOTSUP, str(single.value).split(": ", 1)[1])
    refused([ok, (d / "b", "JPEG", 0, 1)], EINVAL, "jpeg_quality must be 1..100")
    # a size outside a coder's range, judged at the reduced size: 16385 pixels are one too many for WEBP
    wide = rr.default_params(width=16385, height=8, spp=1)
    refused([(d / "m", "OPEN_EXR", 90, 1), (d / "w", "WEBP", 100, 1)], EINVAL, WEBP_RANGE, wide)
    # the context's extra outputs: a collision with the frame's own file
    octx.set_extra_outputs("JPEG:2,JPEG")
    with pytest.raises(rr.RRError) as e:
        octx.render_frame(s04, 30, p, str(d / "a"), "JPEG", 90)
    assert e.value.code == EINVAL and str(d / "a.jpg") in str(e.value)
    with pytest.raises(rr.RRError) as e:
        octx.set_extra_outputs("JPEG:3")
    assert e.value.code == EINVAL
    octx.set_extra_outputs(None)
    assert not list(d.iterdir())
    # a proxy brings the frame back into the coder's range
    octx.render_frame_outputs(s04, 30, wide, [(d / "m", "OPEN_EXR", 90, 1), (d / "w", "WEBP", 100, 2)])
    assert _dims("WEBP", _file(d / "w", "WEBP")) == (8193, 4)
    assert sorted(x.name for x in d.iterdir()) == ["m.exr", "w.webp"]


def test_warnings_are_joined_in_output_order(octx, rr, s04, tmp_path):
    octx.set_exr_codec("PIZ")
    p = _params(rr)
    octx.render_frame_outputs(s04, 30, p, [(tmp_path / "w", "WEBP", 80, 1), (tmp_path / "e", "OPEN_EXR", 90, 2)])
    w = octx.last_warning()
    a, b = w.find("WEBP at quality 80"), w.find("OPEN_EXR with codec PIZ")
    assert 0 <= a < b, w
    octx.render_frame_outputs(s04, 30, p, [(tmp_path / "e", "OPEN_EXR", 90, 1), (tmp_path / "w", "WEBP", 80, 1)])
    w = octx.last_warning()
    assert 0 <= w.find("OPEN_EXR with codec PIZ") < w.find("WEBP at quality 80"), w
    octx.render_frame_outputs(s04, 30, p, [(tmp_path / "j", "JPEG", 90, 1)])
    assert octx.last_warning() == ""


# ------------------------------------------ without new code in the caller ---
def test_extra_outputs_of_the_context(octx, rr, s04, tmp_path):
    p = _params(rr)
    octx.set_extra_outputs("JPEG:4,TARGA")
    octx.render_frame(s04, 30, p, str(tmp_path / "f"), "OPEN_EXR", 85)
    assert sorted(x.name for x in tmp_path.iterdir()) == ["f.exr", "f.r4.jpg", "f.tga"]
    octx.render_frame(s04, 30, p, None, None)  # a frame without a path writes nothing
    octx.set_extra_outputs("")
    assert _file(tmp_path / "f", "OPEN_EXR") == _single(octx, s04, 30, p, tmp_path, "s", "OPEN_EXR")
    assert (tmp_path / "f.r4.jpg").read_bytes() == _single(octx, s04, 30, p, tmp_path, "sj", "JPEG", 85, 4)
    assert _file(tmp_path / "f", "TARGA") == _single(octx, s04, 30, p, tmp_path, "st", "TARGA")


def test_shim_writes_the_extra_outputs_of_the_environment(rr, tmp_path):
    base = {k: v for k, v in os.environ.items() if k != "RR_EXTRA_OUTPUTS"}
    base.update(RR_WIDTH="64", RR_HEIGHT="48", RR_SPP="4")
    files = {}
    for name, extra in (("plain", None), ("extra", "JPEG:2")):
        d = tmp_path / name
        d.mkdir()
        argv = [rr.SHIM_PATH, S04.replace(".rrscene", ".blend"), "--background", "--python", "script.py", "--",
                "--render-output", str(d / "######"), "--render-format", "OPEN_EXR", "--render-frame", "12"]
        env = dict(base, RR_EXTRA_OUTPUTS=extra) if extra else base
        res = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=120)
        assert res.returncode == 0, res.stdout + res.stderr
        assert f"Saved: '{d}/000012.exr'" in res.stdout
        files[name] = {x.name: x.read_bytes() for x in d.iterdir()}
    assert sorted(files["plain"]) == ["000012.exr"]
    assert sorted(files["extra"]) == ["000012.exr", "000012.r2.jpg"]
    assert files["extra"]["000012.exr"] == files["plain"]["000012.exr"]
    assert _dims("JPEG", files["extra"]["000012.r2.jpg"]) == (32, 24)
    bad = subprocess.run([rr.SHIM_PATH, S04, "--", "--render-output", str(tmp_path / "#"), "--render-format", "JPEG",
                          "--render-frame", "1"], capture_output=True, text=True, env=dict(base, RR_EXTRA_OUTPUTS="JPEG:3"),
                         timeout=60)
    assert bad.returncode != 0 and "RR_EXTRA_OUTPUTS='JPEG:3'" in bad.stdout


def test_use_preview_of_the_scene(octx, rr, tmp_path):
    doc = json.load(open(S04))
    p = _params(rr)
    for name, preview in (("with", True), ("without", None)):
        d = tmp_path / name
        d.mkdir()
        if preview is not None:
            doc["render"]["use_preview"] = preview
        else:
            doc["render"].pop("use_preview", None)
        path = tmp_path / (name + ".rrscene")
        path.write_text(json.dumps(doc))
        s = octx.load_scene(str(path))
        try:
            octx.render_frame(s, 30, p, str(d / "f"), "OPEN_EXR", 90)
            octx.render_frame(s, 30, p, str(d / "g"), "PNG", 90)  # only OPEN_EXR frames have a preview
            if preview:
                assert (d / "f.jpg").read_bytes() == _single(octx, s, 30, p, d, "s", "JPEG", 90)
                os.remove(d / "s.jpg")
                octx.set_extra_outputs("TARGA")  # the context's own extra outputs come instead
                octx.render_frame(s, 30, p, str(d / "h"), "OPEN_EXR", 90)
                octx.set_extra_outputs(None)
        finally:
            s.close()
    assert sorted(x.name for x in (tmp_path / "with").iterdir()) == ["f.exr", "f.jpg", "g.png", "h.exr", "h.tga"]
    assert sorted(x.name for x in (tmp_path / "without").iterdir()) == ["f.exr", "g.png"]
