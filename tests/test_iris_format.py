"""IRIS (Silicon Graphics .rgb, run-length coded), the parts that need no GPU: the
host coder's files equal the restatement of tests/iris.py byte for byte, pass
its strict reader, and decode, by that reader and by PIL (which reads run-length
coded SGI files and writes none, so it is a reader of its own), to the image;
the size bound; the refusals; naming and the runner; the reader rejects what it
should; the stand-alone check program under the sanitizers."""
import ctypes
import io
import os
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest
from PIL import Image

import iris as I
from conftest import PKG, ROOT

MODES = {"BW": 1, "RGB": 3, "RGBA": 4}
IMAGES = I.images()


def _host_file(rr, tmp_path, img, mode):
    n = rr.encode_image_mode(img, str(tmp_path / "f"), "IRIS", 90, mode)
    data = (tmp_path / "f.rgb").read_bytes()
    assert n == len(data)
    return data


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} samples differ, first at {bad[0]}"


def test_images_are_the_named_ones():
    """Every size in every kind, and the kinds are what their names say."""
    assert len(I.SIZES) == 17 and (300, 17) in I.SIZES and (5, 1100) in I.SIZES
    for w, h in I.SIZES:
        for kind in ("random", "constant", "two values", "runs of 3", "runs of 2", "odd one out"):
            assert IMAGES[f"{kind} {w}x{h}"].shape == (h, w, 4), (kind, w, h)
    for n in (2, 3):
        for c in (1, 3, 4):
            planes = I.file_planes(IMAGES[f"runs of {n} 300x17"], c)
            for p in planes.reshape(-1, 300):
                lens = np.diff(np.concatenate([[0], np.flatnonzero(p[1:] != p[:-1]) + 1, [300]]))
                assert set(lens[1:-1].tolist()) == {n} and lens[0] <= n and lens[-1] <= n
    planes = I.file_planes(IMAGES["odd one out 257x6"], 1).reshape(-1, 257)
    assert sorted(int(np.flatnonzero(p != p[0])[0]) for p in planes) == sorted(I.ODD_AT)
    assert all(np.count_nonzero(p != p[0]) == 1 for p in planes)
    for c in (3, 4):  # two rows of three channels take the six places
        planes = I.file_planes(IMAGES["odd one out by channel 257x2"], c)[:, :3].reshape(-1, 257)
        assert sorted(int(np.flatnonzero(p != p[0])[0]) for p in planes) == sorted(I.ODD_AT)


@pytest.mark.parametrize("mode", ["BW", "RGB", "RGBA"])
def test_host_files(rr, tmp_path, mode):
    c = MODES[mode]
    for name, img in IMAGES.items():
        h, w = img.shape[:2]
        data = _host_file(rr, tmp_path, img, mode)
        assert data == I.encode(img, c), (name, "host file differs from the restatement")
        px, info = I.read(data)
        assert (info["channels"], info["width"], info["height"]) == (c, w, h), name
        want = I.expected(img, c)
        _same(px, want, name)
        # the bound the stream's buffers are sized by: a condition, not a measurement
        assert info["body"] <= I.body_bound(w, h, c) and max(info["length"]) <= I.plane_bound(w), name
        im = Image.open(io.BytesIO(data))
        assert im.format == "SGI" and im.mode == I.PIL_MODE[c] and im.size == (w, h), name
        _same(np.asarray(im).reshape(h, w, c), want, ("PIL", name))


def test_mode_0_is_rgba(rr, tmp_path):
    img = IMAGES["two values 300x17"]
    assert _host_file(rr, tmp_path, img, 0) == _host_file(rr, tmp_path, img, "RGBA")
    rr.encode_image(img, str(tmp_path / "g"), "IRIS")
    assert (tmp_path / "g.rgb").read_bytes() == I.encode(img, 4)
    assert not np.all(img[..., 3] == 255)  # alpha is the image's own


def test_header_and_tables(rr, tmp_path):
    img = IMAGES["random 65x3"]
    for mode, c in MODES.items():
        data = _host_file(rr, tmp_path, img, mode)
        want = bytes([0x01, 0xDA, 1, 1, 0, 2 if c == 1 else 3, 0, 65, 0, 3, 0, c, 0, 0, 0, 0, 0, 0, 0, 255])
        assert data[:20] == want and data[20:512] == bytes(492), mode
        n = 3 * c
        tab = struct.unpack(f">{2 * n}I", data[512:512 + 8 * n])
        # random bytes are all literal: 65 + 1 header + the terminator
        assert tab[n:] == (67,) * n, mode
        # entry y + z H: file row 0 (the bottom row) first, within a row channel 0 .. C - 1
        order = sorted(range(n), key=lambda e: tab[e])
        assert order == [y + z * 3 for y in range(3) for z in range(c)], mode
        assert tab[0] == 512 + 8 * n and len(data) == 512 + 8 * n + 67 * n
        # file row 0, channel 0 is the image's bottom row
        first = data[tab[0]:tab[0] + 67]
        assert first == bytes([0x80 | 65]) + I.expected(img, c)[2, :, 0].tobytes() + b"\0", mode


def test_packets_of_the_rule(rr, tmp_path):
    """The restatement on row-planes whose packets are written out by hand, and the host coder on the same."""
    def both(*v):
        p = np.array(v, np.uint8)
        img = np.zeros((1, len(p), 4), np.uint8)
        img[0, :, 1] = p  # the G plane of an RGB file; R and B are one run or one byte
        data = _host_file(rr, tmp_path, img, "RGB")
        start, length = struct.unpack(">II", data[512 + 4:512 + 8] + data[512 + 16:512 + 20])
        assert data[start:start + length] == I.pack_plane(p)
        return I.pack_plane(p)

    assert both(1, 2, 2, 3) == bytes([0x84, 1, 2, 2, 3, 0])                      # a pair stays literal
    assert both(1, 2, 2, 2, 3) == bytes([0x81, 1, 3, 2, 0x81, 3, 0])              # three are a run
    assert both(7) == bytes([0x81, 7, 0]) and both(7, 7) == bytes([0x82, 7, 7, 0]) and both(7, 7, 7) == bytes([3, 7, 0])
    assert both(*[9] * 300) == bytes([127, 9, 127, 9, 46, 9, 0])                  # run packets of 127
    assert both(*[9] * 128) == bytes([127, 9, 1, 9, 0])                           # a remainder of 1 is a run packet
    assert both(5, 5, 5, 6, 6, 6) == bytes([3, 5, 3, 6, 0])                       # runs back to back
    lit = (np.arange(130) % 2).astype(np.uint8)
    assert both(*lit) == bytes([0xFF]) + lit[:127].tobytes() + bytes([0x83]) + lit[127:].tobytes() + b"\0"
    for w in (126, 127, 128, 254, 255, 381):  # the bound is met by an all-literal row-plane
        assert len(I.pack_plane((np.arange(w) % 251).astype(np.uint8))) == I.plane_bound(w)
    # packets cross neither a row nor a channel: three equal bytes over a row's end are literal
    img = np.zeros((2, 4, 4), np.uint8)
    img[..., 0] = [[7, 7, 1, 2], [1, 2, 3, 7]]  # the file's rows: bottom first
    px, info = I.read(_host_file(rr, tmp_path, img, "RGB"))
    assert info["packets"][0][0] == [(False, 4)] and info["packets"][1][0] == [(False, 4)]


def test_reader_rejects(rr):
    img = IMAGES["two values 65x3"]
    good = I.encode(img, 3)
    I.read(good)
    with pytest.raises(I.FormatError, match="trailing"):
        I.read(good + b"\0")
    with pytest.raises(I.FormatError, match="short"):
        I.read(good[:-1])
    for at, v in ((0, 0), (1, 0xDB), (2, 0), (3, 2), (5, 2), (11, 2), (12, 1), (19, 254), (20, 1), (24, ord("n")),
                  (107, 1), (511, 1)):
        bad = bytearray(good)
        bad[at] = v
        with pytest.raises(I.FormatError, match="header"):
            I.read(bytes(bad))
    # 4 x 1 grey files by hand
    head = I.header(4, 1, 1)
    tab = lambda start, n: struct.pack(">II", start, n)  # noqa: E731
    assert np.array_equal(I.read(head + tab(520, 3) + bytes([4, 5, 0]))[0][0, :, 0], [5, 5, 5, 5])
    I.read(head + tab(520, 6) + bytes([0x84, 5, 6, 7, 8, 0]))
    with pytest.raises(I.FormatError, match="start entry"):
        I.read(head + tab(521, 3) + bytes([4, 5, 0]))
    with pytest.raises(I.FormatError, match="length entry"):
        I.read(head + tab(520, 4) + bytes([4, 5, 0]))
    with pytest.raises(I.FormatError, match="count 0"):
        I.read(head + tab(520, 3) + bytes([3, 5, 0]))
    with pytest.raises(I.FormatError, match="count 0"):
        I.read(head + tab(520, 4) + bytes([0x80, 4, 5, 0]))
    with pytest.raises(I.FormatError, match="no 0 byte"):
        I.read(head + tab(520, 4) + bytes([4, 5, 1, 5]))
    with pytest.raises(I.FormatError, match="overruns"):
        I.read(head + tab(520, 3) + bytes([5, 5, 0]))
    with pytest.raises(I.FormatError, match="three equal bytes"):
        I.read(head + tab(520, 6) + bytes([0x84, 5, 5, 5, 8, 0]))
    with pytest.raises(I.FormatError, match="below three"):
        I.read(head + tab(520, 6) + bytes([2, 5, 0x82, 6, 7, 0]))
    with pytest.raises(I.FormatError, match="could merge"):
        I.read(head + tab(520, 5) + bytes([2, 5, 2, 5, 0]))
    with pytest.raises(I.FormatError, match="could merge"):
        I.read(head + tab(520, 7) + bytes([0x82, 5, 6, 0x82, 7, 8, 0]))
    # the second table entry of two rows: swapped starts are out of order
    two = I.encode(np.arange(32, dtype=np.uint8).reshape(2, 4, 4), 1)
    I.read(two)
    swapped = two[:512] + two[516:520] + two[512:516] + two[520:]
    with pytest.raises(I.FormatError, match="start entry"):
        I.read(swapped)


def test_refusals(rr, tmp_path):
    n = rr.native
    L = rr.lib()
    out = str(tmp_path / "x").encode()
    nb = ctypes.c_uint64()
    wide = np.zeros((1, 65536, 4), np.uint8)
    ptr = wide.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    # a side above 65535, and a body bound of 2 GB and more: refused before the image is read
    for w, h in ((65536, 1), (1, 65536), (65535, 65535), (32768, 16384), (65535, 9000)):
        assert L.rr_encode_image(ptr, w, h, out, b"IRIS", 90, ctypes.byref(nb)) == n.RR_EINVAL, (w, h)
    for mode in (1, 3, 4):
        assert L.rr_encode_image_mode(ptr, 65536, 1, out, b"IRIS", 90, mode, ctypes.byref(nb)) == n.RR_EINVAL
    assert L.rr_encode_image(None, 4, 4, out, b"IRIS", 90, ctypes.byref(nb)) == n.RR_EINVAL
    assert L.rr_encode_image_mode(ptr, 4, 4, out, b"IRIS", 90, 2, ctypes.byref(nb)) == n.RR_EINVAL
    assert not (tmp_path / "x.rgb").exists()
    # 65535 is inside the format: four channels, each 517 run packets and the terminator
    assert rr.encode_image(wide[:, :65535], str(tmp_path / "y"), "IRIS") == 512 + 32 + 4 * (2 * 517 + 1)
    # the names beside it stay refused, and the message names the new format
    img8 = np.zeros((4, 4, 4), np.uint8)
    for fmt in ("TIFF", "BMP"):
        with pytest.raises(rr.RRError) as e:
            rr.encode_image(img8, str(tmp_path / "z"), fmt)
        assert e.value.code == n.RR_ENOTSUP and f"unsupported output format '{fmt}'" in str(e.value)
        assert "IRIS" in str(e.value)


def test_iris_check_program(tmp_path):
    """tests/cpp/iris_check.cpp: the host coder and the rule functions alone (host code, no HIP
    header), built with the system C++ compiler under AddressSanitizer and UBSan, run as a
    child process, as tests/test_hdr_format.py does."""
    csrc = os.path.join(ROOT, PKG, "csrc")
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "iris_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
           os.path.join(ROOT, "tests", "cpp", "iris_check.cpp"), os.path.join(csrc, "image_io.cpp"), "-o", exe, "-lz",
           "-lpthread"]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "iris_check: ok" in run.stdout


def test_abi_and_naming(rr):
    assert rr.lib().rr_abi_version() == 8
    assert rr.EXTENSIONS["IRIS"] == ".rgb"
    assert rr.output_file_path("/o", "#####", 3, "IRIS") == "/o/00003.rgb"
    assert "TIFF" not in rr.EXTENSIONS and "BMP" not in rr.EXTENSIONS


class _Ctx:
    """Stand-in for RenderContext: records what the runner asks for."""

    def __init__(self):
        self.calls = []

    def load_scene(self, path):
        return types.SimpleNamespace(close=lambda: None)

    def render_frame(self, scene, f, params, out, fmt, q):
        self.calls.append((f, out, fmt))
        t = types.SimpleNamespace(loaded_at=0.0, started_rendering_at=0.0, finished_rendering_at=0.0,
                                  file_saving_started_at=0.0, file_saving_finished_at=0.0)
        return t, types.SimpleNamespace(spp=1)

    def close(self):
        pass


def test_job_reaches_the_context(rr, tmp_path):
    job = rr.BlenderJob.load_from_file(os.path.join(ROOT, "jobs", "04_very-simple_demo_10f-1w.toml"))
    job = rr.BlenderJob.from_dict({**job.to_dict(), "output_directory_path": str(tmp_path / "out"),
                                   "output_file_format": "IRIS"})
    assert all(p.endswith(".rgb") for p in rr.naming.job_output_files(job, str(tmp_path / "out")))
    ctx = _Ctx()
    runner = rr.BackendRunner(ROOT, ctx=ctx)
    runner.render_frame(job, 3)
    assert ctx.calls == [(3, str(tmp_path / "out" / "000003"), "IRIS")]
    for fmt in ("TIFF", "BMP"):
        with pytest.raises(rr.runner.RenderError):
            runner.render_frame(rr.BlenderJob.from_dict({**job.to_dict(), "output_file_format": fmt}), 3)
