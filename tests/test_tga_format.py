"""TARGA and TARGA_RAW, the parts that need no GPU: the host coder's files equal
the restatement of tests/tga.py byte for byte and decode, by its strict reader
and by PIL, to the image; the size bound; the refusals; naming and the runner;
the reader rejects what it should."""
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

import tga as T
from conftest import PKG, ROOT

MODES = {"BW": 1, "RGB": 3, "RGBA": 4}
IMAGES = T.images()


def _host_file(rr, tmp_path, img, fmt, mode):
    n = rr.encode_image_mode(img, str(tmp_path / "f"), fmt, 90, mode)
    data = (tmp_path / "f.tga").read_bytes()
    assert n == len(data)
    return data


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} samples differ, first at {bad[0]}"


@pytest.mark.parametrize("fmt", ["TARGA", "TARGA_RAW"])
@pytest.mark.parametrize("mode", ["BW", "RGB", "RGBA"])
def test_host_files(rr, tmp_path, mode, fmt):
    c, rle = MODES[mode], fmt == "TARGA"
    for name, img in IMAGES.items():
        h, w = img.shape[:2]
        data = _host_file(rr, tmp_path, img, fmt, mode)
        assert data == T.encode(img, c, rle), (name, "host file differs from the restatement")
        px, info = T.read(data)
        assert (info["channels"], info["rle"], info["width"], info["height"]) == (c, rle, w, h), name
        want = T.expected(img, c)
        _same(px, want, name)
        # the bound the stream's buffers are sized by: a condition, not a measurement
        if rle:
            assert info["body"] <= h * T.row_bound(w, c), name
            assert all(sum(k for _, k in row) == w for row in info["packets"]), name
        else:
            assert info["body"] == w * h * c, name
        im = Image.open(io.BytesIO(data))
        assert im.mode == T.PIL_MODE[c] and im.size == (w, h), name
        _same(np.asarray(im).reshape(h, w, c), want, ("PIL", name))


def test_mode_0_is_rgba(rr, tmp_path):
    img = IMAGES["palette 300x3"]
    for fmt in ("TARGA", "TARGA_RAW"):
        assert _host_file(rr, tmp_path, img, fmt, 0) == _host_file(rr, tmp_path, img, fmt, "RGBA")
        rr.encode_image(img, str(tmp_path / "g"), fmt)
        assert (tmp_path / "g.tga").read_bytes() == T.encode(img, 4, fmt == "TARGA")


def test_packets_of_the_rule():
    """The restatement on rows whose packets are written out by hand."""
    def row(*px):
        return np.array(px, np.uint8).reshape(-1, 1)

    assert T.pack_row(row(1, 2, 2, 3)) == bytes([3, 1, 2, 2, 3])               # C = 1: a pair stays literal
    assert T.pack_row(row(1, 2, 2, 2, 3)) == bytes([0, 1, 0x82, 2, 0, 3])      # three are a run
    rgb = np.array([[1, 1, 1], [5, 5, 5], [5, 5, 5], [7, 7, 7]], np.uint8)
    assert T.pack_row(rgb) == bytes([0, 1, 1, 1, 0x81, 5, 5, 5, 0, 7, 7, 7])   # C = 3: two are a run
    assert T.pack_row(np.full((300, 1), 9, np.uint8)) == bytes([0xFF, 9, 0xFF, 9, 0x80 | 43, 9])
    lit = (np.arange(130) % 2).astype(np.uint8).reshape(-1, 1)
    assert T.pack_row(lit) == bytes([127]) + lit[:128].tobytes() + bytes([1]) + lit[128:].tobytes()
    # the named stretches are in the images: runs of every length, literal stretches of 129 and 257 pixels
    runs = T.read(T.encode(IMAGES["runs"], 4, True))[1]["packets"]
    assert [sum(k for r, k in row if r) for row in reversed(runs)] == [0 if n < 2 else n for n in T.RUNS]
    lits = T.read(T.encode(IMAGES["literals"], 4, True))[1]["packets"]
    assert [[k for r, k in row if not r] for row in reversed(lits)] == [[128, 1, 128, 4], [128, 128, 1, 4]]
    # a row's end never merges with the next row's start
    ends = T.read(T.encode(IMAGES["row ends"], 3, True))[1]["packets"]
    assert all(sum(k for _, k in row) == 40 for row in ends)


def test_reader_rejects(rr):
    good = T.encode(IMAGES["runs"], 3, True)
    T.read(good)
    with pytest.raises(T.FormatError, match="trailing"):
        T.read(good + b"\0")
    with pytest.raises(T.FormatError, match="short"):
        T.read(good[:-1])
    # 2 x 2 grey: a run of four crosses the row; a literal count overruns it
    h = T.header(2, 2, 1, True)
    T.read(h + bytes([1, 5, 6, 1, 7, 8]))
    with pytest.raises(T.FormatError, match="crosses"):
        T.read(h + bytes([0x83, 5]))
    with pytest.raises(T.FormatError, match="crosses"):
        T.read(h + bytes([0, 5, 2, 6, 7, 8]))
    # header fields
    for at, v in ((0, 1), (1, 1), (2, 1), (2, 9), (3, 1), (7, 8), (8, 1), (10, 1), (16, 16), (17, 0x20), (17, 8)):
        bad = bytearray(good)
        bad[at] = v
        with pytest.raises(T.FormatError):
            T.read(bytes(bad))
    raw = T.encode(IMAGES["rows"], 4, False)
    T.read(raw)
    for bad in (raw + b"\0", raw[:-1]):
        with pytest.raises(T.FormatError):
            T.read(bad)


def test_refusals(rr, tmp_path):
    n = rr.native
    L = rr.lib()
    out = str(tmp_path / "x").encode()
    nb = ctypes.c_uint64()
    wide = np.zeros((1, 65536, 4), np.uint8)
    for fmt in (b"TARGA", b"TARGA_RAW"):
        for w, h in ((65536, 1), (1, 65536)):
            rc = L.rr_encode_image(wide.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), w, h, out, fmt, 90,
                                   ctypes.byref(nb))
            assert rc == n.RR_EINVAL, (fmt, w, h)
        assert L.rr_encode_image(None, 4, 4, out, fmt, 90, ctypes.byref(nb)) == n.RR_EINVAL
        rc = L.rr_encode_image_mode(wide.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 4, 4, out, fmt, 90, 2,
                                    ctypes.byref(nb))
        assert rc == n.RR_EINVAL
    assert not (tmp_path / "x.tga").exists()
    # 65535 is inside the format
    assert rr.encode_image(wide[:, :65535], str(tmp_path / "y"), "TARGA") == T.HEADER + 512 * 5
    with pytest.raises(rr.RRError) as e:
        rr.encode_image(wide[:, :4], str(tmp_path / "z"), "BMP")
    assert e.value.code == n.RR_ENOTSUP
    assert "TARGA" in str(e.value)


def test_tga_check_program(tmp_path):
    """tests/cpp/tga_check.cpp: the host coder and the rule functions alone (host code, no HIP
    header), built with the system C++ compiler under AddressSanitizer and UBSan, run as a
    child process, as tests/test_iris_format.py does."""
    csrc = os.path.join(ROOT, PKG, "csrc")
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "tga_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
           os.path.join(ROOT, "tests", "cpp", "tga_check.cpp"), os.path.join(csrc, "image_io.cpp"), "-o", exe, "-lz",
           "-lpthread"]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "tga_check: ok" in run.stdout


def test_abi_and_naming(rr):
    assert rr.lib().rr_abi_version() == 8
    assert rr.output_file_path("/o", "#####", 3, "TARGA") == "/o/00003.tga"
    assert rr.output_file_path("/o", "#####", 3, "TARGA_RAW") == "/o/00003.tga"
    assert rr.EXTENSIONS["TARGA"] == rr.EXTENSIONS["TARGA_RAW"] == ".tga"


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


@pytest.mark.parametrize("fmt", ["TARGA", "TARGA_RAW"])
def test_job_reaches_the_context(rr, tmp_path, fmt):
    job = rr.BlenderJob.load_from_file(os.path.join(ROOT, "jobs", "04_very-simple_demo_10f-1w.toml"))
    job = rr.BlenderJob.from_dict({**job.to_dict(), "output_directory_path": str(tmp_path / "out"),
                                   "output_file_format": fmt})
    assert all(p.endswith(".tga") for p in rr.naming.job_output_files(job, str(tmp_path / "out")))
    ctx = _Ctx()
    rr.BackendRunner(ROOT, ctx=ctx).render_frame(job, 3)
    assert ctx.calls == [(3, str(tmp_path / "out" / "000003"), fmt)]


def test_header_bytes(rr, tmp_path):
    img = IMAGES["rows"]
    for mode, c in MODES.items():
        for fmt, rle in (("TARGA", True), ("TARGA_RAW", False)):
            head = _host_file(rr, tmp_path, img, fmt, mode)[:T.HEADER]
            want = bytes([0, 0, (3 if c == 1 else 2) + (8 if rle else 0), 0, 0, 0, 0, 0, 0, 0, 0, 0]) + \
                struct.pack("<HH", 37, 5) + bytes([8 * c, 8 if c == 4 else 0])
            assert head == want, (mode, fmt)
