"""WEBP (lossless, a RIFF container with one VP8L chunk), the parts that need no
GPU: the host coder's files equal the restatement of tests/webp.py byte for
byte, pass its strict reader, and decode, by that reader and by PIL (built
against libwebp: an independent decoder), to the image; quality below 100 gives
the same file and a warning; the size bound; the refusals; naming and the
runner; the reader rejects what it should; the stand-alone check program under
the sanitizers."""
import ctypes
import io
import os
import shutil
import struct
import subprocess
import types

import numpy as np
import pytest
from PIL import Image, features

import webp as W
from conftest import PKG, ROOT

MODES = {"BW": 1, "RGB": 3, "RGBA": 4}
IMAGES = W.images()


def _host_file(rr, tmp_path, img, mode, quality=100):
    n = rr.encode_image_mode(img, str(tmp_path / "f"), "WEBP", quality, mode)
    data = (tmp_path / "f.webp").read_bytes()
    assert n == len(data)
    return data


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} samples differ, first at {bad[0]}"


def _pil(data, w, h, c):
    im = Image.open(io.BytesIO(data))
    assert im.format == "WEBP" and im.size == (w, h) and im.mode == W.PIL_MODE[c], (im.format, im.size, im.mode)
    return np.asarray(im)


def test_pil_reads_webp():
    assert features.check("webp")


def test_rule_pieces():
    """The prefix of a length, the tokens of hand-written rows, the transforms' round trip."""
    assert [W.prefix(v) for v in (1, 2, 3, 4, 5, 6, 7, 9, 4096)] == [
        (0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 1, 0), (4, 1, 1), (5, 1, 0), (6, 2, 0), (23, 10, 1023)]
    assert W.MIN_RUN >= 2
    n = W.MIN_RUN
    row = [7] + [9] * (n + 1) + [8]  # n pixels equal their left neighbour
    assert W.tokens(row) == [("lit", 7), ("lit", 9), ("copy", n), ("lit", 8)]
    row = [7] + [9] * n + [8]  # n - 1: literals
    assert W.tokens(row) == [("lit", 7)] + [("lit", 9)] * n + [("lit", 8)]
    assert W.tokens([5] * 4098) == [("lit", 5), ("copy", 4096), ("lit", 5)]  # a remainder of 1
    assert W.tokens([5] * (4097 + n)) == [("lit", 5), ("copy", 4096), ("copy", n)]
    rng = np.random.default_rng(1)
    res = rng.integers(0, 1 << 32, (7, 9), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(W.residuals(W.from_residuals(res)), res)
    # a tree deeper than the limit is repaired to a complete code of 15 bits
    fib = [1, 1]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    lens, depth = W.lengths(fib, 15)
    assert depth == 19 and max(lens) == 15 and sum(1 << (15 - l) for l in lens) == 1 << 15


@pytest.mark.parametrize("mode", ["BW", "RGB", "RGBA"])
def test_host_files(rr, tmp_path, mode):
    c = MODES[mode]
    for name, img in IMAGES.items():
        h, w = img.shape[:2]
        data = _host_file(rr, tmp_path, img, mode)
        assert data == W.encode(img, c), (name, "host file differs from the restatement")
        px, info = W.read(data)
        assert (info["alpha"], info["width"], info["height"]) == (1 if c == 4 else 0, w, h), name
        want = W.expected(img, c)
        _same(px, want, name)
        if c == 1:
            assert np.all(px[..., 0] == px[..., 1]) and np.all(px[..., 1] == px[..., 2])
        # the bound the stream's buffers are sized by: a condition, not a measurement
        assert info["payload"] <= W.body_bound(w, h) and len(data) <= W.file_bound(w, h), name
        _same(_pil(data, w, h, c), W.pil_expected(img, c), ("PIL", name))


def test_mode_0_is_rgba(rr, tmp_path):
    img = IMAGES["random 300x17"]
    assert _host_file(rr, tmp_path, img, 0) == _host_file(rr, tmp_path, img, "RGBA")
    rr.encode_image(img, str(tmp_path / "g"), "WEBP", 100)
    assert (tmp_path / "g.webp").read_bytes() == W.encode(img, 4)
    assert not np.all(img[..., 3] == 255)  # alpha is the image's own


def test_container_and_header(rr, tmp_path):
    for name in ("random 65x3", "flat 65x3", "random 1x1"):  # an odd and an even payload among them
        img = IMAGES[name]
        h, w = img.shape[:2]
        for mode, c in MODES.items():
            data = _host_file(rr, tmp_path, img, mode)
            n = struct.unpack("<I", data[16:20])[0]
            assert data[:4] == b"RIFF" and data[8:16] == b"WEBPVP8L"
            assert struct.unpack("<I", data[4:8])[0] == len(data) - 8 and len(data) == 20 + n + (n & 1)
            assert len(data) % 2 == 0 and (not n & 1 or data[-1] == 0)
            bits = int.from_bytes(data[20:25], "little")
            assert bits & 255 == 0x2F and (bits >> 8) & 0x3FFF == w - 1 and (bits >> 22) & 0x3FFF == h - 1
            assert (bits >> 36) & 1 == (1 if c == 4 else 0) and (bits >> 37) & 7 == 0


def test_codes_of_the_rule(rr, tmp_path):
    """The forms the rule names: a simple code for at most two used symbols below 256 and for
    an unused alphabet; a normal one otherwise, also for two used symbols with a length among
    them."""
    flat = IMAGES["flat 300x17"]
    info = {}
    assert _host_file(rr, tmp_path, flat, "RGBA") == W.encode(flat, 4, info)
    assert [f["simple"] for f in info["codes"]] == [None, 2, 2, 2, 1]  # first pixel and zeros; distance: one symbol
    assert info["tokens"][1] == [("lit", 0), ("copy", 299)]
    info = {}
    one = np.zeros((2, 2, 4), np.uint8)
    one[..., 3] = 255
    assert _host_file(rr, tmp_path, one, "RGB") == W.encode(one, 3, info)
    assert [f["simple"] for f in info["codes"]] == [1, 1, 1, 1, 0]  # nothing but zeros: no bit a pixel
    assert info["bits"] == info["header_bits"]
    info = {}
    row = np.zeros((1, 40, 4), np.uint8)
    row[..., 3] = 255
    assert _host_file(rr, tmp_path, row, "RGB") == W.encode(row, 3, info)
    assert info["codes"][0] == {"simple": None, "depth": 1, "cl_used": 2, "max_len": 1}  # a literal and a length
    info = {}
    img = W.uniform_red_image()
    assert _host_file(rr, tmp_path, img, "RGBA") == W.encode(img, 4, info)
    assert info["codes"][1]["cl_used"] == 1 and info["codes"][1]["max_len"] == 8
    _same(_pil(_host_file(rr, tmp_path, img, "RGBA"), 64, 64, 4), img, "one used code length")
    info = {}
    img = W.fibonacci_image()
    data = _host_file(rr, tmp_path, img, "RGBA")
    assert data == W.encode(img, 4, info)
    assert info["codes"][0]["depth"] > 15 and info["codes"][0]["max_len"] == 15  # the repair is at work
    _same(_pil(data, 70, 64, 4), img, "repaired lengths")
    _same(W.read(data)[0], img, "repaired lengths, strict reader")


def test_quality(rr, tmp_path):
    """Lossless at every quality; below 100 the same bytes and a warning that names the quality."""
    img = IMAGES["sparse 300x17"]
    warned = rr.native.last_host_warning
    q100 = _host_file(rr, tmp_path, img, "RGB", 100)
    assert warned() == ""
    q90 = _host_file(rr, tmp_path, img, "RGB", 90)
    warning = warned()
    assert q90 == q100
    assert "WEBP" in warning and "90" in warning and "lossy WEBP is not built" in warning
    rr.encode_image(img, str(tmp_path / "q"), "WEBP", 1)
    assert (tmp_path / "q.webp").read_bytes() == W.encode(img, 4) and " 1:" in warned()
    _host_file(rr, tmp_path, img, "RGB", 100)
    assert warned() == ""
    rr.encode_image(img, str(tmp_path / "p"), "PNG", 90)  # another format's quality is not flagged
    assert warned() == ""


def test_reader_rejects(rr):
    img = IMAGES["sparse 65x3"]
    good = W.encode(img, 4)
    W.read(good)
    n = struct.unpack("<I", good[16:20])[0]
    with pytest.raises(W.FormatError, match="trailing"):
        W.read(good + b"\0")
    with pytest.raises(W.FormatError, match="short"):
        W.read(good[:-2])
    with pytest.raises(W.FormatError, match="chunk sizes"):
        W.read(good[:4] + struct.pack("<I", len(good) - 6) + good[8:])
    with pytest.raises(W.FormatError, match="header"):
        W.read(good[:20] + b"\x2E" + good[21:])
    # a longer chunk with the same image in it: bytes, or bits, after the image
    longer = W.wrap(good[20:20 + n] + b"\0\0")
    with pytest.raises(W.FormatError, match="trailing bytes in the chunk"):
        W.read(longer)
    info = W.read(good)[1]
    if info["bits"] % 8:
        body = bytearray(good[20:20 + n])
        body[-1] |= 0x80
        with pytest.raises(W.FormatError, match="trailing bits"):
            W.read(W.wrap(bytes(body)))
    # hand-made payloads: a 4 x 2 image, green a normal code over {0, 256 + prefix(3)}
    def payload(green_lens, toks, w=4, h=2):
        b = W.Bits()
        b.put(0x2F, 8), b.put(w - 1, 14), b.put(h - 1, 14), b.put(0, 1), b.put(0, 3)
        b.put(1, 1), b.put(2, 2), b.put(1, 1), b.put(0, 2), b.put(W.BLOCK_BITS - 2, 3), b.put(0, 1)
        b.simple([1])
        for _ in range(4):
            b.simple([0])
        b.put(0, 1), b.put(0, 1), b.put(0, 1)
        # code lengths 0, 1 and 2 through a complete code-length code: 0 -> 1 bit, 1 and 2 -> 2 bits
        cllen = [0] * 19
        cllen[0], cllen[1], cllen[2] = 1, 2, 2
        cl = W.canonical(cllen)
        b.put(0, 1), b.put(15, 4)
        for k in W.CL_ORDER:
            b.put(cllen[k], 3)
        b.put(0, 1)
        for l in green_lens:
            b.code(cl[l])
        for _ in range(3):
            b.simple([0])
        b.simple([1])
        codes = W.canonical(green_lens)
        for t in toks:
            b.code(codes[t])
            if t == 258:
                pass  # prefix(3) has no extra bits, the distance code's one symbol none
        return W.wrap(b.done())

    lens = [0] * 280
    lens[0], lens[258] = 1, 1
    px, info = W.read(payload(lens, [0, 258, 0, 258]))
    assert info["tokens"] == [[("lit", 0), ("copy", 3)]] * 2 and np.all(px[..., :3] == 0)
    with pytest.raises(W.FormatError, match="crosses a row"):
        W.read(payload(lens, [0, 0, 0, 258, 0]))  # three pixels from the row's third on
    with pytest.raises(W.FormatError, match="crosses a row"):
        W.read(payload(lens, [0, 258, 258, 0]))  # a copy as a row's first pixel
    over = list(lens)
    over[1] = 1
    with pytest.raises(W.FormatError, match="over-subscribed"):
        W.read(payload(over, []))
    under = [0] * 280
    under[0], under[258] = 1, 2
    with pytest.raises(W.FormatError, match="under-subscribed"):
        W.read(payload(under, []))


def test_refusals(rr, tmp_path):
    n = rr.native
    L = rr.lib()
    out = str(tmp_path / "x").encode()
    nb = ctypes.c_uint64()
    wide = np.zeros((1, 16385, 4), np.uint8)
    ptr = wide.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    # a side above 16384: refused before the image is read
    for w, h in ((16385, 1), (1, 16385), (16385, 16385), (65536, 1)):
        assert L.rr_encode_image(ptr, w, h, out, b"WEBP", 100, ctypes.byref(nb)) == n.RR_EINVAL, (w, h)
        assert b"WEBP" in L.rr_last_error(None)
    for mode in (1, 3, 4):
        assert L.rr_encode_image_mode(ptr, 16385, 1, out, b"WEBP", 100, mode, ctypes.byref(nb)) == n.RR_EINVAL
    assert L.rr_encode_image(None, 4, 4, out, b"WEBP", 100, ctypes.byref(nb)) == n.RR_EINVAL
    assert L.rr_encode_image_mode(ptr, 4, 4, out, b"WEBP", 100, 2, ctypes.byref(nb)) == n.RR_EINVAL
    assert not (tmp_path / "x.webp").exists()
    # 16384 is inside the format: one literal and four copies of 4096, 4096, 4096 and 4095
    wide[..., 3] = 255  # the first pixel's residual is 0 too: 16383 pixels equal their left neighbour
    rr.encode_image(wide[:, :16384], str(tmp_path / "y"), "WEBP", 100)
    info = W.read((tmp_path / "y.webp").read_bytes())[1]
    assert info["tokens"] == [[("lit", 0), ("copy", 4096), ("copy", 4096), ("copy", 4096), ("copy", 4095)]]
    # the names beside it stay refused, and the message names the new format
    img8 = np.zeros((4, 4, 4), np.uint8)
    for fmt in ("TIFF", "BMP"):
        with pytest.raises(rr.RRError) as e:
            rr.encode_image(img8, str(tmp_path / "z"), fmt)
        assert e.value.code == n.RR_ENOTSUP and f"unsupported output format '{fmt}'" in str(e.value)
        assert "WEBP" in str(e.value) and "IRIS" in str(e.value) and "TARGA_RAW" in str(e.value)


def test_webp_check_program(tmp_path):
    """tests/cpp/webp_check.cpp: the host coder and the rule functions alone (host code, no HIP
    header), built with the system C++ compiler under AddressSanitizer and UBSan, run as a
    child process, as tests/test_iris_format.py does."""
    csrc = os.path.join(ROOT, PKG, "csrc")
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "webp_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
           os.path.join(ROOT, "tests", "cpp", "webp_check.cpp"), os.path.join(csrc, "image_io.cpp"), "-o", exe, "-lz",
           "-lpthread"]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "webp_check: ok" in run.stdout


def test_abi_and_naming(rr):
    assert rr.lib().rr_abi_version() == 8
    assert rr.EXTENSIONS["WEBP"] == ".webp"
    assert rr.output_file_path("/o", "#####", 3, "WEBP") == "/o/00003.webp"
    assert "TIFF" not in rr.EXTENSIONS and "BMP" not in rr.EXTENSIONS
    assert sorted(rr.EXTENSIONS) == ["HDR", "IRIS", "JPEG", "OPEN_EXR", "PNG", "TARGA", "TARGA_RAW", "WEBP"]


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
                                   "output_file_format": "WEBP"})
    assert all(p.endswith(".webp") for p in rr.naming.job_output_files(job, str(tmp_path / "out")))
    ctx = _Ctx()
    runner = rr.BackendRunner(ROOT, ctx=ctx)
    runner.render_frame(job, 3)
    assert ctx.calls == [(3, str(tmp_path / "out" / "000003"), "WEBP")]
    for fmt in ("TIFF", "BMP"):
        with pytest.raises(rr.runner.RenderError):
            runner.render_frame(rr.BlenderJob.from_dict({**job.to_dict(), "output_file_format": fmt}), 3)
