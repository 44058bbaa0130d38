"""HDR (Radiance RGBE), the parts that need no GPU: the host coder's quads equal
the numpy restatement of tests/hdr.py at every value where the rule branches and
on random float bits; its files equal the restatement byte for byte and pass
the strict reader; flat and coded widths; truncation; BW; the refusals; naming
and the runner; the reader rejects what it should."""
import ctypes
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import color_modes as M
import hdr as H
from conftest import PKG, ROOT

F32 = np.float32
MODES = {"BW": 1, "RGB": 3, "RGBA": 3}
IMAGES = H.images()


def _host_quads(rr, img, mode="RGB"):
    """The quads of the host coder's file, through the strict reader."""
    return H.read(rr.hdr_host(img, mode))[0]


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} samples differ, first at {bad[0]}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


def test_rule_at_its_branches(rr):
    img = H.special_row()
    n = img.shape[1]
    assert 8 <= n <= 32767
    want = H.rgbe(img[..., :3])
    _same(_host_quads(rr, img), want, "coded row")
    for at in range(0, n, 7):  # the same pixels in flat rows
        _same(_host_quads(rr, img[:, at:at + 7]), want[:, at:at + 7], f"flat row from {at}")
    # the quads the issue writes out, by the host coder alone
    def quad(r, g, b):
        return _host_quads(rr, np.array([[[r, g, b, 1.0]]], F32))[0, 0].tolist()

    inf, big = F32(np.inf), np.finfo(F32).max
    assert quad(1.0, 1.0, 1.0) == [128, 128, 128, 129]
    assert quad(0.5, 0.5, 0.5) == [128, 128, 128, 128]
    below_one = np.nextafter(F32(1.0), F32(0.0))
    assert quad(below_one, below_one, below_one) == [255, 255, 255, 128]
    for v in (inf, big, H.MAXV, np.nextafter(H.MAXV, inf)):
        assert quad(v, v, v) == [255, 255, 255, 255], v
    assert quad(np.nextafter(H.MAXV, F32(0)), 0.0, 0.0) == [254, 0, 0, 255]
    for v in (0.0, -0.0, -1.0, F32(np.nan), -inf, np.nextafter(H.TINY, F32(0)), F32(1e-40)):
        assert quad(v, v, v) == [0, 0, 0, 0], v
    assert quad(H.TINY, 0.0, 0.0)[3] == 22 and quad(H.TINY, 0.0, 0.0)[0] >= 128
    assert quad(1.0, 2.0 ** -20, 2.0 ** 20) == [0, 0, 128, 149]     # channels 2^20 apart
    assert quad(F32(1e-40), 1.0e4, -3.0) == [0, 156, 0, 142]        # a denormal beside a large channel


def test_rule_on_random_bits(rr):
    """10^5 quads of random float bits: every exponent, negatives, NaNs, infinities, denormals."""
    rng = np.random.default_rng(20)
    n = 100_000
    bits = rng.integers(0, 1 << 32, (1, n, 4), dtype=np.uint64).astype(np.uint32)
    # every exponent beside every other, 256 x 256 pairs, in the first two channels
    ea, eb = np.divmod(np.arange(65536, dtype=np.uint32), 256)
    bits[0, :65536, 0] = (bits[0, :65536, 0] & 0x007FFFFF) | (ea << 23)
    bits[0, :65536, 1] = (bits[0, :65536, 1] & 0x007FFFFF) | (eb << 23)
    bits[0, :65536:3, 2] |= 0x80000000  # a third channel that often drops out
    bits[0, 70000:70030:3, 0] = 0x7F800000  # infinities are too rare to come up by chance
    bits[0, 70001:70030:3, 1] = 0xFF800000
    img = bits.view(F32)
    assert np.isnan(img).any() and np.isinf(img).any() and (img < 0).any()
    _same(_host_quads(rr, img), H.rgbe(img[..., :3]), "random bits")  # W > 32767: a flat row
    with np.errstate(all="ignore"):
        _same(_host_quads(rr, img, "BW"), H.quads(img, 1), "random bits, BW")


@pytest.mark.parametrize("mode", ["BW", "RGB", "RGBA"])
def test_host_files(rr, mode):
    c = MODES[mode]
    for name, img in IMAGES.items():
        h, w = img.shape[:2]
        data = rr.hdr_host(img, mode)
        assert data == H.encode(img, c), (name, "host file differs from the restatement")
        q, info = H.read(data)
        assert (info["width"], info["height"], info["flat"]) == (w, h, H.flat(w)), name
        _same(q, H.quads(img, c), name)
        # the bound the stream's buffers are sized by: a condition, not a measurement
        assert info["body"] <= h * H.row_bound(w), name
        for row in info["packets"]:
            assert len(row) == 4 and all(sum(n for _, n in plane) == w for plane in row), name
            assert all(1 <= n <= (127 if run else 128) for plane in row for run, n in plane), name
    assert rr.hdr_host(IMAGES["shape 65x3"], 0) == rr.hdr_host(IMAGES["shape 65x3"], "RGB")


def test_header_bytes(rr):
    data = rr.hdr_host(IMAGES["shape 129x3"], "RGB")
    assert data.startswith(b"#?RADIANCE\x0aFORMAT=32-bit_rle_rgbe\x0a\x0a-Y 3 +X 129\x0a\x02\x02\x00\x81")


def test_packets_of_the_rule(rr):
    """The restatement on planes whose packets are written out by hand, and the host coder on the crafted images."""
    P = lambda *v: H.pack_plane(np.array(v, np.uint8))  # noqa: E731
    assert P(1, 2, 2, 2, 3) == bytes([5, 1, 2, 2, 2, 3])                    # three stay literal
    assert P(1, 2, 2, 2, 2, 3) == bytes([1, 1, 128 + 4, 2, 1, 3])            # four are a run
    assert P(*[9] * 300) == bytes([255, 9, 255, 9, 128 + 46, 9])            # run packets of 127
    assert P(*[9] * 128) == bytes([255, 9, 129, 9])                         # a remainder of 1 is legal
    lit = (np.arange(130) % 2).astype(np.uint8)
    assert H.pack_plane(lit) == bytes([128]) + lit[:128].tobytes() + bytes([2]) + lit[128:].tobytes()
    assert P(7, 7, 7, 7) == bytes([132, 7]) and P(7) == bytes([1, 7])
    assert P(5, 5, 5, 5, 6, 6, 6, 6) == bytes([132, 5, 132, 6])             # runs back to back
    # runs of every named length: row i's plane k holds RUNS[(i + k) % len] between literals
    data = rr.hdr_host(IMAGES["runs"], "RGB")
    assert data == H.encode(IMAGES["runs"], 3)
    packets = H.read(data)[1]["packets"]
    for i, row in enumerate(packets):
        for k, plane in enumerate(row):
            n = H.RUNS[(i + k) % len(H.RUNS)]
            assert sum(m for run, m in plane if run) == (n if n >= 4 else 0), (i, k)
            assert [m for run, m in plane if run] == ([127] * (n // 127) + ([n % 127] if n % 127 else []) if n >= 4 else [])
    # literal stretches of 128, 129 and 257 bytes
    data = rr.hdr_host(IMAGES["literals"], "RGB")
    assert data == H.encode(IMAGES["literals"], 3)
    for row, n in zip(H.read(data)[1]["packets"], H.LITS):
        r = row[0]  # R: run 5, lit n, run 4, then literals to the width
        assert r[0] == (True, 5) and [m for run, m in r[1:1 + (n + 127) // 128]] == [128] * (n // 128) + [n % 128] * (n % 128 > 0)
        assert all(not run for run, _ in r[1:1 + (n + 127) // 128])
    # a run that ends a plane, a plane that is one run
    data = rr.hdr_host(IMAGES["run ends"], "RGB")
    assert data == H.encode(IMAGES["run ends"], 3)
    rows = H.read(data)[1]["packets"]
    assert rows[0][0][-1] == (True, 35) and rows[0][1] == [(True, 40)] and rows[0][2] == [(True, 4), (True, 36)]
    assert rows[1][2] == [(False, 40)]  # a run of 3 at the end stays literal
    # packets cross neither a row nor a plane
    data = rr.hdr_host(IMAGES["ends meet"], "RGB")
    assert data == H.encode(IMAGES["ends meet"], 3)
    rows = H.read(data)[1]["packets"]
    assert rows[0][0][-1] == (True, 4) and rows[0][1][0] == (True, 4)
    assert all(sum(m for _, m in plane) == 40 for row in rows for plane in row)
    assert all(not run for run, _ in rows[1][0][:1])  # three equal bytes at a row's start: no run across the rows


@pytest.mark.parametrize("w,is_flat", [(7, True), (8, False), (32767, False), (32768, True)])
def test_flat_and_coded_widths(rr, w, is_flat):
    img = H.shape_image(w, 2, seed=w)
    data = rr.hdr_host(img, "RGB")
    assert data == H.encode(img, 3)
    q, info = H.read(data)
    assert info["flat"] == is_flat and q.shape == (2, w, 4)
    if is_flat:
        assert info["body"] == 8 * w and data[len(H.header(w, 2)):] == H.quads(img, 3).tobytes()
    else:
        assert data[len(H.header(w, 2)):][:4] == bytes([2, 2, w >> 8, w & 255])


def test_truncation_brackets_the_input(rr):
    rng = np.random.default_rng(3)
    img = np.ones((4, 500, 4), F32)
    img[..., :3] = np.exp(rng.normal(0, 6, (4, 500, 3))).astype(F32)
    q = _host_quads(rr, img).astype(np.int64)
    v = img[..., :3].astype(np.float64)
    unit = np.ldexp(1.0, q[..., 3:] - 136)
    lo = q[..., :3] * unit
    assert np.all(q[..., 3] > 0)
    assert np.all(lo <= v) and np.all(v < lo + unit)
    _same(H.decode(q), lo, "decode")
    assert (q[..., :3].max(axis=-1) >= 128).all()  # the largest channel is normalised


def test_bw_is_the_luma_of_the_means(rr):
    img = IMAGES["shape 257x3"]
    q = _host_quads(rr, img, "BW")
    assert np.array_equal(q[..., 0], q[..., 1]) and np.array_equal(q[..., 0], q[..., 2])
    with np.errstate(all="ignore"):
        y = M.luma(img[..., 0], img[..., 1], img[..., 2])
    _same(q, H.rgbe(np.stack([y, y, y], axis=-1)), "BW")
    assert not np.array_equal(q, _host_quads(rr, img, "RGB"))


def test_reader_rejects(rr):
    img = IMAGES["shape 9x2"]
    good = H.encode(img, 3)
    H.read(good)
    with pytest.raises(H.FormatError, match="trailing"):
        H.read(good + b"\0")
    with pytest.raises(H.FormatError, match="short"):  # a short plane
        H.read(good[:-1])
    head = H.header(8, 1)
    ok = head + bytes([2, 2, 0, 8]) + bytes([136, 5]) * 4
    assert np.all(H.read(ok)[0] == 5)
    with pytest.raises(H.FormatError, match="count 0"):
        H.read(head + bytes([2, 2, 0, 8]) + bytes([0, 136, 5]) + bytes([136, 5]) * 3)
    with pytest.raises(H.FormatError, match="overruns"):  # 128 is a literal packet of 128 bytes
        H.read(head + bytes([2, 2, 0, 8]) + bytes([128, 5, 136, 5]) + bytes([136, 5]) * 3)
    with pytest.raises(H.FormatError, match="overruns"):
        H.read(head + bytes([2, 2, 0, 8]) + bytes([137, 5]) + bytes([136, 5]) * 3)
    with pytest.raises(H.FormatError, match="overruns"):
        H.read(head + bytes([2, 2, 0, 8]) + bytes([132, 5, 5, 1, 2, 3, 4, 5]) + bytes([136, 5]) * 3)
    for marker in ([2, 2, 0, 9], [1, 2, 0, 8], [2, 1, 0, 8], [2, 2, 1, 8]):
        with pytest.raises(H.FormatError, match="marker"):
            H.read(head + bytes(marker) + bytes([136, 5]) * 4)
    with pytest.raises(H.FormatError, match="short"):
        H.read(head + bytes([2, 2, 0, 8]) + bytes([136, 5]) * 3)
    for bad in (b"#?RGBE\n" + good[11:], good.replace(b"-Y 2", b"+Y 2"), good.replace(b"rle_rgbe", b"rle_xyze"),
                good.replace(b"\n\n-Y", b"\nEXPOSURE=1\n\n-Y")):
        with pytest.raises(H.FormatError, match="header"):
            H.read(bad)
    flat = H.encode(img[:, :7], 3)
    H.read(flat)
    for bad in (flat + b"\0", flat[:-1]):
        with pytest.raises(H.FormatError):
            H.read(bad)


def test_refusals(rr, tmp_path):
    n = rr.native
    L = rr.lib()
    tiny = np.zeros((1, 1, 4), F32)
    nb = ctypes.c_uint64()
    fp = tiny.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    # a body bound of 2 GB: refused before the image is read (it is one pixel)
    for w, h in ((32768, 16384), (1 << 29, 1), (32767, 16400), (1, 1 << 29)):
        assert L.rr_debug_hdr_host(fp, w, h, 3, None, 0, ctypes.byref(nb)) == n.RR_EINVAL, (w, h)
    assert L.rr_debug_hdr_host(None, 1, 1, 3, None, 0, ctypes.byref(nb)) == n.RR_EINVAL
    assert L.rr_debug_hdr_host(fp, 1, 1, 2, None, 0, ctypes.byref(nb)) == n.RR_EINVAL
    assert L.rr_debug_hdr_host(fp, 1, 1, 3, None, 0, ctypes.byref(nb)) == 0 and nb.value == len(H.header(1, 1)) + 4
    # the host-image entries have no float film
    img8 = np.zeros((4, 4, 4), np.uint8)
    for call in (lambda: rr.encode_image(img8, str(tmp_path / "x"), "HDR"),
                 lambda: rr.encode_image_mode(img8, str(tmp_path / "x"), "HDR", 90, "RGB")):
        with pytest.raises(rr.RRError) as e:
            call()
        assert e.value.code == n.RR_ENOTSUP and "float film" in str(e.value)
    assert not (tmp_path / "x.hdr").exists()
    for fmt in ("TIFF", "BMP"):
        with pytest.raises(rr.RRError) as e:
            rr.encode_image(img8, str(tmp_path / "y"), fmt)
        assert e.value.code == n.RR_ENOTSUP and f"unsupported output format '{fmt}'" in str(e.value)


def test_hdr_check_program(tmp_path):
    """tests/cpp/hdr_check.cpp: the host coder and the rule functions alone (host code, no HIP
    header), built with the system C++ compiler under AddressSanitizer and UBSan, run as a
    child process, as tests/test_settings.py does."""
    csrc = os.path.join(ROOT, PKG, "csrc")
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "hdr_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-ffp-contract=off",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", csrc,
           os.path.join(ROOT, "tests", "cpp", "hdr_check.cpp"), os.path.join(csrc, "image_io.cpp"), "-o", exe, "-lz",
           "-lpthread"]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "hdr_check: ok" in run.stdout


def test_abi_and_naming(rr):
    assert rr.lib().rr_abi_version() == 8
    assert rr.EXTENSIONS["HDR"] == ".hdr"
    assert rr.output_file_path("/o", "#####", 3, "HDR") == "/o/00003.hdr"
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
                                   "output_file_format": "HDR"})
    assert all(p.endswith(".hdr") for p in rr.naming.job_output_files(job, str(tmp_path / "out")))
    ctx = _Ctx()
    runner = rr.BackendRunner(ROOT, ctx=ctx)
    runner.render_frame(job, 3)
    assert ctx.calls == [(3, str(tmp_path / "out" / "000003"), "HDR")]
    for fmt in ("TIFF", "BMP"):
        with pytest.raises(rr.runner.RenderError):
            runner.render_frame(rr.BlenderJob.from_dict({**job.to_dict(), "output_file_format": fmt}), 3)
