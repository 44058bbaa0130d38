"""rr_set_exr_codec without a GPU: the ABI, the setting's spellings and
precedence (tests/cpp/exr_codec_check.cpp under ASan / UBSan), the scene field,
the exporter, the host statements of the two rules against numpy, and the
restatement's writer through its strict reader (tests/exr_codecs.py)."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import color_modes as CM
import exr_codecs as E
import exr_reader as X
from conftest import PKG, ROOT

CSRC = os.path.join(ROOT, PKG, "csrc")
S04 = os.path.join(ROOT, "scenes", "04_very-simple-standin.rrscene")
S01 = os.path.join(ROOT, "scenes", "01_simple-animation.rrscene")
BLEND01 = os.path.join(ROOT, "blender-projects", "01_simple-animation", "01_simple-animation.blend")
NAMES = ["NONE", "RLE", "ZIPS", "ZIP", "PIZ", "PXR24", "B44", "B44A", "DWAA", "DWAB"]


def test_abi_has_the_setter_and_keeps_its_version(rr):
    lib = rr.lib()
    for name in ("rr_set_exr_codec", "rr_debug_scene_exr_codec", "rr_debug_float24", "rr_debug_exr_rle"):
        assert hasattr(lib, name) and name in rr.EXPORTS
    assert lib.rr_abi_version() == 8
    assert lib.rr_set_exr_codec(None, 4) != 0  # NULL ctx: RR_EINVAL
    assert [rr.native.EXR_CODECS[n] for n in NAMES] == list(range(1, 11)) and rr.native.EXR_CODECS[""] == 0


def test_header_documents_the_setter():
    text = open(os.path.join(ROOT, "include", "rr.h")).read()
    doc = text[text.index("Compression of ctx's \"OPEN_EXR\" files"):text.index("int rr_set_exr_codec(")]
    assert "render-timing-script.py:83-92" in doc and "Not pinned" in doc
    for k, name in enumerate(["SCENE"] + NAMES):
        assert re.search(rf"#define RR_EXR_CODEC_{name} {k}\n", doc), name


def test_exr_codec_check_program(tmp_path):
    """Every spelling of RR_EXR_CODEC, the setter's range, resolve_output's precedence, the
    fallback's warning and the rule headers' host side: a stand-alone program of settings.cpp."""
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "exr_codec_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "exr_codec_check.cpp"), os.path.join(CSRC, "settings.cpp"), "-o", exe]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("RR_")}
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "exr_codec_check: ok" in run.stdout


def test_new_rule_headers_are_host_only():
    for name in ("exr_rle_rule.h", "pxr24_rule.h", "rle_rule.h"):
        with open(os.path.join(CSRC, name)) as f:
            assert "hip/" not in f.read(), name


# ------------------------------------------------------------- the scene ---
def _scene_with(tmp_path, name, **render):
    doc = json.load(open(S04))
    doc["render"].update(render)
    p = tmp_path / (name + ".rrscene")
    p.write_text(json.dumps(doc))
    return str(p)


@pytest.mark.parametrize("name", NAMES)
def test_scene_field_is_parsed(rr, tmp_path, name):
    s = rr.Scene(_scene_with(tmp_path, "ok", exr_codec=name))
    try:
        assert s.exr_codec() == rr.native.EXR_CODECS[name]
    finally:
        s.close()


@pytest.mark.parametrize("bad", ["zip", "", "TIFF", 4, None, "ZIP16"])
def test_scene_field_of_an_unknown_name_is_refused(rr, tmp_path, bad):
    with pytest.raises(rr.RRError) as e:
        rr.Scene(_scene_with(tmp_path, "bad", exr_codec=bad))
    assert "render.exr_codec" in str(e.value)


def test_scene_without_the_field_means_zip(rr):
    for f in sorted(os.listdir(os.path.join(ROOT, "scenes"))):
        if not f.endswith(".rrscene") or f.startswith("c5"):
            continue
        path = os.path.join(ROOT, "scenes", f)
        assert "exr_codec" not in json.load(open(path))["render"]
        s = rr.Scene(path)
        try:
            assert s.exr_codec() == rr.native.RR_EXR_CODEC_ZIP
        finally:
            s.close()


def test_exporter_writes_the_field_only_when_not_zip(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import blend_export as B
    args = argparse.Namespace(samples=128, max_bounces=12, clamp_indirect=10.0, seed=0)
    assert json.loads(json.dumps(B.export(BLEND01, args))) == json.load(open(S01))  # the project's codec: ZIP
    assert sorted(B.EXR_CODEC_OF_DNA.values()) == sorted(NAMES)
    # another number in the project's ImageFormatData.exr_codec: the field appears, by name
    real = B.BlendFile.read_struct_at if hasattr(B, "BlendFile") else None
    if real is None:
        pytest.fail("blend_export has no BlendFile")

    def patched(self, at, struct, field):
        return 4 if (struct, field) == ("ImageFormatData", "exr_codec") else real(self, at, struct, field)
    monkeypatch.setattr(B.BlendFile, "read_struct_at", patched)
    assert B.export(BLEND01, args)["render"]["exr_codec"] == "RLE"


# -------------------------------------------------------- the two rules ---
def _float24_cases():
    rng = np.random.default_rng(24)
    edge = [0x00000000, 0x80000000, 0x00000001, 0x0000007F, 0x00000080, 0x00000081, 0x007FFFFF, 0x807FFFFF,
            0x00800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F7FFF7F, 0x7F7FFF80, 0x7F800000, 0xFF800000,
            0x7F800001, 0x7F80007F, 0x7F800080, 0xFF8000FF, 0x7FC00000, 0x7FFFFFFF, 0xFFFFFFFF,
            0x3F80007F, 0x3F800080, 0x3F800081, 0x3F8000FF, 0x3F80017F, 0x3F800180, 0x3FFFFF80, 0x3FFFFFFF]
    return np.concatenate([np.array(edge, np.uint32), rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32)])


def test_float24_is_the_numpy_rule(rr):
    bits = _float24_cases()
    got = rr.native.float24(bits.view(np.float32))
    want = E.float24(bits)
    assert np.array_equal(got, want)
    assert np.all(got < (1 << 24))
    # the table's rows: a round-up into infinity truncates; infinities; a NaN stays a NaN
    assert E.float24(np.uint32(0x7F7FFFFF)) == 0x7F7FFF and E.float24(np.uint32(0x7F800000)) == 0x7F8000
    nan = (bits & 0x7F800000 == 0x7F800000) & (bits & 0x007FFFFF != 0)
    assert np.all((want[nan] & 0x7F8000 == 0x7F8000) & (want[nan] & 0x7FFF != 0))
    fin = bits & 0x7F800000 != 0x7F800000
    assert np.all(want[fin] & 0x7F8000 != 0x7F8000)
    # round to nearest: the 24-bit value << 8 is within half a step (0x80) of the bits
    back = want[fin].astype(np.int64) << 8
    assert np.all(np.abs(back - bits[fin].astype(np.int64)) <= 0x100)


def _rle_rows():
    rng = np.random.default_rng(7)
    rows = [bytes([5]), bytes([5, 5]), bytes([5, 5, 5]), bytes([1, 2]), bytes(range(200)), bytes([9]) * 127,
            bytes([9]) * 128, bytes([9]) * 129, bytes([9]) * 256, bytes([9]) * 257, bytes(range(127)),
            bytes(range(128)), bytes(range(129)), bytes([1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 4, 5]),
            bytes([7]) * 130 + bytes(range(130)) + bytes([8]) * 3 + bytes([1, 2]) + bytes([3]) * 2]
    for n in (1, 2, 3, 255, 256, 257, 259, 260, 600, 2400):
        rows.append(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        rows.append(rng.integers(0, 2, n, dtype=np.uint8).tobytes())      # short runs
        rows.append(np.repeat(rng.integers(0, 256, n, dtype=np.uint8), rng.integers(1, 300, n))[:n].tobytes())
    return rows


def test_host_rle_packets_are_the_numpy_rule_and_decode(rr):
    for row in _rle_rows():
        want = E.rle_packets(row)
        assert rr.native.exr_rle(row) == want, len(row)
        assert E.rle_unpack(want, len(row)) == row
        assert len(want) <= len(row) + (len(row) + 126) // 127


def test_rle_decoder_is_strict():
    assert E.rle_unpack(bytes([2, 7]), 3) == bytes([7, 7, 7])
    assert E.rle_unpack(bytes([254, 1, 2]), 2) == bytes([1, 2])
    for bad, n in ((bytes([2, 7]), 2), (bytes([2, 7]), 4), (bytes([254, 1]), 2), (bytes([2]), 3), (bytes([2, 7, 0]), 3)):
        with pytest.raises(E.ExrError):
            E.rle_unpack(bad, n)


def test_run_row_holds_the_runs_it_says():
    words = E.run_row_words()
    pre = np.frombuffer(X.preprocess(E.raw_rows(words)), np.uint8)
    edges = np.flatnonzero(np.concatenate([[True], pre[1:] != pre[:-1], [True]]))
    runs = sorted(set(np.diff(edges).tolist()))
    assert {2, 3, 128, 129, 256} <= set(runs), runs
    assert not np.any(words & 0x7C00 == 0x7C00)  # no infinity or NaN: floats can name every half


# ---------------------------------------------- writer through the reader ---
def _words(kind, w, h, c, full, seed=0):
    return CM.expected_exr(X.make_image(kind, w, h, seed), c, full)


@pytest.mark.parametrize("codec", [E.NONE, E.RLE, E.PXR24])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_writer_round_trips_through_the_strict_reader(codec, full, c):
    for kind in X.KINDS + ["noise"]:
        for w, h in ((1, 1), (3, 17), (129, 16), (257, 33)):
            words = _words(kind, w, h, c, full)
            data, modes = E.write_exr(words, codec)
            px, rmodes, _ = E.read_exr(data, codec)
            assert rmodes == modes
            assert np.array_equal(px, E.expected_words(words, codec, modes)), (kind, w, h)
            if codec == E.NONE:
                assert set(modes) == {"raw"}


def test_reader_refuses_what_is_not_the_file():
    words = _words("flat", 40, 18, 4, False)
    for codec in (E.NONE, E.RLE, E.PXR24):
        data, _ = E.write_exr(words, codec)
        with pytest.raises(E.ExrError):
            E.read_exr(data, E.RLE if codec != E.RLE else E.NONE)  # the attribute
        with pytest.raises(E.ExrError):
            E.read_exr(data + b"\0", codec)
        with pytest.raises(E.ExrError):
            E.read_exr(data[:-1], codec)
        head = len(E.header_bytes(40, 18, 4, False, codec))
        moved = bytearray(data)
        moved[head] ^= 1  # the first offset
        with pytest.raises(E.ExrError):
            E.read_exr(bytes(moved), codec)
    data, _ = E.write_exr(words, E.PXR24)
    broken = bytearray(data)
    broken[-1] ^= 0xFF  # the last chunk's Adler-32
    with pytest.raises(E.ExrError):
        E.read_exr(bytes(broken), E.PXR24)


def test_conditions_hold_for_the_restatement():
    """What the GPU tests rely on, for their seeds: flat codes everywhere; noise of one and
    three channels nowhere; rows that alternate give RLE alternating modes. With four
    channels A = 1 is a constant plane, a quarter of every scanline: noise codes too."""
    import exr_codec_cases as K
    for full in (False, True):
        for c in (1, 3, 4):
            for w, h in ((300, 33), (129, 17)):
                flat, noise, alt = (K.words(k, w, h, c, full) for k in ("flat", "noise", "alternate"))
                for codec in (E.RLE, E.PXR24):
                    assert "raw" not in E.write_exr(flat, codec)[1]
                    modes = E.write_exr(noise, codec)[1]
                    goes_raw = c != 4 and not (codec == E.PXR24 and full)  # PXR24 drops a float's fourth byte
                    assert (set(modes) == {"raw"}) if goes_raw else ("raw" not in modes), (codec, full, c)
                modes = E.write_exr(alt, E.RLE)[1]
                if c != 4:
                    assert modes == ["rle" if y % 2 == 0 else "raw" for y in range(h)]
    img = K.run_row_image()
    pre = np.frombuffer(X.preprocess(E.raw_rows(CM.expected_exr(img, 3, False))), np.uint8)
    edges = np.flatnonzero(np.concatenate([[True], pre[1:] != pre[:-1], [True]]))
    assert {2, 3, 128, 129, 256} <= set(np.diff(edges).tolist())
