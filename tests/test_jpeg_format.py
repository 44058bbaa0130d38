"""JPEG files held against things the coders do not share: a strict reader
written from T.81 (tests/jpeg_reader.py), itself pinned to libjpeg through PIL;
libjpeg's quantiser and Huffman table bytes; and the forward transform in
float64 (tests/jpeg_cases.py) under a derived rounding rule. Here the host
coder (image_io.cpp) writes the files; tests/test_gpu_jpeg_coeffs.py puts the
device coder's through the same checks. profiles/jpeg_checks.md has the
figures each case printed."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as C
import jpeg_reader as R


# ------------------------------------------------- the reader against libjpeg --
def _pil_bytes(a, **kw):
    b = io.BytesIO()
    Image.fromarray(a, "L" if a.ndim == 2 else "RGB").save(b, "JPEG", **kw)
    return b.getvalue()


@pytest.mark.parametrize("optimize", [False, True])
@pytest.mark.parametrize("restart_rows", [0, 1])
@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (37, 29), (64, 48), (33, 17)])
@pytest.mark.parametrize("quality", [30, 90, 100])
def test_reader_accepts_pil_files(w, h, quality, restart_rows, optimize):
    rgb = C.noise_image(w, h, 3 * w + h)[..., :3]
    grey = rgb[..., 0].copy()
    grey[h // 2:, w // 2:] = 200  # a flat part: EOB-only blocks, long runs beside the noise
    data = _pil_bytes(grey, quality=quality, optimize=optimize, restart_marker_rows=restart_rows)
    j = R.read_jpeg(data)
    assert (j.width, j.height, len(j.components)) == (w, h, 1)
    assert j.dri == (restart_rows and (w + 7) // 8) and len(j.intervals) == ((h + 7) // 8 if restart_rows else 1)
    # the float64 IDCT of the reader's coefficients against libjpeg's integer one:
    # IEEE 1180 allows that a peak error of one code, and no more is given here
    ours = np.clip(np.rint(j.idct_pixels()), 0, 255)
    theirs = np.asarray(Image.open(io.BytesIO(data)), np.float64)
    assert np.abs(ours - theirs).max() <= 1
    data = _pil_bytes(np.ascontiguousarray(rgb), quality=quality, subsampling=2, optimize=optimize,
                      restart_marker_rows=restart_rows)
    j = R.read_jpeg(data)
    assert (j.width, j.height) == (w, h) and [c[1:3] for c in j.components] == [(2, 2), (1, 1), (1, 1)]
    assert j.dri == (restart_rows and (w + 15) // 16) and len(j.intervals) == ((h + 15) // 16 if restart_rows else 1)
    assert j.coeffs[0].shape[:2] == (2 * ((h + 15) // 16), 2 * ((w + 15) // 16))


def _restart_file():
    """A PIL file with restart intervals, a stuffed 0xFF and padding bits in it."""
    data = _pil_bytes(np.ascontiguousarray(C.noise_image(40, 40, 1)[..., 0]), quality=95, restart_marker_rows=1)
    j = R.read_jpeg(data)
    assert len(j.intervals) == 5 and sum(i["stuffed"] for i in j.intervals) > 0
    return data, j


def test_reader_refuses_damaged_files():
    data, j = _restart_file()
    scan = data.index(b"\xff\xda")
    cases = {}
    k = data.index(b"\xff\xd1", scan)
    cases["a flipped RST number"] = data[:k + 1] + b"\xd2" + data[k + 2:]
    k = data.index(b"\xff\x00", scan)
    cases["an un-stuffed 0xFF"] = data[:k + 1] + data[k + 2:]
    cases["a truncated scan"] = data[:len(data) - 40]
    cases["a truncated scan with EOI"] = data[:len(data) - 40] + b"\xff\xd9"
    cases["a byte after EOI"] = data + b"\x00"
    cases["a marker inside an interval"] = data[:scan + 20] + b"\xff\xfe" + data[scan + 20:]
    cases["a missing interval"] = data[:data.index(b"\xff\xd3", scan)] + b"\xff\xd9"
    # 0-bit padding: clear the padding bits of the first interval that has some
    first = next(i for i, iv in enumerate(j.intervals) if iv["pad_bits"] > 1 and iv["last_byte"] != 0xFF)
    k = scan
    for _ in range(first + 1):
        k = next(m for m in range(k + 2, len(data)) if data[m] == 0xFF and 0xD0 <= data[m + 1] <= 0xD9)
    pad = j.intervals[first]["pad_bits"]
    assert data[k - 1] == j.intervals[first]["last_byte"]
    cases["0-bit padding"] = data[:k - 1] + bytes([data[k - 1] & ~((1 << pad) - 1) & 0xFF]) + data[k:]
    cases["one 0-bit in the padding"] = data[:k - 1] + bytes([data[k - 1] & 0xFE]) + data[k:]
    for what, bad in cases.items():
        with pytest.raises(R.FormatError):
            R.read_jpeg(bad)
            pytest.fail(f"{what}: accepted")


def _with_dht(data, tc_th, bits, vals):
    """`data` with the DHT of class / id `tc_th` replaced."""
    seg = bytes([tc_th]) + bytes(bits) + bytes(vals)
    new = b"\xff\xc4" + (len(seg) + 2).to_bytes(2, "big") + seg
    for old in R.segments_of(data, 0xC4):
        if old[4] == tc_th:
            return data.replace(old, new)
    raise AssertionError("no such table")


def test_reader_refuses_bad_tables_and_symbols():
    data = _pil_bytes(np.ascontiguousarray(C.noise_image(16, 16, 2)[..., 0]), quality=90)
    j = R.read_jpeg(data)
    dc = R.segments_of(data, 0xC4)[0]
    bits, vals = list(dc[5:21]), list(dc[21:])
    for what, bad in {
        "DC category 12": _with_dht(data, 0x00, bits[:8] + [bits[8] + 1] + bits[9:], vals + [12]),
        "AC category 11": _with_dht(data, 0x10, [0, 1] + [0] * 14, [0x0B]),
        "AC size 0, run 3": _with_dht(data, 0x10, [0, 2] + [0] * 14, [0x00, 0x30]),
        "a symbol twice": _with_dht(data, 0x00, [0, 2] + [0] * 14, [1, 1]),
        "too many codes": _with_dht(data, 0x00, [3] + [0] * 15, [0, 1, 2]),
        "a progressive frame": data.replace(b"\xff\xc0", b"\xff\xc2", 1),
    }.items():
        with pytest.raises(R.FormatError):
            R.read_jpeg(bad)
            pytest.fail(f"{what}: accepted")
    # a code not in the table, and a run past coefficient 63: one-code AC tables
    # over the same scan bytes. DC table: category 0 only ("0"); each block is
    # then "0" + AC symbols.
    small = _with_dht(_with_dht(data, 0x00, [1] + [0] * 15, [0]), 0x10, [1] + [0] * 15, [0xF1])
    small = small[:small.index(b"\xff\xda") + 10]  # up to and including the SOS segment
    assert j.coeffs[0].shape[:2] == (2, 2)
    with pytest.raises(R.FormatError, match="no code of the table"):
        R.read_jpeg(small + b"\x7f" + b"\xff\xd9")  # DC "0", then 1111111: no code
    with pytest.raises(R.FormatError, match="passes coefficient 63"):
        # DC "0", then (run 15, size 1) "0" + one magnitude bit, five times: coefficient 80
        R.read_jpeg(small + bytes([0b00101010, 0b10111111]) + b"\xff\xd9")


# ------------------------------------------------------ independent tables ---
def _host(rr, tmp_path, rgba, quality, mode):
    if mode == "BW":
        rr.encode_image_mode(rgba, str(tmp_path / "h"), "JPEG", quality, "BW")
    else:
        rr.encode_image(rgba, str(tmp_path / "h"), "JPEG", quality)
    return (tmp_path / "h.jpg").read_bytes()


@pytest.mark.parametrize("quality", C.TABLE_QUALITIES)
def test_table_segments_equal_libjpegs(rr, tmp_path, quality):
    img = C.noise_image(16, 16, 0)
    for mode in ("BW", "RGB"):
        ours, pil = _host(rr, tmp_path, img, quality, mode), C.pil_file(quality, mode == "BW")
        assert R.segments_of(ours, 0xDB) == R.segments_of(pil, 0xDB), (mode, "DQT")
        assert R.segments_of(ours, 0xC4) == R.segments_of(pil, 0xC4), (mode, "DHT")
        assert len(R.segments_of(ours, 0xDB)) == (1 if mode == "BW" else 2)
        assert [len(s) - 4 for s in R.segments_of(ours, 0xC4)] == [29, 179, 29, 179][:2 if mode == "BW" else 4]


# ------------------------------------------------------- the coder's files ---
def test_synthesised_luma_blocks(rr, tmp_path):
    img, rows = C.synth_luma(50)
    for mode in ("BW", "RGB"):
        what = f"synth-luma-q50-{mode}"
        j, cov, _ = C.verify(_host(rr, tmp_path, img, 50, mode), img, 50, mode, what)
        C.check_synth_luma(j, cov, rows, what)


def test_synthesised_chroma_blocks(rr, tmp_path):
    img, rows = C.synth_chroma(50)
    j, cov, _ = C.verify(_host(rr, tmp_path, img, 50, "RGB"), img, 50, "RGB", "synth-chroma-q50-RGB")
    C.check_synth_chroma(j, cov, rows, "synth-chroma-q50-RGB")


@pytest.mark.parametrize("mode", ["BW", "RGB"])
def test_full_swing_quality_100(rr, tmp_path, mode):
    img = C.full_swing()
    j, cov, _ = C.verify(_host(rr, tmp_path, img, 100, mode), img, 100, mode, f"full-swing-q100-{mode}")
    C.check_full_swing(cov, mode)


@pytest.mark.parametrize("mode", ["BW", "RGB"])
def test_padded_last_byte_of_0xff(rr, tmp_path, mode):
    img = C.padff_image(mode)
    data = _host(rr, tmp_path, img, 90, mode)
    j, _, _ = C.verify(data, img, 90, mode, f"padded-0xff-{mode}")
    C.check_padded_ff(data, j, mode)


_PLAIN = C.plain_cases()


@pytest.mark.parametrize("case", [c for c in _PLAIN if not c[0].startswith("ragged")], ids=lambda c: c[0])
def test_host_file_against_float64(rr, tmp_path, case):
    what, mode, quality, build = case
    img = build()
    C.verify(_host(rr, tmp_path, img, quality, mode), img, quality, mode, what)


@pytest.mark.parametrize("w", C.RAGGED)
def test_ragged_edges(rr, tmp_path, w):
    for what, mode, quality, build in _PLAIN:
        if what.startswith(f"ragged{w}x"):
            img = build()
            C.verify(_host(rr, tmp_path, img, quality, mode), img, quality, mode, what)


def test_inputs_are_what_they_claim():
    """distinct_image: every pixel at least 33 codes from its eight neighbours in
    every channel; the rows257 inputs have more than 256 MCU rows."""
    a = C.distinct_image(33, 33)[..., :3].astype(int)
    for dy, dx in ((0, 1), (1, 0), (1, 1)):
        assert np.abs(a[dy:, dx:] - a[:33 - dy, :33 - dx]).min() >= 33
    assert np.abs(a[1:, :-1] - a[:-1, 1:]).min() >= 33
    sizes = {c[0]: c[3]().shape for c in _PLAIN if c[0].startswith("rows257")}
    assert sizes == {"rows257-BW": (2056, 8, 4), "rows257-RGB": (4112, 16, 4)}
