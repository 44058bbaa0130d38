"""rr_set_exr_codec on the device: NONE, RLE and PXR24 files of
rr_debug_encode_device("OPEN_EXR", 16 | 32, mode, ...) and of rendered frames
against the restatement and the strict reader of tests/exr_codecs.py.

NONE and RLE files equal the restatement's byte for byte. A PXR24 file's coded
chunks are deflate streams of the device coder, whose token choice no zlib level
restates: the file is compared chunk by chunk after inflating (the chunk
positions, and what every stream holds), raw chunks byte for byte.

The noise condition "only raw chunks" holds for one and three channels. With
four, rr_debug_encode_device writes A = 1: a constant plane, a quarter of every
scanline, which RLE packs and deflate removes, so a four-channel noise file has
coded chunks; there the RLE modes are the restatement's and PXR24 has no raw chunk.
Nor has a FLOAT PXR24 file of noise: its streams hold 3 bytes of a sample's 4 (raw
FLOAT chunks come from the widths 1 and 2). The flat FLOAT image is black: a flat
row of floats whose bytes differ alternates two byte values after the reorder, has
no run of three, and RLE stores it raw (tests/exr_codec_cases.py)."""
import os

import numpy as np
import pytest

import exr_codec_cases as K
import exr_codecs as E
import exr_reader as X
from conftest import SCENES

pytestmark = pytest.mark.gpu

CODECS = {E.NONE: "NONE", E.RLE: "RLE", E.PXR24: "PXR24"}
MODES = {1: "BW", 3: "RGB", 4: "RGBA"}


@pytest.fixture
def codec_ctx(ctx):
    yield ctx
    ctx.set_exr_codec("")
    ctx.set_exr_depth(0)
    ctx.set_color_mode(0)


def _encode(ctx, img, codec, c, full):
    ctx.set_exr_codec(CODECS[codec])
    return ctx.encode_device("OPEN_EXR", img, 32 if full else 16, MODES[c])


def _check(ctx, kind, w, h, codec, c, full, seed=0, img=None):
    """The device file of the image against the restatement; -> (device modes, restatement's modes)."""
    img = K.image(kind, w, h, full, seed) if img is None else img
    with np.errstate(all="ignore"):
        words = K.CM.expected_exr(img, c, full)
    data = _encode(ctx, img, codec, c, full)
    ref, ref_modes = E.write_exr(words, codec)
    px, modes, chunks = E.read_exr(data, codec)  # the strict reader accepts it
    what = f"{CODECS[codec]} {kind} {w}x{h} C={c} {'FLOAT' if full else 'HALF'}"
    if codec != E.PXR24:
        assert data == ref, what
        assert modes == ref_modes, what
    else:  # chunk by chunk after inflating
        for (y, mode, content), row0 in zip(chunks, range(0, h, X.ROWS)):
            part = words[row0:row0 + X.ROWS]
            assert y == row0
            assert content == (E.raw_rows(part) if mode == "raw" else E.pxr24_front(part)), (what, y)
        rebuilt = E.assemble(w, h, c, full, codec, [(y, data_of) for y, data_of in _payloads(data, codec)])
        assert rebuilt == data, what
    assert np.array_equal(px, E.expected_words(words, codec, modes)), what
    return modes, ref_modes


def _payloads(data, codec):
    """[(y, payload)] of a file the strict reader has accepted."""
    import struct
    px, modes, chunks = E.read_exr(data, codec)
    h, w, c = px.shape
    head = len(E.header_bytes(w, h, c, px.dtype == np.uint32, codec))
    offs = struct.unpack_from(f"<{len(chunks)}Q", data, head)
    out = []
    for o in offs:
        y, size = struct.unpack_from("<ii", data, o)
        out.append((y, data[o + 8:o + 8 + size]))
    return out


@pytest.mark.parametrize("full", [False, True], ids=["half", "float"])
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("codec", [E.NONE, E.RLE, E.PXR24], ids=["none", "rle", "pxr24"])
def test_files_are_the_restatements(codec_ctx, codec, c, full):
    """Every size of the table, as flat, noise and alternating rows; make_image's kinds at 300 x 33."""
    for k, (w, h) in enumerate(K.SIZES):
        for kind in ("flat", "noise", "alternate"):
            _check(codec_ctx, kind, w, h, codec, c, full, seed=k)
    for kind in X.KINDS:
        _check(codec_ctx, kind, 300, 33, codec, c, full)
    if full:
        _check(codec_ctx, "float_edges", 300, 33, codec, c, full)


@pytest.mark.parametrize("full", [False, True], ids=["half", "float"])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_chunk_modes_are_conditions(codec_ctx, c, full):
    """Flat: no raw chunk. Noise: only raw chunks (one and three channels; the module's
    docstring says what four give). Alternating rows: RLE's modes are the restatement's,
    which for one and three channels alternate."""
    for w, h in ((300, 33), (129, 17), (3, 16)):
        for codec in (E.RLE, E.PXR24):
            modes, _ = _check(codec_ctx, "flat", w, h, codec, c, full)
            if w > 3:  # three pixels: a run packet saves nothing of a scanline that short
                assert "raw" not in modes, (codec, w, h)
            modes, ref = _check(codec_ctx, "noise", w, h, codec, c, full)
            if c != 4 and not (codec == E.PXR24 and full):
                assert set(modes) == {"raw"}, (codec, w, h)
            elif codec == E.RLE:
                assert modes == ref
            elif w > 3:  # A = 1, or a FLOAT chunk's 3 bytes of 4: the stream is shorter
                assert "raw" not in modes
        modes, ref = _check(codec_ctx, "alternate", w, h, E.RLE, c, full)
        assert modes == ref
        if c != 4 and w > 3:
            assert modes == ["rle" if y % 2 == 0 else "raw" for y in range(h)]


def test_runs_of_exact_lengths(codec_ctx):
    """A row whose predicted bytes hold runs of exactly 2, 3, 128, 129 and 256 equal bytes."""
    img = K.run_row_image()
    modes, _ = _check(codec_ctx, "runs", img.shape[1], 1, E.RLE, 3, False, img=img)
    assert modes == ["rle"]


def test_float24_values_in_coded_chunks(codec_ctx):
    """FLOAT with PXR24: coded chunks decode to float24 << 8, infinities and NaNs included."""
    img = K.image("float_edges", 300, 33, True)
    data = _encode(codec_ctx, img, E.PXR24, 3, True)
    px, modes, _ = E.read_exr(data, E.PXR24)
    assert "pxr24" in modes
    words = K.CM.expected_exr(img, 3, True)
    assert np.array_equal(px, E.expected_words(words, E.PXR24, modes))
    assert np.any(px != words)  # the rounding is there


# ------------------------------------------------------- rendered frames ---
def _render(ctx, s, rr, tmp_path, name, depth):
    p = rr.default_params(spp=4, width=64, height=48)
    ctx.set_exr_depth(depth)
    ctx.render_frame(s, 9, p, str(tmp_path / name), "OPEN_EXR", 0)
    return (tmp_path / (name + ".exr")).read_bytes()


@pytest.mark.parametrize("depth", [16, 32])
def test_rendered_frames_hold_the_zip_files_pixels(codec_ctx, rr, tmp_path, depth):
    ctx = codec_ctx
    s = ctx.load_scene(os.path.join(SCENES, "04_very-simple-standin.rrscene"))
    try:
        zip0 = _render(ctx, s, rr, tmp_path, "zip0", depth)  # before any setter was called with a codec
        want, _ = K.CM.read_exr(zip0)
        for codec, name in CODECS.items():
            ctx.set_exr_codec(name)
            data = _render(ctx, s, rr, tmp_path, name, depth)
            assert ctx.last_warning() == ""
            px, modes, _ = E.read_exr(data, codec)
            assert np.array_equal(px, E.expected_words(want, codec, modes)), name
            assert data == E.write_exr(want, codec)[0] or codec == E.PXR24
        ctx.set_exr_codec("ZIP")
        assert _render(ctx, s, rr, tmp_path, "zip1", depth) == zip0
        ctx.set_exr_codec("")
        assert _render(ctx, s, rr, tmp_path, "zip2", depth) == zip0
    finally:
        s.close()


def test_frames_in_flight_keep_the_codec_of_their_submit(codec_ctx, rr, tmp_path):
    ctx = codec_ctx
    s = ctx.load_scene(os.path.join(SCENES, "04_very-simple-standin.rrscene"))
    try:
        p = rr.default_params(spp=4, width=64, height=48)
        tickets = []
        for name in ("RLE", "NONE", "ZIP", "PXR24"):
            ctx.set_exr_codec(name)
            tickets.append(ctx.submit_frame(s, 9, p, str(tmp_path / name), "OPEN_EXR"))
            if len(tickets) == 2:  # two pending, then the next two
                for t in tickets:
                    ctx.complete_frame(t)
                tickets = []
        for t in tickets:
            ctx.complete_frame(t)
        want, _ = K.CM.read_exr((tmp_path / "ZIP.exr").read_bytes())
        for codec, name in CODECS.items():
            px, modes, _ = E.read_exr((tmp_path / (name + ".exr")).read_bytes(), codec)
            assert np.array_equal(px, E.expected_words(want, codec, modes)), name
    finally:
        s.close()


# --------------------------------------------------------------- fallback ---
@pytest.mark.parametrize("name", ["ZIPS", "PIZ", "DWAA"])
def test_codecs_not_built_fall_back_to_zip_and_say_so(codec_ctx, rr, name):
    ctx = codec_ctx
    img = X.make_image("gradient", 40, 20)
    ctx.set_exr_codec("ZIP")
    want = ctx.encode_device("OPEN_EXR", img, 16, "RGBA")
    ctx.set_exr_codec(getattr(rr.native, "RR_EXR_CODEC_" + name))
    assert ctx.encode_device("OPEN_EXR", img, 16, "RGBA") == want
    w = ctx.last_warning()
    assert name in w and "ZIP" in w


def test_values_outside_the_setting_are_refused(codec_ctx, rr):
    for bad in (99, -1, 11):
        with pytest.raises(rr.native.RRError) as e:
            codec_ctx.set_exr_codec(bad)
        assert e.value.code == rr.native.RR_EINVAL


@pytest.mark.parametrize("depth,w", [(16, (1 << 19) + 1), (32, (1 << 18) + 1)])
def test_widths_outside_the_range_are_refused(codec_ctx, rr, depth, w):
    """The ZIP coder's range at the same depth and its refusal text, before any launch."""
    ctx = codec_ctx
    img = np.zeros((1, w, 4), np.float32)
    ctx.set_exr_codec("ZIP")
    with pytest.raises(rr.native.RRError) as z:
        ctx.encode_device("OPEN_EXR", img, depth, "RGBA")
    for name in ("RLE", "NONE", "PXR24"):
        ctx.set_exr_codec(name)
        with pytest.raises(rr.native.RRError) as e:
            ctx.encode_device("OPEN_EXR", img, depth, "RGBA")
        assert e.value.code == rr.native.RR_EINVAL and str(e.value) == str(z.value)
