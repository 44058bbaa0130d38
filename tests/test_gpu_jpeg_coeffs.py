"""The device JPEG coder (jpeg.hip) on the inputs of tests/jpeg_cases.py: its
bytes equal the host coder's, and, in their own right, pass the strict reader
of tests/jpeg_reader.py and the float64 rule, so a failure names the block and
the coefficient. The inputs reach what the 1080p cases of test_gpu_jpeg.py do
not: chains of ZRLs in both AC tables, blocks without EOB, tiny blocks sharing
an output word, DC category 11 and AC category 10, both branches of the
quality scaling, ragged edges over pixels that all differ, more than 256
restart intervals (k_jpeg_finish's strided sum), a frame 65535 wide, and an
interval whose padded last byte is 0xFF."""
import pytest

import jpeg_cases as C

pytestmark = pytest.mark.gpu


def _host(rr, tmp_path, rgba, quality, mode):
    if mode == "BW":
        rr.encode_image_mode(rgba, str(tmp_path / "h"), "JPEG", quality, "BW")
    else:
        rr.encode_image(rgba, str(tmp_path / "h"), "JPEG", quality)
    return (tmp_path / "h.jpg").read_bytes()


def _device(ctx, rr, tmp_path, rgba, quality, mode, what):
    """Device bytes of `rgba`, checked: -> (bytes, Jpeg, coverage)."""
    dev = ctx.encode_device("JPEG", rgba, 8, mode, quality=quality)
    if mode == "RGB":
        assert ctx.jpeg_device(rgba, quality) == dev, what
    j, cov, _ = C.verify(dev, rgba, quality, mode, what + " (device)")
    host = _host(rr, tmp_path, rgba, quality, mode)
    assert len(dev) == len(host) and dev == host, what
    return dev, j, cov


def test_synthesised_luma_blocks(ctx, rr, tmp_path):
    img, rows = C.synth_luma(50)
    for mode in ("BW", "RGB"):
        what = f"synth-luma-q50-{mode}"
        _, j, cov = _device(ctx, rr, tmp_path, img, 50, mode, what)
        C.check_synth_luma(j, cov, rows, what)


def test_synthesised_chroma_blocks(ctx, rr, tmp_path):
    img, rows = C.synth_chroma(50)
    _, j, cov = _device(ctx, rr, tmp_path, img, 50, "RGB", "synth-chroma-q50-RGB")
    C.check_synth_chroma(j, cov, rows, "synth-chroma-q50-RGB")


@pytest.mark.parametrize("mode", ["BW", "RGB"])
def test_full_swing_quality_100(ctx, rr, tmp_path, mode):
    img = C.full_swing()
    _, _, cov = _device(ctx, rr, tmp_path, img, 100, mode, f"full-swing-q100-{mode}")
    C.check_full_swing(cov, mode)


@pytest.mark.parametrize("mode", ["BW", "RGB"])
def test_padded_last_byte_of_0xff(ctx, rr, tmp_path, mode):
    img = C.padff_image(mode)
    dev, j, _ = _device(ctx, rr, tmp_path, img, 90, mode, f"padded-0xff-{mode}")
    C.check_padded_ff(dev, j, mode)


_PLAIN = C.plain_cases()


@pytest.mark.parametrize("case", [c for c in _PLAIN if not c[0].startswith("ragged")], ids=lambda c: c[0])
def test_device_file_against_float64(ctx, rr, tmp_path, case):
    """The wide BW cases are the first BW frames of more than 1024 blocks any
    test codes on the device; they found the DC codes k_jpeg_emit lost there
    (profiles/jpeg_checks.md)."""
    what, mode, quality, build = case
    _device(ctx, rr, tmp_path, build(), quality, mode, what)


@pytest.mark.parametrize("w", C.RAGGED)
def test_ragged_edges(ctx, rr, tmp_path, w):
    for what, mode, quality, build in _PLAIN:
        if what.startswith(f"ragged{w}x"):
            _device(ctx, rr, tmp_path, build(), quality, mode, what)


@pytest.mark.parametrize("mode", ["BW", "RGB"])
def test_no_state_leaks_between_frames(ctx, mode):
    """257 MCU rows, then one, then the 257 again in one context: the `ready` and
    `row_bits` words the first frame left behind do not reach the later ones."""
    tall = next(c for c in _PLAIN if c[0] == f"rows257-{mode}")[3]()
    tiny = C.noise_image(1, 1, 9)
    first = ctx.encode_device("JPEG", tall, 8, mode, quality=90)
    small = ctx.encode_device("JPEG", tiny, 8, mode, quality=90)
    assert ctx.encode_device("JPEG", tall, 8, mode, quality=90) == first
    assert ctx.encode_device("JPEG", tiny, 8, mode, quality=90) == small
    C.verify(first, tall, 90, mode, f"rows257-{mode} (device)")
    C.verify(small, tiny, 90, mode, f"1x1-{mode} (device)")
