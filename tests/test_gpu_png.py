"""The device PNG path (png.hip + deflate.hip: Sub filter, LZ77 over the distances 1 / 4 /
row above, one dynamic-Huffman block per 16-row band with a stored fallback)
writes files that decode to exactly the input pixels, deterministically, within
size conditions that only real dynamic codes and working matches meet; rendered
frames take it when rr_set_device_png is on and keep the host encoder's bytes
when it is off; frames in flight do not share its buffers. What the files
contain — tokens, code lengths, stored or dynamic per band — is pinned to
oracle/png_oracle.py in tests/test_gpu_png_tokens.py."""
import zlib

import numpy as np
import pytest
from PIL import Image

from conftest import scene_path

pytestmark = pytest.mark.gpu


def _img(kind, w, h, seed=0):
    rng = np.random.default_rng(seed)
    if kind in ("noise", "noise4"):
        a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    elif kind == "flat":
        a = np.full((h, w, 4), 77, np.uint8)
    elif kind == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        a = np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) % 256), np.full_like(x, 255)],
                     -1).astype(np.uint8)
    elif kind == "sparse":  # mostly flat with isolated spikes
        a = np.full((h, w, 4), 128, np.uint8)
        m = rng.random((h, w)) < 0.01
        a[m, :3] = 255
    if kind != "noise4":  # noise4: the alpha channel is random too
        a[..., 3] = 255
    return a


def _idat(data):
    i = data.index(b"IDAT")
    ln = int.from_bytes(data[i - 4:i], "big")
    return data[i + 4:i + 4 + ln]


def _check_file(data, img, tmp_path, name="f.png"):
    h, w = img.shape[:2]
    path = tmp_path / name
    path.write_bytes(data)
    back = np.asarray(Image.open(path).convert("RGBA"))
    assert np.array_equal(back, img)
    raw = zlib.decompress(_idat(data))  # raises on a bad Adler-32 or block structure
    assert len(raw) == (4 * w + 1) * h
    rows = np.frombuffer(raw, np.uint8).reshape(h, 4 * w + 1)
    assert rows[:, 0].max() <= 4
    return len(raw)


CASES = [("noise", 1, 1), ("noise", 8, 8), ("noise", 17, 9), ("flat", 64, 48), ("gradient", 333, 257),
         ("sparse", 320, 200), ("noise", 256, 64), ("flat", 1, 300), ("gradient", 8200, 3), ("noise4", 4100, 16),
         ("sparse", 1920, 1080)]


@pytest.mark.parametrize("kind,w,h", CASES)
def test_device_png_round_trip(ctx, tmp_path, kind, w, h):
    img = _img(kind, w, h, seed=w * 7 + h)
    data = ctx.png_device(img)
    raw = _check_file(data, img, tmp_path)
    print(f"{kind} {w}x{h}: file {len(data)} bytes, raw {raw}, ratio {len(data) / raw:.4f}")
    assert len(data) <= raw + raw / 100 + 1024  # the stored fallback bounds every band
    if (kind, w, h) == ("gradient", 333, 257):
        assert len(data) < 0.25 * raw  # residuals are almost all 0 / 1: per-band dynamic codes
    assert ctx.png_device(img) == data  # same image, same bytes


def test_device_png_flat_frame_needs_matches(ctx, tmp_path):
    """Huffman codes alone cannot go below one bit a byte (0.125 of raw)."""
    img = _img("flat", 1920, 1080)
    data = ctx.png_device(img)
    raw = _check_file(data, img, tmp_path)
    print(f"flat 1920x1080: file {len(data)} bytes, raw {raw}, ratio {len(data) / raw:.5f}")
    assert len(data) < 0.02 * raw


def _scene(ctx, which):
    return ctx.load_scene(scene_path("04_very-simple-standin.rrscene" if which == "04vs"
                                     else "02_physics-standin.rrscene"))


@pytest.mark.parametrize("which,frame", [("04vs", 9), ("02", 90)])
def test_rendered_frame_device_png(ctx, rr, tmp_path, which, frame):
    """Tile path (04vs) and split path (02): the device-coded file decodes to
    the frame's pixels; with the switch off the file is the host encoder's."""
    s = _scene(ctx, which)
    try:
        p = rr.default_params(spp=4, width=250, height=141)
        _, rgba, _ = ctx.render_to_memory(s, frame, p)
        ctx.set_device_png(True)
        _, stats = ctx.render_frame(s, frame, p, str(tmp_path / "dev"), "PNG")
        data = (tmp_path / "dev.png").read_bytes()
        assert stats.output_bytes == len(data)
        _check_file(data, rgba, tmp_path, "copy.png")
        ctx.set_device_png(False)
        _, stats = ctx.render_frame(s, frame, p, str(tmp_path / "host"), "PNG")
        rr.encode_image(rgba, str(tmp_path / "ref"), "PNG")
        host = (tmp_path / "host.png").read_bytes()
        assert host == (tmp_path / "ref.png").read_bytes()
        assert stats.output_bytes == len(host)
    finally:
        ctx.set_device_png(False)
        s.close()


def test_frames_in_flight_keep_their_own_png_buffers(ctx, rr, tmp_path):
    s = _scene(ctx, "04vs")
    try:
        p = rr.default_params(spp=4, width=250, height=141)
        frames = [3, 4, 5]
        want = {f: ctx.render_to_memory(s, f, p)[1] for f in frames}
        assert not np.array_equal(want[3], want[5])
        ctx.set_device_png(True)
        tickets = [ctx.submit_frame(s, f, p, str(tmp_path / f"f{f}"), "PNG") for f in frames]
        for t in tickets:
            ctx.complete_frame(t)
        for f in frames:
            _check_file((tmp_path / f"f{f}.png").read_bytes(), want[f], tmp_path, f"copy{f}.png")
    finally:
        ctx.set_device_png(False)
        s.close()
