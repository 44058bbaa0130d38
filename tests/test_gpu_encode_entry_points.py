"""The coders' inspection entry points share one body (rr_debug.cpp debug_encode): the five
older ones (png_device, png16_device, jpeg_device, exr_device, exr32_device) give the bytes of
encode_device at the same format and depth, except that the two EXR ones keep the image's own
alpha where encode_device writes A = 1. And an inspection call leaves the frame slots alone: a
frame rendered after one is the file it was before.

Sizes: 64 x 17 is two deflate bands of 16 rows, the second a single row; 33 x 33 is three bands
at an odd width."""
import numpy as np
import pytest

import exr32_reader as F
import exr_reader as X
from conftest import scene_path

pytestmark = pytest.mark.gpu

S04 = scene_path("04_very-simple-standin.rrscene")
SIZES = [(64, 17), (33, 33)]


@pytest.fixture(scope="module")
def c(rr):
    with rr.RenderContext(0) as ctx:
        yield ctx


def image8(w, h):
    rng = np.random.default_rng(1000 * w + h)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[: h // 2, : w // 2] = (200, 30, 90, 255)  # a flat part, so that the coders find matches too
    return img


def image_float(w, h):
    """Means in [0, 1.5) with an alpha that is never 1 and exact in half floats (k / 64)."""
    rng = np.random.default_rng(2000 * w + h)
    img = rng.random((h, w, 4), dtype=np.float32) * np.float32(1.5)
    img[..., 3] = rng.integers(8, 56, (h, w)).astype(np.float32) / np.float32(64)
    img[: h // 2, : w // 2, :3] = (0.25, 0.5, 1.25)
    return img


@pytest.mark.parametrize("w,h", SIZES)
def test_png8_and_jpeg_entry_points_are_encode_device(c, w, h):
    img = image8(w, h)
    assert c.png_device(img) == c.encode_device("PNG", img, 8, 0)
    assert c.jpeg_device(img, 90) == c.encode_device("JPEG", img, 8, 0, quality=90)


@pytest.mark.parametrize("w,h", SIZES)
def test_png16_entry_point_is_encode_device(c, w, h):
    f = image_float(w, h)
    assert c.png16_device(f) == c.encode_device("PNG", f, 16, 0)


@pytest.mark.parametrize("w,h", SIZES)
def test_exr_entry_points_keep_alpha_and_encode_device_writes_one(c, w, h):
    f = image_float(w, h)
    own, _, _, _ = X.read_exr(c.exr_device(f))
    one, _, _, _ = X.read_exr(c.encode_device("OPEN_EXR", f, 16, 0))
    assert own.shape == one.shape == (h, w, 4)
    assert np.array_equal(own[..., 3], f[..., 3].astype(np.float16).view(np.uint16))
    assert np.all(one[..., 3] == 0x3C00)
    assert np.array_equal(own[..., :3], one[..., :3])
    own32, _, _, _ = F.read_exr32(c.exr32_device(f))
    one32, _, _, _ = F.read_exr32(c.encode_device("OPEN_EXR", f, 32, 0))
    assert own32.shape == one32.shape == (h, w, 4)
    assert np.array_equal(own32[..., 3], f[..., 3].view(np.uint32))
    assert np.all(one32[..., 3] == 0x3F800000)
    assert np.array_equal(own32[..., :3], one32[..., :3])
    assert np.array_equal(own32[..., :3], f[..., :3].view(np.uint32))


def test_inspection_call_leaves_the_frame_slots_alone(rr, c, tmp_path):
    scene = c.load_scene(S04)
    params = rr.default_params(width=64, height=36, spp=4)

    def frame(name):
        c.render_frame(scene, 30, params, str(tmp_path / name), "JPEG", 90)
        return (tmp_path / (name + ".jpg")).read_bytes()

    before = frame("before")
    assert before[:2] == b"\xff\xd8"
    grey = c.encode_device("JPEG", image8(33, 33), 8, "BW", quality=50)
    assert grey[:2] == b"\xff\xd8" and grey != before
    # one frame for every slot (RR_MAX_FRAMES_IN_FLIGHT = 3), whichever the call may have touched
    for k in range(3):
        assert frame(f"after{k}") == before
    scene.close()
