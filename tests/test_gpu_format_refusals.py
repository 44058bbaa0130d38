"""What rr_debug_encode_device refuses, word for word: an image of the wrong type, a depth the
format does not have, a name nobody writes, and a size outside a coder's range. The texts are
the ones these calls gave before the formats were stated in one table (csrc/formats.hpp) and
are written out here; every call is refused before any launch."""
import ctypes

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu

IMG8 = np.zeros((8, 8, 4), np.uint8)
IMGF = np.zeros((8, 8, 4), np.float32)

TAKES8 = "{} takes an RGBA8 image at depth 8"
HDR_TAKES = "HDR takes a float RGBA image at depth 32"
PNG8_TAKES = "8-bit PNG takes an RGBA8 image"
FLOAT_TAKES = "16-bit PNG and OPEN_EXR take a float RGBA image"
NO_SUCH = "no such format and depth: '{}' at {}"

# (format, depth, float image?, the refusal)
WRONG = [
    # the formats of one coder: the other image type, then a depth they do not have
    ("JPEG", 8, True, TAKES8.format("JPEG")), ("JPEG", 0, True, TAKES8.format("JPEG")),
    ("JPEG", 16, False, TAKES8.format("JPEG")), ("JPEG", 32, True, TAKES8.format("JPEG")),
    ("TARGA", 8, True, TAKES8.format("TARGA")), ("TARGA", 16, False, TAKES8.format("TARGA")),
    ("TARGA_RAW", 0, True, TAKES8.format("TARGA")), ("TARGA_RAW", 32, False, TAKES8.format("TARGA")),
    ("IRIS", 8, True, TAKES8.format("IRIS")), ("IRIS", 16, False, TAKES8.format("IRIS")),
    ("WEBP", 8, True, TAKES8.format("WEBP")), ("WEBP", 32, False, TAKES8.format("WEBP")),
    ("HDR", 32, False, HDR_TAKES), ("HDR", 0, False, HDR_TAKES), ("HDR", 16, True, HDR_TAKES), ("HDR", 8, False, HDR_TAKES),
    # PNG and OPEN_EXR, where the depth chooses the coder
    ("PNG", 8, True, PNG8_TAKES), ("PNG", 0, True, PNG8_TAKES),
    ("PNG", 16, False, FLOAT_TAKES), ("PNG", 32, False, FLOAT_TAKES), ("PNG", 12, False, FLOAT_TAKES),
    ("PNG", 32, True, NO_SUCH.format("PNG", 32)), ("PNG", 12, True, NO_SUCH.format("PNG", 12)),
    ("OPEN_EXR", 0, False, FLOAT_TAKES), ("OPEN_EXR", 16, False, FLOAT_TAKES), ("OPEN_EXR", 32, False, FLOAT_TAKES),
    ("OPEN_EXR", 8, False, FLOAT_TAKES), ("OPEN_EXR", 8, True, NO_SUCH.format("OPEN_EXR", 8)),
    ("OPEN_EXR", 24, True, NO_SUCH.format("OPEN_EXR", 24)),
    # names nobody writes
    ("TIFF", 8, False, FLOAT_TAKES), ("TIFF", 8, True, NO_SUCH.format("TIFF", 8)), ("TIFF", 0, True, NO_SUCH.format("TIFF", 0)),
    ("jpeg", 8, True, NO_SUCH.format("jpeg", 8)), ("", 16, True, NO_SUCH.format("", 16)),
]

TARGA_RANGE = "image size outside the TARGA format's range (65535 x 65535, a body below 2 GB)"
IRIS_RANGE = "image size outside the IRIS format's range (65535 x 65535, a body bound below 2 GB)"
WEBP_RANGE = "image size outside the WEBP format's range (16384 x 16384, a payload bound below 2 GB)"

# (format, depth, float image?, width, height, the refusal): the plan refuses, nothing is launched
# and the 8 x 8 image is not read
RANGE = [
    ("TARGA", 8, False, 65536, 1, TARGA_RANGE), ("TARGA_RAW", 8, False, 65536, 1, TARGA_RANGE),
    ("TARGA", 0, False, 1, 65536, TARGA_RANGE),
    ("IRIS", 8, False, 65536, 1, IRIS_RANGE), ("IRIS", 0, False, 1, 65536, IRIS_RANGE),
    ("WEBP", 8, False, 16385, 1, WEBP_RANGE), ("WEBP", 0, False, 1, 16385, WEBP_RANGE),
    ("HDR", 32, True, 65536, 16384, "image size outside the HDR coder's range (a body bound below 2 GB)"),
    ("JPEG", 8, False, 65536, 1, "image size outside the JPEG format's range"),
    ("PNG", 8, False, (1 << 20) + 1, 1, "image size outside the device PNG encoder's range"),
    ("PNG", 16, True, (1 << 19) + 1, 1, "image size outside the device 16-bit PNG encoder's range"),
    ("OPEN_EXR", 16, True, (1 << 19) + 1, 1, "image size outside the device EXR encoder's range"),
    ("OPEN_EXR", 32, True, (1 << 18) + 1, 1, "image size outside the device 32-bit EXR encoder's range"),
]


def _refused(ctx, rr, fmt, depth, is_float, w, h, mode=4):
    img = IMGF if is_float else IMG8
    n = ctypes.c_uint64()
    rc = rr.lib().rr_debug_encode_device(ctx.handle, fmt.encode(), depth, mode, img.ctypes.data_as(ctypes.c_void_p),
                                         int(is_float), w, h, 0, ctypes.c_float(1.0), 90, None, 0, ctypes.byref(n))
    return rc, rr.lib().rr_last_error(ctx.handle).decode()


def test_refusal_texts(ctx, rr, tmp_path):
    for fmt, depth, is_float, text in WRONG:
        assert _refused(ctx, rr, fmt, depth, is_float, 8, 8) == (rr.native.RR_EINVAL, text), (fmt, depth, is_float)
    for fmt, depth, is_float, w, h, text in RANGE:
        for mode in (0, 1, 3, 4):
            assert _refused(ctx, rr, fmt, depth, is_float, w, h, mode) == (rr.native.RR_EINVAL, text), (fmt, w, h, mode)
    assert set(fmt for fmt, *_ in WRONG if fmt in rr.EXTENSIONS) == set(rr.EXTENSIONS)  # every format was asked
    # the three refusals that list the formats: a submitted frame's, and the host coders' two
    s = ctx.load_scene(scene_path("04_very-simple-standin.rrscene"))
    try:
        with pytest.raises(rr.RRError) as e:
            ctx.submit_frame(s, 3, rr.default_params(spp=1, width=8, height=8), str(tmp_path / "f"), "TIFF", 90)
    finally:
        s.close()
    assert e.value.code == rr.native.RR_ENOTSUP and str(e.value).endswith(
        ": unsupported output format 'TIFF' (JPEG, PNG, OPEN_EXR, TARGA, TARGA_RAW, HDR, IRIS and WEBP are supported)")
    for fmt, text in (("HDR", "unsupported output format 'HDR' for an RGBA8 image: it needs the float film (JPEG, PNG, "
                              "TARGA, TARGA_RAW, IRIS and WEBP are supported here)"),
                      ("OPEN_EXR", "unsupported output format 'OPEN_EXR' for an RGBA8 image: it needs the float film "
                                   "(JPEG, PNG, TARGA, TARGA_RAW, IRIS and WEBP are supported here)"),
                      ("TIFF", "unsupported output format 'TIFF' (JPEG, PNG, TARGA, TARGA_RAW, IRIS and WEBP are "
                               "supported here; OPEN_EXR and HDR need the float film)")):
        with pytest.raises(rr.RRError) as e:
            rr.encode_image_mode(IMG8, str(tmp_path / "h"), fmt, 90, 4)
        assert e.value.code == rr.native.RR_ENOTSUP and str(e.value).endswith(": " + text), fmt
    assert not list(tmp_path.iterdir())
