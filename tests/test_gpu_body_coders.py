"""The TARGA, HDR, IRIS and WEBP device coders share one scratch buffer and one
pinned stream per frame slot (device.hpp body_scratch, frame.hpp CodedOut): calls
of the four on one context, the buffers growing and then reused below their
capacity, each give the host coder's file."""
import ctypes

import numpy as np
import pytest

import iris as I

pytestmark = pytest.mark.gpu


def _device_file(ctx, rr, fmt, img, c):
    """One rr_debug_encode_device call; the buffer is above every format's bound
    (IRIS at 9 bytes a row-plane is the longest: 19 bytes for 9)."""
    is_float = img.dtype == np.float32
    h, w = img.shape[:2]
    out = np.zeros(4096 + 16 * 4 * w * h, np.uint8)
    n = ctypes.c_uint64()
    rc = rr.lib().rr_debug_encode_device(ctx.handle, fmt.encode(), 0, c, img.ctypes.data_as(ctypes.c_void_p),
                                         int(is_float), w, h, 0, ctypes.c_float(1.0), 100,
                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), out.size, ctypes.byref(n))
    assert rc == 0, rr.lib().rr_last_error(ctx.handle)
    assert n.value <= out.size
    return out[:n.value].tobytes()


def _host_file(rr, tmp_path, fmt, img, c):
    if fmt == "HDR":
        return rr.hdr_host(img, c)
    rr.encode_image_mode(img, str(tmp_path / "h"), fmt, 100, c)
    return (tmp_path / ("h" + rr.EXTENSIONS[fmt])).read_bytes()


def test_formats_in_turn_on_one_context(rr, tmp_path):
    """IRIS, TARGA, TARGA_RAW, HDR, WEBP, IRIS on a fresh context, large and small
    in turn. The buffers grow at the first call and again at the WEBP call (its
    residuals, records and 60-bit-a-pixel bound are above a one-channel IRIS
    file's records); the calls between and the last reuse them below capacity."""
    dev = I.device_images(256)
    across = np.ascontiguousarray(dev["across steps"])  # 808 x 7
    tall = np.ascontiguousarray(dev["tall 9x700"])
    row = np.ascontiguousarray(tall[:1])  # 9 x 1
    rng = np.random.default_rng(5)
    film = (rng.integers(0, 3, (2, 8, 4)) * 0.5).astype(np.float32)  # 8 x 2: HDR's smallest coded width
    calls = [("IRIS", across, 1), ("TARGA", row, 4), ("TARGA_RAW", tall, 4), ("HDR", film, 3), ("WEBP", across, 4),
             ("IRIS", across, 1)]
    with rr.RenderContext(0) as fresh:
        got = [_device_file(fresh, rr, fmt, img, c) for fmt, img, c in calls]
    for k, (fmt, img, c) in enumerate(calls):
        assert got[k] == _host_file(rr, tmp_path, fmt, img, c), (k, fmt, "device file differs from the host coder's")
    assert got[0] == got[5]
