"""The device PNG switch at the C-ABI boundary (no GPU needed): librr.so exports
rr_set_device_png and rr_debug_png_device, the binding lists them, and a NULL
context is refused errno-style."""


def test_png_device_symbols_are_exported(rr):
    L = rr.lib()
    for name in ("rr_set_device_png", "rr_debug_png_device"):
        assert hasattr(L, name), f"librr.so does not export {name}"
        assert name in rr.EXPORTS


def test_set_device_png_null_context(rr):
    L = rr.lib()
    assert L.rr_set_device_png(None, 1) == -22
    assert b"NULL" in L.rr_last_error(None)


def test_debug_png_device_bad_arguments(rr):
    import ctypes
    n = ctypes.c_uint64()
    assert rr.lib().rr_debug_png_device(None, None, 4, 4, None, 0, ctypes.byref(n)) == -22
