"""ctypes binding of the renderer's C ABI (include/rr.h, lib/librr.so).

This is the Python host's view of the drop-in boundary; the Rust worker binds
the same symbols through an `extern "C"` block. The library is
the in-tree build from __graft_entry__.build(); there is no fallback: if it is
missing or fails to load, every entry point raises RRError.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "librr.so")
SHIM_PATH = os.path.join(_HERE, "lib", "rr-blender-shim")

RR_OK, RR_ENOENT, RR_EIO, RR_ENOMEM, RR_ENODEV, RR_EINVAL, RR_ENOTSUP = 0, -2, -5, -12, -19, -22, -95
RR_EBUSY = -16
RR_MAX_FRAMES_IN_FLIGHT = 3
RR_MAX_FRAME_OUTPUTS = 4
RR_VIEW_SCENE, RR_VIEW_STANDARD, RR_VIEW_RAW, RR_VIEW_FILMIC = -1, 0, 1, 2
RR_VIEW_FILMIC_LOG, RR_VIEW_FALSE_COLOR = 3, 4
# rr_set_look's names (include/rr.h), each also with Blender's "Filmic - " prefix
LOOKS = ["None", "Very High Contrast", "High Contrast", "Medium High Contrast", "Medium Contrast",
         "Medium Low Contrast", "Low Contrast", "Very Low Contrast"]
RR_ABI_VERSION = 8
QWIDTH = 6  # children per quantised node of the split path (rr_device.h kQWidth)
RR_CAM_FLOATS, RR_LIGHT_FLOATS, RR_MAT_FLOATS, RR_RENDER_INTS, RR_RENDER_FLOATS = 16, 12, 12, 10, 4


class RRError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"rr error {code}: {message}")
        self.code = code


class RenderParams(ctypes.Structure):
    _fields_ = [("spp", ctypes.c_int32), ("max_bounces", ctypes.c_int32),
                ("clamp_indirect", ctypes.c_float), ("seed", ctypes.c_uint32),
                ("use_scene_seed", ctypes.c_int32), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32), ("view_transform", ctypes.c_int32),
                ("spp_per_chunk", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("max_diffuse_bounces", ctypes.c_int32), ("max_glossy_bounces", ctypes.c_int32)]


class FrameOutput(ctypes.Structure):
    """rr_frame_output: one file of a frame (submit_frame_outputs)."""
    _fields_ = [("out_path", ctypes.c_char_p), ("format", ctypes.c_char_p),
                ("jpeg_quality", ctypes.c_int32), ("reduce", ctypes.c_int32)]


class FrameTiming(ctypes.Structure):
    _fields_ = [("loaded_at", ctypes.c_double), ("started_rendering_at", ctypes.c_double),
                ("finished_rendering_at", ctypes.c_double), ("file_saving_started_at", ctypes.c_double),
                ("file_saving_finished_at", ctypes.c_double)]


class FrameStats(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("spp", ctypes.c_int32),
                ("chunks", ctypes.c_int32), ("camera_rays", ctypes.c_uint64),
                ("extension_rays", ctypes.c_uint64), ("shadow_rays", ctypes.c_uint64),
                ("primary_continued", ctypes.c_uint64), ("primary_shadow", ctypes.c_uint64),
                ("anim_ms", ctypes.c_double), ("build_ms", ctypes.c_double), ("trace_ms", ctypes.c_double),
                ("readback_ms", ctypes.c_double), ("encode_ms", ctypes.c_double), ("total_ms", ctypes.c_double),
                ("bvh_rebuilt", ctypes.c_int32), ("n_triangles", ctypes.c_int32),
                ("output_bytes", ctypes.c_uint64),
                ("kernel_ms", ctypes.c_double * 8), ("kernel_launches", ctypes.c_int32 * 8),
                ("trav_nodes", ctypes.c_uint64 * 3), ("trav_tris", ctypes.c_uint64 * 3),
                ("camera_rays_traced", ctypes.c_uint64), ("view_transform", ctypes.c_int32),
                ("view_transform_substituted", ctypes.c_int32), ("kernel_clock_ghz", ctypes.c_double),
                ("kernel_wave_fill", ctypes.c_double), ("tile_slices", ctypes.c_int32),
                ("stack_drops", ctypes.c_int32),
                ("extension_rays_escaped", ctypes.c_uint64), ("shadow_rays_escaped", ctypes.c_uint64),
                ("kernel_entry_spread", ctypes.c_double), ("kernel_exit_spread", ctypes.c_double)]

    def as_dict(self) -> dict:
        out = {}
        for k, _ in self._fields_:
            v = getattr(self, k)
            out[k] = list(v) if not isinstance(v, (int, float)) else v
        return out


RR_FLAG_PROFILE_KERNELS, RR_FLAG_COUNT_TRAVERSAL, RR_FLAG_WAVEFRONT = 1, 2, 4
KERNEL_CLASSES = ["build", "primary", "extend", "shadow", "accumulate", "shade", "tiles"]
RR_K_PNG = 7  # FrameStats.kernel_ms index of the device deflate coder (PNG with rr_set_device_png, 16-bit PNG, or OPEN_EXR), the TARGA packer, the HDR, the IRIS or the WEBP coder


# Every symbol include/rr.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "rr_render_params_default", "rr_abi_version", "rr_create", "rr_scene_load", "rr_render_frame",
    "rr_frame_submit", "rr_frame_complete",
    "rr_render_frame_to_memory", "rr_scene_resolution", "rr_encode_image", "rr_last_error",
    "rr_last_warning", "rr_set_ocio_config", "rr_synchronize",
    "rr_scene_free", "rr_destroy", "rr_debug_counts", "rr_debug_scene_mesh", "rr_debug_frame_state", "rr_debug_bvh",
    "rr_debug_trace", "rr_debug_object_matrix", "rr_debug_qbvh", "rr_debug_bvh_hier", "rr_debug_jpeg_device",
    "rr_debug_bsdf_sample", "rr_debug_fastmath_check", "rr_debug_tile_costs",
    "rr_set_device_png", "rr_debug_png_device", "rr_debug_exr_device",
    "rr_set_png_depth", "rr_debug_png16_device", "rr_debug_srgb16_table",
    "rr_set_exr_depth", "rr_debug_exr32_device",
    "rr_set_color_mode", "rr_encode_image_mode", "rr_debug_encode_device",
    "rr_set_look", "rr_set_display_gamma", "rr_debug_view_device", "rr_debug_display_gamma", "rr_debug_scene_view",
    "rr_set_dither", "rr_debug_dither_noise", "rr_debug_sin_fixed",
    "rr_set_png_compression", "rr_encode_image_png", "rr_debug_png_filters", "rr_debug_scene_png_compression",
    "rr_debug_hdr_host",
    "rr_set_exr_codec", "rr_debug_scene_exr_codec", "rr_debug_float24", "rr_debug_exr_rle",
    "rr_frame_submit_outputs", "rr_render_frame_outputs", "rr_last_output_bytes", "rr_set_extra_outputs",
    "rr_debug_film_reduce",
    "rr_set_region", "rr_set_region_off", "rr_set_region_from_scene", "rr_region_resolution", "rr_debug_film_window",
]

# rr_set_exr_codec's values (include/rr.h), by Blender's names of the codecs
EXR_CODECS = {"": 0, "NONE": 1, "RLE": 2, "ZIPS": 3, "ZIP": 4, "PIZ": 5, "PXR24": 6, "B44": 7, "B44A": 8,
              "DWAA": 9, "DWAB": 10}
RR_EXR_CODEC_SCENE, RR_EXR_CODEC_NONE, RR_EXR_CODEC_RLE, RR_EXR_CODEC_ZIPS, RR_EXR_CODEC_ZIP = 0, 1, 2, 3, 4
RR_EXR_CODEC_PIZ, RR_EXR_CODEC_PXR24, RR_EXR_CODEC_B44, RR_EXR_CODEC_B44A = 5, 6, 7, 8
RR_EXR_CODEC_DWAA, RR_EXR_CODEC_DWAB = 9, 10


def exr_codec_value(codec) -> int:
    """One of Blender's codec names, "" / None (the scene's), or an RR_EXR_CODEC_* value, as an int."""
    if codec is None:
        return RR_EXR_CODEC_SCENE
    if isinstance(codec, str):
        if codec not in EXR_CODECS:
            raise ValueError(f"EXR codec must be one of {', '.join(k for k in EXR_CODECS if k)}, got {codec!r}")
        return EXR_CODECS[codec]
    return int(codec)


# rr_set_png_compression's values beside 0 .. 100 (include/rr.h)
RR_PNG_COMPRESSION_LEGACY, RR_PNG_COMPRESSION_SCENE = -1, -2


def png_compression_value(v) -> int:
    """0 .. 100, "legacy" / None, "scene", or one of the RR_PNG_COMPRESSION_* values, as an int."""
    if v is None or v == "legacy":
        return RR_PNG_COMPRESSION_LEGACY
    if v == "scene":
        return RR_PNG_COMPRESSION_SCENE
    if isinstance(v, str):
        raise ValueError(f"PNG compression must be 0 .. 100, 'legacy' or 'scene', got {v!r}")
    return int(v)


# rr_set_dither's value for "the scene's render.dither_intensity" (include/rr.h)
RR_DITHER_SCENE = -1.0

# rr_set_color_mode's values (include/rr.h): the channels the file holds.
RR_COLOR_SCENE, RR_COLOR_BW, RR_COLOR_RGB, RR_COLOR_RGBA = 0, 1, 3, 4
COLOR_MODES = {"": RR_COLOR_SCENE, "BW": RR_COLOR_BW, "RGB": RR_COLOR_RGB, "RGBA": RR_COLOR_RGBA}


def color_mode_value(mode) -> int:
    """"BW" / "RGB" / "RGBA" / "" / None, or one of the RR_COLOR_* values, as an int."""
    if mode is None:
        return RR_COLOR_SCENE
    if isinstance(mode, str):
        if mode not in COLOR_MODES:
            raise ValueError(f"colour mode must be BW, RGB or RGBA, got {mode!r}")
        return COLOR_MODES[mode]
    return int(mode)

_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    # RR_LIB_PATH: an alternative in-tree build of the same library (A/B timing
    # of kernel variants, tools/ab_variants.sh); never a different implementation.
    path = os.environ.get("RR_LIB_PATH", LIB_PATH)
    if not os.path.isfile(path):
        raise RRError(RR_ENOENT, f"{path} is missing: build it with __graft_entry__.build() "
                                 "(there is no CPU fallback)")
    L = ctypes.CDLL(path)
    if L.rr_abi_version() != RR_ABI_VERSION:
        raise RRError(RR_EINVAL, f"{path}: ABI {L.rr_abi_version()}, this binding expects {RR_ABI_VERSION} "
                                 "(rebuild with __graft_entry__.build())")
    P, c_int, i32, u32, f32p, u8p = ctypes.c_void_p, ctypes.c_int, ctypes.c_int32, ctypes.c_uint32, \
        ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8)
    i32p, u32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint32)
    sig = {
        "rr_render_params_default": (None, [ctypes.POINTER(RenderParams)]),
        "rr_abi_version": (i32, []),
        "rr_create": (c_int, [c_int, ctypes.POINTER(P)]),
        "rr_scene_load": (c_int, [P, ctypes.c_char_p, ctypes.POINTER(P)]),
        "rr_render_frame": (c_int, [P, P, i32, ctypes.POINTER(RenderParams), ctypes.c_char_p, ctypes.c_char_p, i32,
                                    ctypes.POINTER(FrameTiming), ctypes.POINTER(FrameStats)]),
        "rr_frame_submit": (c_int, [P, P, i32, ctypes.POINTER(RenderParams), ctypes.c_char_p, ctypes.c_char_p, i32,
                                    ctypes.POINTER(ctypes.c_uint64)]),
        "rr_frame_complete": (c_int, [P, ctypes.c_uint64, ctypes.POINTER(FrameTiming), ctypes.POINTER(FrameStats)]),
        "rr_render_frame_to_memory": (c_int, [P, P, i32, ctypes.POINTER(RenderParams), f32p, u8p,
                                              ctypes.POINTER(FrameStats)]),
        "rr_scene_resolution": (c_int, [P, ctypes.POINTER(RenderParams), i32p, i32p]),
        "rr_encode_image": (c_int, [u8p, i32, i32, ctypes.c_char_p, ctypes.c_char_p, i32,
                                    ctypes.POINTER(ctypes.c_uint64)]),
        "rr_last_error": (ctypes.c_char_p, [P]),
        "rr_last_warning": (ctypes.c_char_p, [P]),
        "rr_set_ocio_config": (c_int, [P, ctypes.c_char_p]),
        "rr_synchronize": (c_int, [P]),
        "rr_scene_free": (None, [P]),
        "rr_destroy": (None, [P]),
        "rr_debug_counts": (c_int, [P, i32p, i32p, i32p, i32p]),
        "rr_debug_scene_mesh": (c_int, [P, f32p, i32p]),
        "rr_debug_frame_state": (c_int, [P, P, i32, ctypes.POINTER(RenderParams), f32p, i32p, f32p, f32p, f32p,
                                         f32p, i32p, f32p]),
        "rr_debug_bvh": (c_int, [P, P, i32, u32p, u32p, i32p, f32p]),
        "rr_debug_trace": (c_int, [P, P, i32, i32, i32, f32p, f32p, i32p, u8p]),
        "rr_debug_qbvh": (c_int, [P, P, i32, i32p, i32p, u32p, i32p]),
        "rr_debug_bvh_hier": (c_int, [P, P, i32, i32, u32p, u32p, i32p, f32p]),
        "rr_debug_jpeg_device": (c_int, [P, u8p, i32, i32, i32, u8p, ctypes.c_uint64,
                                         ctypes.POINTER(ctypes.c_uint64)]),
        "rr_set_device_png": (c_int, [P, i32]),
        "rr_debug_png_device": (c_int, [P, u8p, i32, i32, u8p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
        "rr_debug_exr_device": (c_int, [P, f32p, i32, i32, u8p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
        "rr_set_png_depth": (c_int, [P, i32]),
        "rr_debug_png16_device": (c_int, [P, f32p, i32, i32, i32, ctypes.c_float, u8p, ctypes.c_uint64,
                                          ctypes.POINTER(ctypes.c_uint64)]),
        "rr_debug_srgb16_table": (c_int, [f32p, i32, i32p]),
        "rr_set_exr_depth": (c_int, [P, i32]),
        "rr_debug_exr32_device": (c_int, [P, f32p, i32, i32, u8p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
        "rr_set_color_mode": (c_int, [P, i32]),
        "rr_encode_image_mode": (c_int, [u8p, i32, i32, ctypes.c_char_p, ctypes.c_char_p, i32, i32,
                                         ctypes.POINTER(ctypes.c_uint64)]),
        "rr_debug_encode_device": (c_int, [P, ctypes.c_char_p, i32, i32, ctypes.c_void_p, i32, i32, i32, i32,
                                           ctypes.c_float, i32, u8p, ctypes.c_uint64,
                                           ctypes.POINTER(ctypes.c_uint64)]),
        "rr_set_look": (c_int, [P, ctypes.c_char_p]),
        "rr_set_display_gamma": (c_int, [P, ctypes.c_float]),
        "rr_debug_view_device": (c_int, [P, f32p, i32, i32, i32, ctypes.c_float, u8p]),
        "rr_debug_display_gamma": (c_int, [f32p, ctypes.c_uint64, ctypes.c_float, f32p]),
        "rr_debug_scene_view": (c_int, [P, i32p, ctypes.c_char_p, i32, f32p]),
        "rr_set_dither": (c_int, [P, ctypes.c_float]),
        "rr_debug_dither_noise": (c_int, [i32, i32, f32p]),
        "rr_debug_sin_fixed": (c_int, [f32p, ctypes.c_uint64, f32p]),
        "rr_set_png_compression": (c_int, [P, i32]),
        "rr_encode_image_png": (c_int, [u8p, i32, i32, ctypes.c_char_p, i32, i32, ctypes.POINTER(ctypes.c_uint64)]),
        "rr_debug_png_filters": (c_int, [u8p, i32, i32, i32, u8p]),
        "rr_debug_scene_png_compression": (c_int, [P, i32p]),
        "rr_set_exr_codec": (c_int, [P, i32]),
        "rr_debug_scene_exr_codec": (c_int, [P, i32p]),
        "rr_debug_float24": (c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]),
        "rr_debug_exr_rle": (c_int, [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                     ctypes.POINTER(ctypes.c_uint64)]),
        "rr_frame_submit_outputs": (c_int, [P, P, i32, ctypes.POINTER(RenderParams), ctypes.POINTER(FrameOutput), i32,
                                            ctypes.POINTER(ctypes.c_uint64)]),
        "rr_render_frame_outputs": (c_int, [P, P, i32, ctypes.POINTER(RenderParams), ctypes.POINTER(FrameOutput), i32,
                                            ctypes.POINTER(FrameTiming), ctypes.POINTER(FrameStats)]),
        "rr_last_output_bytes": (c_int, [P, i32, ctypes.POINTER(ctypes.c_uint64)]),
        "rr_set_extra_outputs": (c_int, [P, ctypes.c_char_p]),
        "rr_debug_film_reduce": (c_int, [P, f32p, i32, i32, i32, f32p]),
        "rr_set_region": (c_int, [P, i32, i32, i32, i32, i32]),
        "rr_set_region_off": (c_int, [P]),
        "rr_set_region_from_scene": (c_int, [P, i32]),
        "rr_region_resolution": (c_int, [P, P, P, ctypes.POINTER(i32), ctypes.POINTER(i32)]),
        "rr_debug_film_window": (c_int, [P, f32p, i32, i32, i32, i32, i32, i32, i32, ctypes.c_float, f32p]),
        "rr_debug_hdr_host": (c_int, [f32p, i32, i32, i32, u8p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
        "rr_debug_object_matrix": (c_int, [P, i32, ctypes.c_double, ctypes.POINTER(ctypes.c_double)]),
        "rr_debug_bsdf_sample": (c_int, [P, f32p, f32p, f32p, i32, f32p, f32p, f32p, f32p, i32p]),
        "rr_debug_fastmath_check": (c_int, [P, ctypes.c_uint32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
        "rr_debug_tile_costs": (c_int, [P, c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int32),
                                        ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint64), c_int]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _check(rc: int, ctx=None):
    if rc != 0:
        msg = lib().rr_last_error(ctx).decode("utf-8", "replace")
        raise RRError(rc, msg)


def _ptr(a: np.ndarray | None, ctype):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.POINTER(ctype))


def default_params(**overrides) -> RenderParams:
    p = RenderParams()
    lib().rr_render_params_default(ctypes.byref(p))
    for k, v in overrides.items():
        if v is None:
            continue
        if k == "seed":
            p.use_scene_seed = 0
        setattr(p, k, v)
    return p


@dataclass
class FrameState:
    tris: np.ndarray        # (n, 3, 3) world-space vertices
    tri_mat: np.ndarray     # (n,)
    camera: np.ndarray      # (16,)
    lights: np.ndarray      # (nl, 12)
    materials: np.ndarray   # (nm, 12)
    world: np.ndarray       # (3,)
    render_ints: np.ndarray  # (RR_RENDER_INTS,)
    render_floats: np.ndarray  # (4,)


class Scene:
    """An exported project (.rrscene) — host-only until a RenderContext uses it."""

    def __init__(self, path: str, ctx: "RenderContext | None" = None):
        self.path = os.fspath(path)
        h = ctypes.c_void_p()
        _check(lib().rr_scene_load(ctx.handle if ctx else None, self.path.encode(), ctypes.byref(h)))
        self.handle = h
        self.ctx = ctx

    def close(self):
        if self.handle:
            lib().rr_scene_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def counts(self) -> dict:
        v = [ctypes.c_int32() for _ in range(4)]
        _check(lib().rr_debug_counts(self.handle, *[ctypes.byref(x) for x in v]))
        return dict(zip(["triangles", "lights", "materials", "objects"], [x.value for x in v]))

    def mesh(self) -> tuple[np.ndarray, np.ndarray]:
        """Object-space triangles (n, 3, 3) float32 and the object index of each
        (rr_debug_scene_mesh)."""
        n = self.counts()["triangles"]
        local = np.zeros((max(n, 1), 3, 3), np.float32)
        obj = np.zeros(max(n, 1), np.int32)
        _check(lib().rr_debug_scene_mesh(self.handle, _ptr(local, ctypes.c_float), _ptr(obj, ctypes.c_int32)))
        return local[:n], obj[:n]

    def resolution(self, params: RenderParams | None = None) -> tuple[int, int]:
        w, h = ctypes.c_int32(), ctypes.c_int32()
        _check(lib().rr_scene_resolution(self.handle, ctypes.byref(params) if params else None,
                                         ctypes.byref(w), ctypes.byref(h)))
        return w.value, h.value

    def frame_constants(self, frame: int, params: RenderParams | None = None) -> FrameState:
        """Host-only frame evaluation (no device): camera, lights, materials, world, render ints/floats."""
        c = self.counts()
        nl, nm = c["lights"], c["materials"]
        cam = np.zeros(RR_CAM_FLOATS, np.float32)
        lights = np.zeros((max(nl, 1), RR_LIGHT_FLOATS), np.float32)
        mats = np.zeros((max(nm, 1), RR_MAT_FLOATS), np.float32)
        world = np.zeros(3, np.float32)
        ri = np.zeros(RR_RENDER_INTS, np.int32)
        rf = np.zeros(RR_RENDER_FLOATS, np.float32)
        tm = np.zeros(max(c["triangles"], 1), np.int32)
        _check(lib().rr_debug_frame_state(None, self.handle, int(frame), ctypes.byref(params) if params else None,
                                          None, _ptr(tm, ctypes.c_int32), _ptr(cam, ctypes.c_float),
                                          _ptr(lights, ctypes.c_float),
                                          _ptr(mats, ctypes.c_float), _ptr(world, ctypes.c_float),
                                          _ptr(ri, ctypes.c_int32), _ptr(rf, ctypes.c_float)))
        # tris stay empty (world triangles need the device); tri_mat is the scene's, per triangle
        return FrameState(np.zeros((0, 3, 3), np.float32), tm[:c["triangles"]], cam, lights[:nl], mats[:nm],
                          world, ri, rf)

    def view_settings(self) -> tuple[int, str, float]:
        """rr_debug_scene_view: the view transform (RR_VIEW_*), look name (no
        prefix) and display gamma the scene file asks for (host only)."""
        v, g = ctypes.c_int32(), ctypes.c_float()
        look = ctypes.create_string_buffer(64)
        _check(lib().rr_debug_scene_view(self.handle, ctypes.byref(v), look, 64, ctypes.byref(g)))
        return v.value, look.value.decode(), g.value

    def png_compression(self) -> int:
        """rr_debug_scene_png_compression: the scene file's render.png_compression,
        0 .. 100, or RR_PNG_COMPRESSION_LEGACY where it has none (host only)."""
        v = ctypes.c_int32()
        _check(lib().rr_debug_scene_png_compression(self.handle, ctypes.byref(v)))
        return v.value

    def exr_codec(self) -> int:
        """rr_debug_scene_exr_codec: the scene file's render.exr_codec as an
        RR_EXR_CODEC_* value, RR_EXR_CODEC_ZIP where it has none (host only)."""
        v = ctypes.c_int32()
        _check(lib().rr_debug_scene_exr_codec(self.handle, ctypes.byref(v)))
        return v.value

    def object_matrix(self, obj: int, frame: float) -> np.ndarray:
        m = (ctypes.c_double * 16)()
        _check(lib().rr_debug_object_matrix(self.handle, obj, float(frame), m))
        return np.array(m[:], dtype=np.float64).reshape(4, 4)


class RenderContext:
    """One HIP device (rr_ctx). Not thread-safe; one frame in flight at a time."""

    def __init__(self, device: int = 0, png_depth: int = 0, exr_depth: int = 0, color_mode=0,
                 look: str | None = None, display_gamma: float = 0.0, dither=None, png_compression=None,
                 exr_codec=None):
        """exr_codec: the compression of "OPEN_EXR" frames (set_exr_codec): one of Blender's names
        or an RR_EXR_CODEC_* value; None: the context's own (the scene's, or what RR_EXR_CODEC says).
        dither: the dither of the 8-bit images (set_dither): an intensity in [0, 2] or
        "scene"; None: the context's own (0, or what RR_DITHER says).
        png_compression: the compression of "PNG" files (set_png_compression): 0 .. 100,
        "scene" or "legacy"; None: the context's own (legacy, or what RR_PNG_COMPRESSION says).
        png_depth: bits per sample of "PNG" frames (set_png_depth; 0: the scene's).
        exr_depth: channel type of "OPEN_EXR" frames (set_exr_depth; 0: the scene's).
        color_mode: "BW" / "RGB" / "RGBA" of every file (set_color_mode; 0: the scene's).
        look: the look of Filmic frames (set_look; None: the scene's).
        display_gamma: the display gamma of every frame (set_display_gamma; 0: the scene's)."""
        h = ctypes.c_void_p()
        _check(lib().rr_create(int(device), ctypes.byref(h)))
        self.handle = h
        if png_depth:
            self.set_png_depth(png_depth)
        if exr_depth:
            self.set_exr_depth(exr_depth)
        if color_mode_value(color_mode):
            self.set_color_mode(color_mode)
        if look:
            self.set_look(look)
        if display_gamma:
            self.set_display_gamma(display_gamma)
        if dither is not None:
            self.set_dither(dither)
        if png_compression is not None:
            self.set_png_compression(png_compression)
        if exr_codec is not None:
            self.set_exr_codec(exr_codec)
        self.device = device

    def close(self):
        if self.handle:
            lib().rr_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def load_scene(self, path: str) -> Scene:
        return Scene(path, self)

    def set_ocio_config(self, directory: str | None):
        """rr_set_ocio_config: Blender colour-management directory whose Filmic
        LUTs implement RR_VIEW_FILMIC (None: none; Filmic falls back to Standard)."""
        _check(lib().rr_set_ocio_config(self.handle, directory.encode() if directory else None), self.handle)

    def synchronize(self):
        """rr_synchronize: wait for all device work this context enqueued."""
        _check(lib().rr_synchronize(self.handle), self.handle)

    def last_warning(self) -> str:
        return lib().rr_last_warning(self.handle).decode("utf-8", "replace")

    def render_frame(self, scene: Scene, frame: int, params: RenderParams | None = None,
                     out_path: str | None = None, fmt: str | None = "JPEG", quality: int = 90):
        t, s = FrameTiming(), FrameStats()
        _check(lib().rr_render_frame(self.handle, scene.handle, int(frame),
                                     ctypes.byref(params) if params else None,
                                     out_path.encode() if out_path is not None else None,
                                     fmt.encode() if (fmt is not None and out_path is not None) else None,
                                     int(quality), ctypes.byref(t), ctypes.byref(s)), self.handle)
        return t, s

    def submit_frame(self, scene: Scene, frame: int, params: RenderParams | None = None,
                     out_path: str | None = None, fmt: str | None = "JPEG", quality: int = 90) -> int:
        """rr_frame_submit: enqueue the frame's device work, return its ticket."""
        t = ctypes.c_uint64()
        _check(lib().rr_frame_submit(self.handle, scene.handle, int(frame),
                                     ctypes.byref(params) if params else None,
                                     out_path.encode() if out_path is not None else None,
                                     fmt.encode() if (fmt is not None and out_path is not None) else None,
                                     int(quality), ctypes.byref(t)), self.handle)
        return int(t.value)

    @staticmethod
    def _outputs(outputs):
        """(path, fmt[, quality[, reduce]]) tuples as an rr_frame_output array (quality 90, reduce 1)."""
        arr = (FrameOutput * max(len(outputs), 1))()
        for a, o in zip(arr, outputs):
            path, fmt, quality, reduce = tuple(o) + (90, 1)[len(o) - 2:]
            a.out_path = os.fspath(path).encode() if path is not None else None
            a.format = fmt.encode() if fmt is not None else None
            a.jpeg_quality, a.reduce = int(quality), int(reduce)
        return arr

    def submit_frame_outputs(self, scene: Scene, frame: int, params: RenderParams | None, outputs) -> int:
        """rr_frame_submit_outputs: one frame, several files. outputs: (path, fmt, quality, reduce)
        tuples, path without extension, reduce 1, 2, 4 or 8 (a proxy reduced by that factor)."""
        t = ctypes.c_uint64()
        _check(lib().rr_frame_submit_outputs(self.handle, scene.handle, int(frame),
                                             ctypes.byref(params) if params else None,
                                             self._outputs(outputs), len(outputs), ctypes.byref(t)), self.handle)
        return int(t.value)

    def render_frame_outputs(self, scene: Scene, frame: int, params: RenderParams | None, outputs):
        """rr_render_frame_outputs: submit_frame_outputs + complete_frame; (timing, stats)."""
        t, s = FrameTiming(), FrameStats()
        _check(lib().rr_render_frame_outputs(self.handle, scene.handle, int(frame),
                                             ctypes.byref(params) if params else None,
                                             self._outputs(outputs), len(outputs), ctypes.byref(t),
                                             ctypes.byref(s)), self.handle)
        return t, s

    def last_output_bytes(self, index: int = 0) -> int:
        """rr_last_output_bytes: the size of file `index` of the frame completed last."""
        n = ctypes.c_uint64()
        _check(lib().rr_last_output_bytes(self.handle, int(index), ctypes.byref(n)), self.handle)
        return int(n.value)

    def set_extra_outputs(self, spec: str | None = None):
        """rr_set_extra_outputs: files every frame with a path also writes, "FORMAT[:K],..."
        ("JPEG:4,PNG": <path>.r4.jpg and <path>.png); None / "": none."""
        _check(lib().rr_set_extra_outputs(self.handle, spec.encode() if spec else None), self.handle)

    def set_region(self, region=None, crop: bool = False, from_scene: bool | None = None):
        """rr_set_region: frames render the rectangle (x0, y0, x1, y1) of full-frame pixels, rows top first, half
        open; crop: the outputs are the region's pixels alone, else the full frame with (0, 0, 0, 0) outside.
        None: rr_set_region_off. from_scene (when given): rr_set_region_from_scene, a scene's render.border
        comes before this region."""
        if region is None:
            _check(lib().rr_set_region_off(self.handle), self.handle)
        else:
            x0, y0, x1, y1 = (int(v) for v in region)
            _check(lib().rr_set_region(self.handle, x0, y0, x1, y1, 1 if crop else 0), self.handle)
        if from_scene is not None:
            _check(lib().rr_set_region_from_scene(self.handle, 1 if from_scene else 0), self.handle)

    def set_region_from_scene(self, on: bool = True):
        """rr_set_region_from_scene: a scene's render.border gives the region of its frames."""
        _check(lib().rr_set_region_from_scene(self.handle, 1 if on else 0), self.handle)

    def region_resolution(self, scene: Scene, params: RenderParams | None = None):
        """rr_region_resolution: (width, height) of the files and of render_to_memory's images."""
        w, h = ctypes.c_int32(), ctypes.c_int32()
        _check(lib().rr_region_resolution(self.handle, scene.handle, ctypes.byref(params) if params else None,
                                          ctypes.byref(w), ctypes.byref(h)), self.handle)
        return int(w.value), int(h.value)

    def film_window(self, rgba: np.ndarray, region, crop: bool, alpha_sum: float = 1.0) -> np.ndarray:
        """rr_debug_film_window: k_film_window over an (H, W, 4) float32 image."""
        rgba = np.ascontiguousarray(rgba, dtype=np.float32)
        h, w = rgba.shape[:2]
        x0, y0, x1, y1 = (int(v) for v in region)
        out = np.zeros((y1 - y0, x1 - x0, 4) if crop else (h, w, 4), np.float32)
        _check(lib().rr_debug_film_window(self.handle, _ptr(rgba, ctypes.c_float), w, h, x0, y0, x1, y1,
                                          1 if crop else 0, float(alpha_sum), _ptr(out, ctypes.c_float)), self.handle)
        return out

    def film_reduce(self, rgba: np.ndarray, reduce: int) -> np.ndarray:
        """rr_debug_film_reduce on the device: the box mean of an (H, W, 4) float32 image."""
        return film_reduce(rgba, reduce, self)

    def complete_frame(self, ticket: int):
        """rr_frame_complete: wait, encode + write; (timing, stats)."""
        t, s = FrameTiming(), FrameStats()
        _check(lib().rr_frame_complete(self.handle, ctypes.c_uint64(ticket), ctypes.byref(t), ctypes.byref(s)),
               self.handle)
        return t, s

    def render_to_memory(self, scene: Scene, frame: int, params: RenderParams | None = None,
                         film: bool = True, rgba: bool = True):
        w, h = self.region_resolution(scene, params)  # the frame's, or with a cropped region that region's
        f = np.zeros((h, w, 4), np.float32) if film else None
        r = np.zeros((h, w, 4), np.uint8) if rgba else None
        s = FrameStats()
        _check(lib().rr_render_frame_to_memory(self.handle, scene.handle, int(frame),
                                               ctypes.byref(params) if params else None,
                                               _ptr(f, ctypes.c_float), _ptr(r, ctypes.c_uint8),
                                               ctypes.byref(s)), self.handle)
        return f, r, s

    def frame_state(self, scene: Scene, frame: int, params: RenderParams | None = None) -> FrameState:
        c = scene.counts()
        n, nl, nm = c["triangles"], c["lights"], c["materials"]
        tris = np.zeros((max(n, 1), 3, 3), np.float32)
        mats_i = np.zeros(max(n, 1), np.int32)
        cam = np.zeros(RR_CAM_FLOATS, np.float32)
        lights = np.zeros((max(nl, 1), RR_LIGHT_FLOATS), np.float32)
        mats = np.zeros((max(nm, 1), RR_MAT_FLOATS), np.float32)
        world = np.zeros(3, np.float32)
        ri = np.zeros(RR_RENDER_INTS, np.int32)
        rf = np.zeros(RR_RENDER_FLOATS, np.float32)
        _check(lib().rr_debug_frame_state(self.handle, scene.handle, int(frame),
                                          ctypes.byref(params) if params else None,
                                          _ptr(tris, ctypes.c_float) if self.handle else None,
                                          _ptr(mats_i, ctypes.c_int32),
                                          _ptr(cam, ctypes.c_float), _ptr(lights, ctypes.c_float),
                                          _ptr(mats, ctypes.c_float), _ptr(world, ctypes.c_float),
                                          _ptr(ri, ctypes.c_int32), _ptr(rf, ctypes.c_float)), self.handle)
        return FrameState(tris[:n], mats_i[:n], cam, lights[:nl], mats[:nm], world, ri, rf)

    def bvh(self, scene: Scene, frame: int, hier: int = 0):
        """rr_debug_bvh_hier: (keys, order, children (ni,2), boxes (ni,12)); hier
        2 = LBVH, 3 = PLOC, 0 = the frame's hierarchy."""
        n = scene.counts()["triangles"]
        ni = max(n - 1, 1)
        keys = np.zeros(n, np.uint32)
        order = np.zeros(n, np.uint32)
        children = np.zeros((ni, 2), np.int32)
        boxes = np.zeros((ni, 12), np.float32)
        _check(lib().rr_debug_bvh_hier(self.handle, scene.handle, int(frame), int(hier), _ptr(keys, ctypes.c_uint32),
                                  _ptr(order, ctypes.c_uint32), _ptr(children, ctypes.c_int32),
                                  _ptr(boxes, ctypes.c_float)), self.handle)
        return keys, order, children, boxes

    def qbvh(self, scene: Scene, frame: int, with_order: bool = False):
        """rr_debug_qbvh: (children (nq, QWIDTH) with the implicit references
        spelled out, nodes (nq, 16) uint32: the raw 64-byte quantised nodes,
        rr_device.h QNode6); with_order: also the original triangle id at each
        position of the hierarchy's triangle array."""
        nq = ctypes.c_int32()
        _check(lib().rr_debug_qbvh(self.handle, scene.handle, int(frame), ctypes.byref(nq), None, None, None),
               self.handle)
        ch = np.zeros((max(nq.value, 1), QWIDTH), np.int32)
        bx = np.zeros((max(nq.value, 1), 16), np.uint32)
        orig = np.zeros(max(scene.counts()["triangles"], 1), np.int32)
        _check(lib().rr_debug_qbvh(self.handle, scene.handle, int(frame), ctypes.byref(nq), _ptr(ch, ctypes.c_int32),
                                   _ptr(bx, ctypes.c_uint32), _ptr(orig, ctypes.c_int32)), self.handle)
        if with_order:
            return ch[:nq.value], bx[:nq.value], orig[:scene.counts()["triangles"]]
        return ch[:nq.value], bx[:nq.value]

    def jpeg_device(self, rgba: np.ndarray, quality: int = 90) -> bytes:
        """rr_debug_jpeg_device: the JPEG file bytes of an (H, W, 4) uint8 image
        encoded on the device (forward DCT + Huffman coding)."""
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        h, w = rgba.shape[:2]
        n = ctypes.c_uint64()
        _check(lib().rr_debug_jpeg_device(self.handle, _ptr(rgba, ctypes.c_uint8), w, h, int(quality), None, 0,
                                          ctypes.byref(n)), self.handle)
        out = np.zeros(n.value, np.uint8)
        _check(lib().rr_debug_jpeg_device(self.handle, _ptr(rgba, ctypes.c_uint8), w, h, int(quality),
                                          _ptr(out, ctypes.c_uint8), n.value, ctypes.byref(n)), self.handle)
        return out.tobytes()

    def set_device_png(self, on: bool = True):
        """rr_set_device_png: code "PNG" frames of this context on the device
        (png.hip) instead of reading the image back for the host's zlib threads."""
        _check(lib().rr_set_device_png(self.handle, 1 if on else 0), self.handle)

    def png_device(self, rgba: np.ndarray) -> bytes:
        """rr_debug_png_device: the PNG file bytes of an (H, W, 4) uint8 image
        encoded on the device (Sub filter, LZ77, dynamic Huffman)."""
        rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
        h, w = rgba.shape[:2]
        raw = (4 * w + 1) * h
        out = np.zeros(raw + raw // 8 + 4096, np.uint8)  # above the all-stored worst case
        n = ctypes.c_uint64()
        _check(lib().rr_debug_png_device(self.handle, _ptr(rgba, ctypes.c_uint8), w, h,
                                         _ptr(out, ctypes.c_uint8), out.size, ctypes.byref(n)), self.handle)
        if n.value > out.size:
            raise RRError(RR_EINVAL, f"device PNG of {n.value} bytes exceeds the {out.size}-byte buffer")
        return out[:n.value].tobytes()

    def set_png_depth(self, depth: int = 0):
        """rr_set_png_depth: bits per sample of "PNG" frames of this context, 0
        (the scene's render.color_depth), 8 or 16. 16-bit frames are always coded
        on the device (png16.hip)."""
        _check(lib().rr_set_png_depth(self.handle, int(depth)), self.handle)

    def png16_device(self, rgba: np.ndarray, view_transform: int = 0, exposure_scale: float = 1.0) -> bytes:
        """rr_debug_png16_device: the 16-bit RGBA PNG file bytes of an (H, W, 4)
        float32 image of means, taken through exposure, clamp, view transform and
        quantize16 and encoded on the device (png16.hip). Alpha is forced to 1."""
        rgba = np.ascontiguousarray(rgba, dtype=np.float32)
        h, w = rgba.shape[:2]
        raw = (8 * w + 1) * h
        out = np.zeros(raw + 5 * (raw // 65535 + (h + 15) // 16 + 1) + 1024, np.uint8)  # above the all-stored worst case
        n = ctypes.c_uint64()
        _check(lib().rr_debug_png16_device(self.handle, _ptr(rgba, ctypes.c_float), w, h, int(view_transform),
                                           ctypes.c_float(exposure_scale), _ptr(out, ctypes.c_uint8), out.size,
                                           ctypes.byref(n)), self.handle)
        if n.value > out.size:
            raise RRError(RR_EINVAL, f"device PNG of {n.value} bytes exceeds the {out.size}-byte buffer")
        return out[:n.value].tobytes()

    def exr_device(self, rgba: np.ndarray) -> bytes:
        """rr_debug_exr_device: the OpenEXR file bytes (half A, B, G, R; ZIP) of an
        (H, W, 4) float32 image of means, encoded on the device (exr.hip)."""
        rgba = np.ascontiguousarray(rgba, dtype=np.float32)
        h, w = rgba.shape[:2]
        out = np.zeros(8 * w * h + 16 * ((h + 15) // 16) + 1024, np.uint8)  # above the all-raw worst case
        n = ctypes.c_uint64()
        _check(lib().rr_debug_exr_device(self.handle, _ptr(rgba, ctypes.c_float), w, h,
                                         _ptr(out, ctypes.c_uint8), out.size, ctypes.byref(n)), self.handle)
        if n.value > out.size:
            raise RRError(RR_EINVAL, f"device EXR of {n.value} bytes exceeds the {out.size}-byte buffer")
        return out[:n.value].tobytes()

    def set_exr_codec(self, codec=RR_EXR_CODEC_SCENE):
        """rr_set_exr_codec: Blender's image_settings.exr_codec for this context's
        "OPEN_EXR" frames: "NONE", "RLE", "ZIP" or "PXR24" (coded on the device), ""
        / None for each scene's render.exr_codec (ZIP without one), or one of the
        codecs that are not built ("ZIPS", "PIZ", "B44", "B44A", "DWAA", "DWAB"):
        such a frame is written as ZIP and last_warning says so."""
        _check(lib().rr_set_exr_codec(self.handle, exr_codec_value(codec)), self.handle)

    def set_exr_depth(self, depth: int = 0):
        """rr_set_exr_depth: channel type of "OPEN_EXR" frames of this context, 0
        (the scene's render.exr_depth), 16 (HALF) or 32 (FLOAT: the film's means
        bit for bit)."""
        _check(lib().rr_set_exr_depth(self.handle, int(depth)), self.handle)

    def set_color_mode(self, mode=0):
        """rr_set_color_mode: Blender's image_settings.color_mode for the files of
        this context: "BW" (grey, Rec.709 luma), "RGB", "RGBA" or the RR_COLOR_*
        values; 0 / "": the scene's render.color_mode, else each format's own layout."""
        _check(lib().rr_set_color_mode(self.handle, color_mode_value(mode)), self.handle)

    def set_look(self, name: str | None = None):
        """rr_set_look: the look of this context's Filmic frames, one of LOOKS
        (also with Blender's "Filmic - " prefix); None / "": the scene's render.look."""
        _check(lib().rr_set_look(self.handle, name.encode() if name else None), self.handle)

    def set_display_gamma(self, gamma: float = 0.0):
        """rr_set_display_gamma: the display gamma of this context's frames, in
        (0, 5]; 0: the scene's render.gamma. 1 skips the step."""
        _check(lib().rr_set_display_gamma(self.handle, ctypes.c_float(gamma)), self.handle)

    def set_dither(self, intensity=0.0):
        """rr_set_dither: the dither of this context's 8-bit images, an intensity
        in [0, 2] (0: none), or "scene" (RR_DITHER_SCENE) for each scene's
        render.dither_intensity."""
        v = RR_DITHER_SCENE if intensity == "scene" else float(intensity)
        _check(lib().rr_set_dither(self.handle, ctypes.c_float(v)), self.handle)

    def set_png_compression(self, percent="legacy"):
        """rr_set_png_compression: Blender's image_settings.compression for this
        context's "PNG" files: 0 .. 100 (libpng's adaptive row filters; the host
        coder at Blender's zlib level), "scene" for each scene's
        render.png_compression, or "legacy" (the default: Sub on every row, host
        level 1)."""
        _check(lib().rr_set_png_compression(self.handle, png_compression_value(percent)), self.handle)

    def view_device(self, rgba: np.ndarray, view_transform: int = 0, exposure_scale: float = 1.0) -> np.ndarray:
        """rr_debug_view_device: the (H, W, 4) uint8 image the 8-bit view pass
        makes of an (H, W, 4) float32 image of means, with this context's look
        and display gamma."""
        rgba = np.ascontiguousarray(rgba, dtype=np.float32)
        h, w = rgba.shape[:2]
        out = np.zeros((h, w, 4), np.uint8)
        _check(lib().rr_debug_view_device(self.handle, _ptr(rgba, ctypes.c_float), w, h, int(view_transform),
                                          ctypes.c_float(exposure_scale), _ptr(out, ctypes.c_uint8)), self.handle)
        return out

    def encode_device(self, fmt: str, image: np.ndarray, depth: int = 0, color_mode=0, view_transform: int = 0,
                      exposure_scale: float = 1.0, quality: int = 90) -> bytes:
        """rr_debug_encode_device: the file bytes of an (H, W, 4) image coded on the
        device as `fmt` ("JPEG", "PNG", "OPEN_EXR", "TARGA", "TARGA_RAW", "HDR",
        "IRIS", "WEBP") at `depth` in `color_mode`. uint8 images for JPEG, 8-bit PNG,
        TARGA, IRIS and WEBP, float32 means for the others; "HDR" at depth 0 or 32 and
        no other. `quality`: JPEG's; a "WEBP" file is lossless at every quality, and
        one below 100 is flagged (last_warning)."""
        if fmt == "HDR" and (image.dtype == np.uint8 or int(depth) not in (0, 32)):
            raise RRError(RR_EINVAL, "HDR takes a float image at depth 0 or 32")
        is_float = image.dtype != np.uint8
        image = np.ascontiguousarray(image, dtype=np.float32 if is_float else np.uint8)
        h, w = image.shape[:2]
        args = (self.handle, fmt.encode(), int(depth), color_mode_value(color_mode),
                image.ctypes.data_as(ctypes.c_void_p), 1 if is_float else 0, w, h, int(view_transform),
                ctypes.c_float(exposure_scale), int(quality))
        n = ctypes.c_uint64()
        _check(lib().rr_debug_encode_device(*args, None, 0, ctypes.byref(n)), self.handle)
        out = np.zeros(n.value, np.uint8)
        _check(lib().rr_debug_encode_device(*args, _ptr(out, ctypes.c_uint8), out.size, ctypes.byref(n)), self.handle)
        if n.value > out.size:
            raise RRError(RR_EINVAL, f"device file of {n.value} bytes exceeds the {out.size}-byte buffer")
        return out[:n.value].tobytes()

    def exr32_device(self, rgba: np.ndarray) -> bytes:
        """rr_debug_exr32_device: the OpenEXR file bytes (FLOAT A, B, G, R; ZIP) of
        an (H, W, 4) float32 image of means, encoded on the device (exr.hip)."""
        rgba = np.ascontiguousarray(rgba, dtype=np.float32)
        h, w = rgba.shape[:2]
        out = np.zeros(16 * w * h + 16 * ((h + 15) // 16) + 1024, np.uint8)  # above the all-raw worst case
        n = ctypes.c_uint64()
        _check(lib().rr_debug_exr32_device(self.handle, _ptr(rgba, ctypes.c_float), w, h,
                                           _ptr(out, ctypes.c_uint8), out.size, ctypes.byref(n)), self.handle)
        if n.value > out.size:
            raise RRError(RR_EINVAL, f"device EXR of {n.value} bytes exceeds the {out.size}-byte buffer")
        return out[:n.value].tobytes()

    def bsdf_sample(self, mat12, n, wo, u):
        """rr_debug_bsdf_sample: (wi [k,3], f [k,3], pdf [k], ok [k]: 0 end, 1 diffuse, 2 glossy)."""
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
        m, n, wo, u = f32(mat12), f32(n), f32(wo), f32(u).reshape(-1, 3)
        k = u.shape[0]
        wi, f = np.zeros((k, 3), np.float32), np.zeros((k, 3), np.float32)
        pdf, ok = np.zeros(k, np.float32), np.zeros(k, np.int32)
        _check(lib().rr_debug_bsdf_sample(self.handle, _ptr(m, ctypes.c_float), _ptr(n, ctypes.c_float),
                                          _ptr(wo, ctypes.c_float), k, _ptr(u, ctypes.c_float),
                                          _ptr(wi, ctypes.c_float), _ptr(f, ctypes.c_float),
                                          _ptr(pdf, ctypes.c_float), _ptr(ok, ctypes.c_int32)), self.handle)
        return wi, f, pdf, ok

    def fastmath_check(self, lo: int = 0, n: int = 1 << 32):
        """rr_debug_fastmath_check: mismatches of (sqrt_rn in range, sqrt_rn outside, sqrt_any,
        rcp_rn in range, rcp_rn outside)."""
        out = (ctypes.c_uint64 * 5)()
        _check(lib().rr_debug_fastmath_check(self.handle, int(lo), int(n), out), self.handle)
        return tuple(int(v) for v in out)

    def tile_costs(self, capacity: int = 1 << 20, units: int = 1 << 16, raw: bool = False):
        """rr_debug_tile_costs: (per-tile real-time ticks of the last tile frame's
        units, the box tiles' hand-out order it used, each of the slot buffers'
        length; per box unit u its (start, end) ticks when that frame was a
        counting frame, shape (units, 2)). raw: the cost array untrimmed (all
        `capacity` words): behind the frame's own tile count T it holds, at
        [T, 2T), the samples a counting launch's covered body ran per tile."""
        costs = np.zeros(capacity, np.uint32)
        order = np.zeros(capacity, np.int32)
        log = np.zeros((max(units, 1), 2), np.uint64)
        n = ctypes.c_int32(0)
        _check(lib().rr_debug_tile_costs(self.handle, capacity, _ptr(costs, ctypes.c_uint32),
                                         _ptr(order, ctypes.c_int32), ctypes.byref(n),
                                         _ptr(log, ctypes.c_uint64), units), self.handle)
        m = min(int(n.value), capacity)
        return (costs if raw else costs[:m]), order[:m], log[:units]

    def trace(self, scene: Scene, frame: int, rays: np.ndarray, width: int = 0):
        """rr_debug_trace; width 0 = the hierarchy the frame kernels use."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = rays.shape[0]
        hits = np.zeros((max(n, 1), 4), np.float32)
        prims = np.zeros(max(n, 1), np.int32)
        occ = np.zeros(max(n, 1), np.uint8)
        _check(lib().rr_debug_trace(self.handle, scene.handle, int(frame), int(width), n, _ptr(rays, ctypes.c_float),
                                    _ptr(hits, ctypes.c_float), _ptr(prims, ctypes.c_int32),
                                    _ptr(occ, ctypes.c_uint8)), self.handle)
        return hits[:n], prims[:n], occ[:n]


def srgb16_table() -> np.ndarray:
    """rr_debug_srgb16_table: the float32 sRGB table of the 16-bit PNG path
    (intervals + 1 entries; host only, no device needed)."""
    n = ctypes.c_int32()
    _check(lib().rr_debug_srgb16_table(None, 0, ctypes.byref(n)))
    t = np.zeros(n.value, np.float32)
    _check(lib().rr_debug_srgb16_table(_ptr(t, ctypes.c_float), t.size, ctypes.byref(n)))
    return t


def display_gamma(values: np.ndarray, gamma: float) -> np.ndarray:
    """rr_debug_display_gamma: values ** (1 / gamma) by the renderer's fixed
    log2 / exp2 polynomials, evaluated on the host (no device needed)."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.zeros_like(v)
    _check(lib().rr_debug_display_gamma(_ptr(v.reshape(-1), ctypes.c_float), v.size, ctypes.c_float(gamma),
                                        _ptr(out.reshape(-1), ctypes.c_float)))
    return out


def sin_fixed(values: np.ndarray) -> np.ndarray:
    """rr_debug_sin_fixed: the dither's fixed sine of float32 values, evaluated
    on the host (no device needed)."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.zeros_like(v)
    _check(lib().rr_debug_sin_fixed(_ptr(v.reshape(-1), ctypes.c_float), v.size, _ptr(out.reshape(-1), ctypes.c_float)))
    return out


def dither_noise(width: int, height: int) -> np.ndarray:
    """rr_debug_dither_noise: the dither's noise n of every pixel, (height,
    width) float32, rows top to bottom, evaluated on the host."""
    out = np.zeros((int(height), int(width)), np.float32)
    _check(lib().rr_debug_dither_noise(int(width), int(height), _ptr(out.reshape(-1), ctypes.c_float)))
    return out


def encode_image(rgba: np.ndarray, out_path_no_ext: str, fmt: str, quality: int = 90) -> int:
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w = rgba.shape[:2]
    nbytes = ctypes.c_uint64()
    _check(lib().rr_encode_image(_ptr(rgba, ctypes.c_uint8), w, h, out_path_no_ext.encode(), fmt.encode(),
                                 int(quality), ctypes.byref(nbytes)))
    return nbytes.value


def last_host_warning() -> str:
    """rr_last_warning without a context: the warning of this thread's last
    encode_image / encode_image_mode ("WEBP" below quality 100), "" if none."""
    return lib().rr_last_warning(None).decode("utf-8", "replace")


def encode_image_mode(rgba: np.ndarray, out_path_no_ext: str, fmt: str, quality: int = 90, color_mode=0) -> int:
    """rr_encode_image_mode: the host encoders in a colour mode ("BW", "RGB", "RGBA", 0)."""
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w = rgba.shape[:2]
    nbytes = ctypes.c_uint64()
    _check(lib().rr_encode_image_mode(_ptr(rgba, ctypes.c_uint8), w, h, out_path_no_ext.encode(), fmt.encode(),
                                      int(quality), color_mode_value(color_mode), ctypes.byref(nbytes)))
    return nbytes.value


def encode_image_png(rgba: np.ndarray, out_path_no_ext: str, color_mode=0, compression="legacy") -> int:
    """rr_encode_image_png: the host PNG coder in a colour mode with a compression
    setting (0 .. 100, or "legacy" for encode_image_mode's bytes)."""
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w = rgba.shape[:2]
    nbytes = ctypes.c_uint64()
    _check(lib().rr_encode_image_png(_ptr(rgba, ctypes.c_uint8), w, h, out_path_no_ext.encode(),
                                     color_mode_value(color_mode), png_compression_value(compression),
                                     ctypes.byref(nbytes)))
    return nbytes.value


def hdr_host(rgba: np.ndarray, color_mode=0) -> bytes:
    """rr_debug_hdr_host: the Radiance RGBE file ("HDR") the host coder makes of an
    (H, W, 4) float32 image of means in `color_mode` ("BW", or "RGB" / "RGBA" / 0
    for RGB). No context and no device: the reference for the device coder's bytes."""
    rgba = np.ascontiguousarray(rgba, dtype=np.float32)
    h, w = rgba.shape[:2]
    args = (_ptr(rgba, ctypes.c_float), w, h, color_mode_value(color_mode))
    n = ctypes.c_uint64()
    _check(lib().rr_debug_hdr_host(*args, None, 0, ctypes.byref(n)))
    out = np.zeros(n.value, np.uint8)
    _check(lib().rr_debug_hdr_host(*args, _ptr(out, ctypes.c_uint8), out.size, ctypes.byref(n)))
    return out[:n.value].tobytes()


def png_filters(raw: np.ndarray, bpp: int) -> np.ndarray:
    """rr_debug_png_filters: the filter type rr_set_png_compression's rule gives
    every row of (rows, row_bytes) uint8 raw scanlines with `bpp` bytes a pixel,
    evaluated on the host."""
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    rows, row_bytes = raw.shape
    out = np.zeros(rows, np.uint8)
    _check(lib().rr_debug_png_filters(_ptr(raw.reshape(-1), ctypes.c_uint8), row_bytes, rows, int(bpp),
                                      _ptr(out, ctypes.c_uint8)))
    return out


def film_reduce(rgba: np.ndarray, reduce: int, ctx: "RenderContext | None" = None) -> np.ndarray:
    """rr_debug_film_reduce: the (ceil(H / reduce), ceil(W / reduce), 4) box mean of an (H, W, 4)
    float32 image by csrc/reduce_rule.h, on ctx's device, or on the host without a context."""
    rgba = np.ascontiguousarray(rgba, dtype=np.float32)
    h, w = rgba.shape[:2]
    k = max(int(reduce), 1)
    out = np.zeros((-(-h // k), -(-w // k), 4), np.float32)
    _check(lib().rr_debug_film_reduce(ctx.handle if ctx else None, _ptr(rgba, ctypes.c_float), w, h, int(reduce),
                                      _ptr(out, ctypes.c_float)), ctx.handle if ctx else None)
    return out


def float24(values) -> np.ndarray:
    """rr_debug_float24: the 24-bit form PXR24 files hold of float32 values
    (host only), as uint32."""
    a = np.ascontiguousarray(values, dtype=np.float32).ravel()
    out = np.zeros(a.size, np.uint32)
    _check(lib().rr_debug_float24(a.ctypes.data, a.size, out.ctypes.data))
    return out


def exr_rle(data) -> bytes:
    """rr_debug_exr_rle: the packets an RLE chunk holds for bytes that are
    already reordered and differenced (host only)."""
    a = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
    cap = a.size + a.size // 127 + 2
    out = np.zeros(cap, np.uint8)
    n = ctypes.c_uint64()
    _check(lib().rr_debug_exr_rle(a.ctypes.data, a.size, out.ctypes.data, cap, ctypes.byref(n)))
    return out[: n.value].tobytes()
