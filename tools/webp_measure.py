#!/usr/bin/env python3
"""WEBP output measured (profiles/webp_device.md).

1080p frames of the 04vs stand-in (128 spp) and of the noisy 02 stand-in (64
spp) written as WEBP in the three colour modes and beside them, in the same
process, as IRIS and as device PNG, with kernel profiling: coder time
(kernel_ms[RR_K_PNG], all the coder's kernels under one event pair),
readback_ms, encode_ms and the file's size. Each WEBP file is held against the
host coder's file of the frame's 8-bit image (byte for byte), against PIL's
decode of it (the pixels) and against the all-literal bound. Beside the sizes:
PIL's own lossless files of the same pixels at methods 0 and 6.

With --min-runs the host coder's rule is restated by tests/webp.py at other
minimum copy lengths on a frame saved with --save (no GPU; slow: pure Python).

Needs the GPU unless --min-runs is given; prints one JSON line per result.
    python tools/webp_measure.py [--out DIR] [--reps 5] [--scenes 04vs,02] [--save DIR]
    python tools/webp_measure.py --min-runs 2,3,4,5 --frames DIR
"""
import argparse
import importlib
import io
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "diploma_thesis-distributed_rendering_of_cgi_using_a_render_cluster_amd"
SCENES = {"04vs": "04_very-simple-standin.rrscene", "01": "01_simple-animation.rrscene",
          "02": "02_physics-standin.rrscene"}
EXT = {"WEBP": ".webp", "IRIS": ".rgb", "PNG": ".png"}
CASES = [("WEBP", m) for m in ("BW", "RGB", "RGBA")] + [("IRIS", "RGBA"), ("PNG", "RGBA"), ("PNG", "RGB")]
CHANNELS = {"BW": 1, "RGB": 3, "RGBA": 4}


def per_frame(rr, W, root, ctx, which, out, reps, save):
    from PIL import Image
    s = ctx.load_scene(os.path.join(root, "scenes", SCENES[which]))
    ctx.set_device_png(True)
    try:
        p = rr.default_params(width=1920, height=1080, flags=rr.native.RR_FLAG_PROFILE_KERNELS)
        rgba8 = ctx.render_to_memory(s, 3, p)[1]
        if save:
            os.makedirs(save, exist_ok=True)
            np.save(os.path.join(save, f"{which}_rgba8.npy"), rgba8)
        res = []
        for fmt, mode in CASES:
            ctx.set_color_mode(mode)
            name = f"{which}_{fmt}_{mode}"
            rows = []
            for k in range(reps + 1):  # the first frame warms up
                _, st = ctx.render_frame(s, 3, p, os.path.join(out, name), fmt, 100)
                if k:
                    rows.append((st.kernel_ms[rr.native.RR_K_PNG], st.readback_ms, st.encode_ms, st.total_ms))
            data = open(os.path.join(out, name + EXT[fmt]), "rb").read()
            m = np.mean(rows, 0)
            r = {"what": "per-frame", "scene": which, "format": fmt, "mode": mode, "spp": int(st.spp),
                 "file_bytes": len(data), "coder_ms": round(m[0], 3), "coder_ms_min": round(min(x[0] for x in rows), 3),
                 "coder_ms_max": round(max(x[0] for x in rows), 3), "readback_ms": round(m[1], 3),
                 "encode_ms": round(m[2], 3), "total_ms": round(m[3], 3)}
            if fmt == "WEBP":
                c = CHANNELS[mode]
                rr.encode_image_mode(rgba8, os.path.join(out, name + "_host"), "WEBP", 100, mode)
                assert data == open(os.path.join(out, name + "_host.webp"), "rb").read(), "not the host coder's file"
                im = Image.open(io.BytesIO(data))
                assert np.array_equal(np.asarray(im), W.pil_expected(rgba8, c)), "PIL decodes other pixels"
                assert len(data) <= W.file_bound(1920, 1080), "a file above the all-literal bound"
                r["bound_bytes"] = W.file_bound(1920, 1080)
                for method in (0, 6):
                    buf = io.BytesIO()
                    Image.fromarray(W.pil_expected(rgba8, c)).save(buf, "WEBP", lossless=True, method=method, quality=100)
                    r[f"pil_method{method}_bytes"] = buf.tell()
            res.append(r)
        return res
    finally:
        ctx.set_color_mode(0)
        ctx.set_device_png(False)
        s.close()


def min_runs(W, frames, values):
    for name in sorted(os.listdir(frames)):
        if not name.endswith("_rgba8.npy"):
            continue
        rgba8 = np.load(os.path.join(frames, name))
        for v in values:
            W.MIN_RUN = v
            info = {}
            data = W.encode(rgba8, 4, info)
            copies = sum(1 for row in info["tokens"] for kind, _ in row if kind == "copy")
            print(json.dumps({"what": "min-run", "frame": name, "min_run": v, "file_bytes": len(data), "copies": copies,
                              "header_bits": info["header_bits"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--save", default=None, help="keep the frames' 8-bit images here (.npy)")
    ap.add_argument("--scenes", default="04vs,02", help="comma-separated: 04vs, 01, 02")
    ap.add_argument("--min-runs", default=None, help="comma-separated minimum copy lengths: restatement sizes, no GPU")
    ap.add_argument("--frames", default=None, help="where --save put the frames")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import webp as W
    if a.min_runs:
        return min_runs(W, a.frames, [int(v) for v in a.min_runs.split(",")])
    rr = importlib.import_module(PKG)
    out = a.out or tempfile.mkdtemp(prefix="webp_measure_")
    os.makedirs(out, exist_ok=True)
    ctx = rr.RenderContext(0)
    try:
        for which in a.scenes.split(","):
            for r in per_frame(rr, W, HERE, ctx, which, out, a.reps, a.save):
                print(json.dumps(r), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
