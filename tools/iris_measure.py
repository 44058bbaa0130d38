#!/usr/bin/env python3
"""IRIS output measured (profiles/iris_device.md).

1080p frames of the 04vs stand-in, of 01 (whose frame 3 is 04vs's) and of the
noisy 02 stand-in written as IRIS in the three colour modes, and beside them, in the same process, as TARGA in the same modes and as
HDR, with kernel profiling: coder time (kernel_ms[RR_K_PNG], all the coder's
kernels under one event pair), readback_ms, encode_ms and the file's size. Each
IRIS file is held against the restatement of tests/iris.py on the frame's 8-bit
image (byte for byte) and against the all-literal bound; the RGBA file also
goes through the strict reader, and its pixels are the TARGA file's.

Needs the GPU; prints one JSON line per result.
    python tools/iris_measure.py [--out DIR] [--reps 5] [--scenes 04vs,01,02]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "diploma_thesis-distributed_rendering_of_cgi_using_a_render_cluster_amd"
SCENES = {"04vs": "04_very-simple-standin.rrscene", "01": "01_simple-animation.rrscene",
          "02": "02_physics-standin.rrscene"}
EXT = {"IRIS": ".rgb", "TARGA": ".tga", "HDR": ".hdr"}
CASES = [("IRIS", m) for m in ("BW", "RGB", "RGBA")] + [("TARGA", m) for m in ("BW", "RGB", "RGBA")] + [("HDR", "RGB")]
CHANNELS = {"BW": 1, "RGB": 3, "RGBA": 4}


def per_frame(rr, I, T, root, ctx, which, out, reps):
    s = ctx.load_scene(os.path.join(root, "scenes", SCENES[which]))
    try:
        p = rr.default_params(width=1920, height=1080, flags=rr.native.RR_FLAG_PROFILE_KERNELS)
        rgba8 = ctx.render_to_memory(s, 3, p)[1]
        res, files = [], {}
        for fmt, mode in CASES:
            ctx.set_color_mode(mode)
            name = f"{which}_{fmt}_{mode}"
            rows = []
            for k in range(reps + 1):  # the first frame warms up
                _, st = ctx.render_frame(s, 3, p, os.path.join(out, name), fmt)
                if k:
                    rows.append((st.kernel_ms[rr.native.RR_K_PNG], st.readback_ms, st.encode_ms, st.total_ms))
            files[(fmt, mode)] = data = open(os.path.join(out, name + EXT[fmt]), "rb").read()
            m = np.mean(rows, 0)
            r = {"what": "per-frame", "scene": which, "format": fmt, "mode": mode, "spp": int(st.spp),
                 "file_bytes": len(data), "coder_ms": round(m[0], 3), "coder_ms_min": round(min(x[0] for x in rows), 3),
                 "coder_ms_max": round(max(x[0] for x in rows), 3), "readback_ms": round(m[1], 3),
                 "encode_ms": round(m[2], 3), "total_ms": round(m[3], 3)}
            if fmt == "IRIS":
                c = CHANNELS[mode]
                assert data == I.encode(rgba8, c), "the file is not the restatement's"
                bound = I.HEADER + I.body_bound(1920, 1080, c)
                assert len(data) <= bound, "a file above the all-literal bound"
                r["bound_bytes"] = bound
            res.append(r)
        px, info = I.read(files[("IRIS", "RGBA")])
        assert np.array_equal(px, T.read(files[("TARGA", "RGBA")])[0]), "IRIS and TARGA pixels differ"
        n_run = sum(k for row in info["packets"] for plane in row for run, k in plane if run)
        res[2]["run_bytes_share"] = round(n_run / (4 * 1920 * 1080), 4)
        return res
    finally:
        ctx.set_color_mode(0)
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scenes", default="04vs,01,02", help="comma-separated: 04vs, 01, 02")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    rr = importlib.import_module(PKG)
    import iris as I
    import tga as T
    out = a.out or tempfile.mkdtemp(prefix="iris_measure_")
    os.makedirs(out, exist_ok=True)
    ctx = rr.RenderContext(0)
    try:
        for which in a.scenes.split(","):
            for r in per_frame(rr, I, T, HERE, ctx, which, out, a.reps):
                print(json.dumps(r), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
