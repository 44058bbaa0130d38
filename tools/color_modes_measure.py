#!/usr/bin/env python3
"""Colour modes measured (profiles/color_modes.md).

  sizes:     the 1080p frames of the 04vs (128 spp) and 02 (64 spp) stand-ins
             written in every mode x deflate-coded format: file size against
             the same file with its front-end bytes deflated by zlib level 1
             (tests/color_modes.py). With RR_LIB_PATH naming a build of other
             free distances for C = 1 (-DRR_PNG8_Y_DIST=... etc.), that
             build's sizes. JPEG: the file sizes alone.
  per-frame: coder time (kernel_ms[RR_K_PNG]; JPEG has no class of its own and
             reports readback_ms, image done to outputs on the host, which the
             JPEG kernels fill), encode_ms and file bytes of the
             same frames in every mode, mean of 5 serial frames after a
             warm-up.

Needs the GPU; prints one JSON line per result.
    python tools/color_modes_measure.py sizes [--label 2,1,2,1]
    python tools/color_modes_measure.py per-frame
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
SCENES = {"04vs": "04_very-simple-standin.rrscene", "02": "02_physics-standin.rrscene"}
# name, format, device PNG, PNG depth, EXR depth
FORMATS = [("png8", "PNG", True, 8, 0), ("png16", "PNG", False, 16, 0), ("exr16", "OPEN_EXR", False, 0, 16),
           ("exr32", "OPEN_EXR", False, 0, 32), ("jpeg", "JPEG", False, 0, 0)]
EXT = {"PNG": ".png", "OPEN_EXR": ".exr", "JPEG": ".jpg"}


def select(ctx, fmt, mode):
    _, _, dev_png, png_depth, exr_depth = fmt
    ctx.set_device_png(dev_png)
    ctx.set_png_depth(png_depth)
    ctx.set_exr_depth(exr_depth)
    ctx.set_color_mode(mode)


def sizes(rr, ctx, M, which, out, label, modes):
    s = ctx.load_scene(os.path.join(HERE, "scenes", SCENES[which]))
    try:
        p = rr.default_params(width=1920, height=1080)
        for fmt in FORMATS:
            for mode in modes:
                if fmt[0] == "jpeg" and mode == "RGBA":
                    continue
                select(ctx, fmt, mode)
                _, st = ctx.render_frame(s, 3, p, os.path.join(out, "sz"), fmt[1], 90)
                data = open(os.path.join(out, "sz" + EXT[fmt[1]]), "rb").read()
                row = {"what": "sizes", "scene": which, "label": label, "format": fmt[0], "mode": mode,
                       "spp": int(st.spp), "device_bytes": len(data)}
                if fmt[1] == "PNG":
                    ref = M.png_zlib1_file_bytes(data, M.read_png(data)[1])
                elif fmt[1] == "OPEN_EXR":
                    info = M.read_exr(data)[1]
                    ref = info["zlib1_file_bytes"]
                    row["raw_chunks"] = info["modes"].count("raw")
                else:
                    ref = None
                if ref:
                    row.update(zlib1_bytes=ref, device_over_zlib1=round(len(data) / ref, 4))
                print(json.dumps(row), flush=True)
    finally:
        s.close()


def per_frame(rr, ctx, which, out, reps=5):
    s = ctx.load_scene(os.path.join(HERE, "scenes", SCENES[which]))
    try:
        p = rr.default_params(width=1920, height=1080, flags=rr.native.RR_FLAG_PROFILE_KERNELS)
        for fmt in FORMATS:
            for mode in ("RGBA", "RGB", "BW"):
                if fmt[0] == "jpeg" and mode == "RGBA":
                    continue
                select(ctx, fmt, mode)
                rows = []
                for k in range(reps + 1):  # the first frame warms up
                    _, st = ctx.render_frame(s, 3, p, os.path.join(out, "pf"), fmt[1], 90)
                    coder = st.readback_ms if fmt[0] == "jpeg" else st.kernel_ms[rr.native.RR_K_PNG]
                    if k:
                        rows.append((coder, st.encode_ms))
                m = np.mean(rows, 0)
                print(json.dumps({"what": "per-frame", "scene": which, "format": fmt[0], "mode": mode,
                                  "spp": int(st.spp), "file_bytes": int(st.output_bytes),
                                  "coder_ms": round(float(m[0]), 3), "encode_ms": round(float(m[1]), 3)}), flush=True)
    finally:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["sizes", "per-frame"])
    ap.add_argument("--label", default="")
    ap.add_argument("--modes", default="RGBA,RGB,BW")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import color_modes as M
    rr = importlib.import_module(PKG)
    out = a.out or tempfile.mkdtemp(prefix="color_modes_measure_")
    os.makedirs(out, exist_ok=True)
    ctx = rr.RenderContext(0)
    try:
        for which in ("04vs", "02"):
            if a.what == "sizes":
                sizes(rr, ctx, M, which, out, a.label, a.modes.split(","))
            else:
                per_frame(rr, ctx, which, out)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
