#!/usr/bin/env python3
"""16-bit PNG output measured (profiles/png16_device.md).

  per-frame: 1080p frames of the 04vs and 02 stand-ins written as 16-bit PNG
             with kernel profiling: file size against zlib.compress(level 1)
             over the same filtered bytes (tests/png16_reader.py), coder time
             (kernel_ms[RR_K_PNG]), readback_ms, encode_ms.
  rate:      frames per second of 02 with three frames in flight, written as
             device PNG at --depth 8 or 16. One figure per process, so that a
             caller can alternate processes (and, with --root, checkouts: the
             8-bit figure of another commit comes from that commit's tree).

Needs the GPU; prints one JSON line per result.
    python tools/png16_measure.py per-frame [--out DIR]
    python tools/png16_measure.py rate --depth 16 [--frames 24] [--root TREE] [--out DIR]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "diploma_thesis-distributed_rendering_of_cgi_using_a_render_cluster_amd"
SCENES = {"04vs": "04_very-simple-standin.rrscene", "02": "02_physics-standin.rrscene"}


def per_frame(rr, P, root, ctx, which, out, reps=5):
    s = ctx.load_scene(os.path.join(root, "scenes", SCENES[which]))
    try:
        p = rr.default_params(width=1920, height=1080, flags=rr.native.RR_FLAG_PROFILE_KERNELS)
        film = ctx.render_to_memory(s, 3, p)[0]
        state = ctx.frame_state(s, 3, p)
        want = P.front_end(film, int(state.render_ints[5]), float(state.render_floats[2]), rr.native.srgb16_table())
        rows = []
        ctx.set_png_depth(16)
        for k in range(reps + 1):  # the first frame warms up
            _, st = ctx.render_frame(s, 3, p, os.path.join(out, f"{which}_pf"), "PNG")
            if k:
                rows.append((st.kernel_ms[rr.native.RR_K_PNG], st.readback_ms, st.encode_ms, st.total_ms))
        data = open(os.path.join(out, f"{which}_pf.png"), "rb").read()
        px, info = P.read_png16(data)
        assert np.array_equal(px, want), "the file does not decode to the restated samples"
        ref = len(P.wrap(1920, 1080, zlib.compress(info["raw"], 1)))
        # the 8-bit device PNG of the same frame, for scale
        ctx.set_png_depth(8)
        ctx.set_device_png(True)
        _, st8 = ctx.render_frame(s, 3, p, os.path.join(out, f"{which}_pf8"), "PNG")
        ctx.set_device_png(False)
        ctx.set_png_depth(0)
        m = np.mean(rows, 0)
        return {"what": "per-frame", "scene": which, "spp": int(st.spp), "raw_bytes": len(info["raw"]),
                "device_bytes": len(data), "zlib1_bytes": ref, "device_over_zlib1": round(len(data) / ref, 4),
                "png8_device_bytes": int(st8.output_bytes), "png8_coder_ms": round(st8.kernel_ms[rr.native.RR_K_PNG], 3),
                "coder_ms": round(m[0], 3), "readback_ms": round(m[1], 3), "encode_ms": round(m[2], 3),
                "total_ms": round(m[3], 3)}
    finally:
        s.close()


def rate(rr, ctx, s, p, out, frames):
    def run(n, first):
        pending = []
        for f in range(first, first + n):
            pending.append(ctx.submit_frame(s, 1 + f % 100, p, os.path.join(out, f"r{f % 8}"), "PNG"))
            if len(pending) >= rr.native.RR_MAX_FRAMES_IN_FLIGHT:
                ctx.complete_frame(pending.pop(0))
        for t in pending:
            ctx.complete_frame(t)
    run(4, 0)  # warm-up: buffers of this format
    t0 = time.perf_counter()
    run(frames, 4)
    return frames / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["per-frame", "rate"])
    ap.add_argument("--depth", type=int, default=16, choices=[8, 16])
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--root", default=HERE, help="the checkout whose package and scenes are measured")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    rr = importlib.import_module(PKG)
    out = a.out or tempfile.mkdtemp(prefix="png16_measure_")
    os.makedirs(out, exist_ok=True)
    ctx = rr.RenderContext(0)
    try:
        if a.what == "per-frame":
            sys.path.insert(0, os.path.join(root, "tests"))
            import png16_reader as P
            for which in ("04vs", "02"):
                print(json.dumps(per_frame(rr, P, root, ctx, which, out)), flush=True)
            return
        s = ctx.load_scene(os.path.join(root, "scenes", SCENES["02"]))
        try:
            ctx.set_device_png(True)
            if a.depth == 16:
                ctx.set_png_depth(16)
            fps = rate(rr, ctx, s, rr.default_params(width=1920, height=1080), out, a.frames)
            print(json.dumps({"what": "rate", "scene": "02", "depth": a.depth, "label": a.label, "frames": a.frames,
                              "fps": round(fps, 3)}), flush=True)
        finally:
            s.close()
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
