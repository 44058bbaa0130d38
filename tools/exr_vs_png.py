#!/usr/bin/env python3
"""OPEN_EXR output measured against PNG (profiles/exr_device.md).

  per-frame: 1080p frames of the 04vs and 02 stand-ins written as OPEN_EXR with
             kernel profiling: file size against the reference writer's zlib
             level 1 file of the same pixels (tests/exr_reader.py), coder time
             (kernel_ms[RR_K_PNG]), readback_ms, encode_ms.
  rate:      frames per second of 02 with three frames in flight, written as
             OPEN_EXR / PNG (host) / PNG (device), alternating runs, spread.

Needs the GPU; prints one JSON line per result.
    python tools/exr_vs_png.py [--frames 24] [--runs 3] [--out DIR]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
rr = importlib.import_module("diploma_thesis-distributed_rendering_of_cgi_using_a_render_cluster_amd")
import exr_reader as X  # noqa: E402

SCENES = {"04vs": "04_very-simple-standin.rrscene", "02": "02_physics-standin.rrscene"}


def per_frame(ctx, which, out, reps=5):
    s = ctx.load_scene(os.path.join(ROOT, "scenes", SCENES[which]))
    try:
        p = rr.default_params(width=1920, height=1080, flags=rr.native.RR_FLAG_PROFILE_KERNELS)
        film = ctx.render_to_memory(s, 3, p)[0]
        want = X.expected_halfs(film)
        rows = []
        for k in range(reps + 1):  # the first frame warms up
            _, st = ctx.render_frame(s, 3, p, os.path.join(out, f"{which}_pf"), "OPEN_EXR")
            if k:
                rows.append((st.kernel_ms[rr.native.RR_K_PNG], st.readback_ms, st.encode_ms, st.total_ms))
        data = open(os.path.join(out, f"{which}_pf.exr"), "rb").read()
        px, _, sizes, modes = X.read_exr(data)
        assert np.array_equal(px, want), "the file does not decode to the film's halfs"
        ref = X.write_exr(want, 1)
        m = np.mean(rows, 0)
        return {"what": "per-frame", "scene": which, "spp": int(st.spp), "raw_bytes": 8 * 1920 * 1080,
                "device_bytes": len(data), "zlib1_bytes": len(ref), "device_over_zlib1": round(len(data) / len(ref), 4),
                "raw_chunks": modes.count("raw"), "chunks": len(modes),
                "coder_ms": round(m[0], 3), "readback_ms": round(m[1], 3), "encode_ms": round(m[2], 3),
                "total_ms": round(m[3], 3)}
    finally:
        s.close()


def rate(ctx, s, p, out, fmt, device_png, frames):
    ctx.set_device_png(device_png)
    try:
        def run(n, first):
            pending = []
            for f in range(first, first + n):
                pending.append(ctx.submit_frame(s, 1 + f % 100, p, os.path.join(out, f"r{f % 8}"), fmt))
                if len(pending) >= rr.native.RR_MAX_FRAMES_IN_FLIGHT:
                    ctx.complete_frame(pending.pop(0))
            for t in pending:
                ctx.complete_frame(t)
        run(4, 0)  # warm-up: buffers of this format
        t0 = time.perf_counter()
        run(frames, 4)
        return frames / (time.perf_counter() - t0)
    finally:
        ctx.set_device_png(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = a.out or tempfile.mkdtemp(prefix="exr_vs_png_")
    os.makedirs(out, exist_ok=True)
    ctx = rr.RenderContext(0)
    try:
        for which in ("04vs", "02"):
            print(json.dumps(per_frame(ctx, which, out)), flush=True)
        s = ctx.load_scene(os.path.join(ROOT, "scenes", SCENES["02"]))
        try:
            p = rr.default_params(width=1920, height=1080)
            modes = [("OPEN_EXR", "OPEN_EXR", False), ("PNG host", "PNG", False), ("PNG device", "PNG", True)]
            fps = {m[0]: [] for m in modes}
            for _ in range(a.runs):  # alternating
                for name, fmt, dev in modes:
                    fps[name].append(round(rate(ctx, s, p, out, fmt, dev, a.frames), 3))
            for name, v in fps.items():
                print(json.dumps({"what": "rate", "scene": "02", "format": name, "frames": a.frames, "fps": v,
                                  "mean": round(float(np.mean(v)), 3), "spread": round(max(v) - min(v), 3)}),
                      flush=True)
        finally:
            s.close()
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
