#!/usr/bin/env python3
"""OPEN_EXR with FLOAT channels measured (profiles/exr32_device.md).

  sizes:     the 1080p frames of the 04vs and 02 stand-ins written as FLOAT
             OPEN_EXR: file size against the reference writer's zlib level 1
             file of the same floats (tests/exr32_reader.py), raw chunks. With
             RR_LIB_PATH naming a build of another distance triple
             (-DRR_EXR32_DROP=n), that triple's sizes.
  per-frame: coder time (kernel_ms[RR_K_PNG]), readback_ms, encode_ms of the
             same frames at --depth 16 (HALF) or 32 (FLOAT), mean of 5 serial
             frames after a warm-up.
  rate:      frames per second of --scene with three frames in flight at
             --depth. One figure per process, so that a caller can alternate
             processes (and, with --root, checkouts: the HALF figure of
             another commit comes from that commit's package; the scenes are
             this tree's).

Needs the GPU; prints one JSON line per result.
    python tools/exr32_measure.py sizes [--label 2,2W,8W]
    python tools/exr32_measure.py per-frame --depth 32
    python tools/exr32_measure.py rate --scene 02 --depth 32 [--frames 24] [--root TREE]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "diploma_thesis-distributed_rendering_of_cgi_using_a_render_cluster_amd"
SCENES = {"04vs": "04_very-simple-standin.rrscene", "02": "02_physics-standin.rrscene"}


def sizes(rr, ctx, which, out, label):
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import exr32_reader as F
    s = ctx.load_scene(os.path.join(HERE, "scenes", SCENES[which]))
    try:
        p = rr.default_params(width=1920, height=1080)
        want = F.bits(ctx.render_to_memory(s, 3, p)[0])
        ctx.set_exr_depth(32)
        _, st = ctx.render_frame(s, 3, p, os.path.join(out, f"{which}_sz"), "OPEN_EXR")
        data = open(os.path.join(out, f"{which}_sz.exr"), "rb").read()
        px, _, _, modes = F.read_exr32(data)
        assert np.array_equal(px, want), "the file does not decode to the film's floats"
        ref = F.write_exr32(want, 1)
        return {"what": "sizes", "scene": which, "label": label, "spp": int(st.spp), "raw_bytes": 16 * 1920 * 1080,
                "device_bytes": len(data), "zlib1_bytes": len(ref), "device_over_zlib1": round(len(data) / len(ref), 4),
                "device_over_raw": round(len(data) / (16 * 1920 * 1080), 4),
                "raw_chunks": modes.count("raw"), "chunks": len(modes)}
    finally:
        s.close()


def per_frame(rr, ctx, which, out, depth, reps=5):
    s = ctx.load_scene(os.path.join(HERE, "scenes", SCENES[which]))
    try:
        p = rr.default_params(width=1920, height=1080, flags=rr.native.RR_FLAG_PROFILE_KERNELS)
        rows = []
        for k in range(reps + 1):  # the first frame warms up
            _, st = ctx.render_frame(s, 3, p, os.path.join(out, f"{which}_pf"), "OPEN_EXR")
            if k:
                rows.append((st.kernel_ms[rr.native.RR_K_PNG], st.readback_ms, st.encode_ms, st.total_ms))
        m = np.mean(rows, 0)
        return {"what": "per-frame", "scene": which, "depth": depth, "spp": int(st.spp),
                "file_bytes": int(st.output_bytes), "coder_ms": round(m[0], 3), "readback_ms": round(m[1], 3),
                "encode_ms": round(m[2], 3), "total_ms": round(m[3], 3)}
    finally:
        s.close()


def rate(rr, ctx, s, p, out, frames):
    def run(n, first):
        pending = []
        for f in range(first, first + n):
            pending.append(ctx.submit_frame(s, 1 + f % 100, p, os.path.join(out, f"r{f % 8}"), "OPEN_EXR"))
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
    ap.add_argument("what", choices=["sizes", "per-frame", "rate"])
    ap.add_argument("--depth", type=int, default=32, choices=[16, 32])
    ap.add_argument("--scene", default="02", choices=sorted(SCENES))
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--root", default=HERE, help="the checkout whose package is measured")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    rr = importlib.import_module(PKG)
    out = a.out or tempfile.mkdtemp(prefix="exr32_measure_")
    os.makedirs(out, exist_ok=True)
    ctx = rr.RenderContext(0)
    try:
        if a.what == "sizes":
            for which in ("04vs", "02"):
                print(json.dumps(sizes(rr, ctx, which, out, a.label)), flush=True)
            return
        if a.depth == 32:  # a checkout without the call writes HALF, which is what --depth 16 asks of it
            ctx.set_exr_depth(32)
        if a.what == "per-frame":
            for which in ("04vs", "02"):
                print(json.dumps(per_frame(rr, ctx, which, out, a.depth)), flush=True)
            return
        s = ctx.load_scene(os.path.join(HERE, "scenes", SCENES[a.scene]))
        try:
            fps = rate(rr, ctx, s, rr.default_params(width=1920, height=1080), out, a.frames)
            print(json.dumps({"what": "rate", "scene": a.scene, "depth": a.depth, "label": a.label,
                              "frames": a.frames, "fps": round(fps, 3)}), flush=True)
        finally:
            s.close()
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
