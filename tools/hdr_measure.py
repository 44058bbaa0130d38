#!/usr/bin/env python3
"""HDR output measured (profiles/hdr_device.md).

  per-frame: 1080p frames of the 04vs and 02 stand-ins written as HDR and as
             OPEN_EXR with HALF and with FLOAT channels, with kernel profiling:
             coder time (kernel_ms[RR_K_PNG]), readback_ms, encode_ms, the
             file's size; the HDR file against the restatement of tests/hdr.py
             on the FLOAT file's values (byte for byte) and against the
             all-literal bound.
  rate:      frames per second of 02 with three frames in flight, written as
             --format HDR or OPEN_EXR (HALF). One figure per process, so that a
             caller can alternate processes (and, with --root, checkouts: the
             OPEN_EXR figure of another commit comes from that commit's tree).

Needs the GPU; prints one JSON line per result.
    python tools/hdr_measure.py per-frame [--out DIR]
    python tools/hdr_measure.py rate --format HDR [--frames 24] [--root TREE] [--out DIR]
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
CASES = (("HDR", 0, ".hdr"), ("OPEN_EXR", 16, ".exr"), ("OPEN_EXR", 32, ".exr"))


def per_frame(rr, H, X, root, ctx, which, out, reps=5):
    s = ctx.load_scene(os.path.join(root, "scenes", SCENES[which]))
    try:
        p = rr.default_params(width=1920, height=1080, flags=rr.native.RR_FLAG_PROFILE_KERNELS)
        res, files = [], {}
        for fmt, depth, ext in CASES:
            ctx.set_exr_depth(depth)
            name = f"{which}_{fmt}_{depth}"
            rows = []
            for k in range(reps + 1):  # the first frame warms up
                _, st = ctx.render_frame(s, 3, p, os.path.join(out, name), fmt)
                if k:
                    rows.append((st.kernel_ms[rr.native.RR_K_PNG], st.readback_ms, st.encode_ms, st.total_ms))
            files[(fmt, depth)] = data = open(os.path.join(out, name + ext), "rb").read()
            m = np.mean(rows, 0)
            res.append({"what": "per-frame", "scene": which, "format": fmt, "depth": depth, "spp": int(st.spp),
                        "file_bytes": len(data), "coder_ms": round(m[0], 3),
                        "coder_ms_min": round(min(x[0] for x in rows), 3),
                        "coder_ms_max": round(max(x[0] for x in rows), 3), "readback_ms": round(m[1], 3),
                        "encode_ms": round(m[2], 3), "total_ms": round(m[3], 3)})
        means = np.ascontiguousarray(X.read_exr32(files[("OPEN_EXR", 32)])[0]).view(np.float32)
        hdr = files[("HDR", 0)]
        assert hdr == H.encode(means, 3), "the file is not the restatement's"
        bound = len(H.header(1920, 1080)) + 1080 * H.row_bound(1920)
        assert len(hdr) <= bound, "a file above the all-literal bound"
        q, info = H.read(hdr)
        n_run = sum(n for row in info["packets"] for plane in row for run, n in plane if run)
        res[0].update(bound_bytes=bound, run_bytes_share=round(n_run / (4 * 1920 * 1080), 4),
                      bw_file_bytes=len(H.encode(means, 1)))
        return res
    finally:
        ctx.set_exr_depth(0)
        s.close()


def rate(rr, ctx, s, p, out, frames, fmt):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["per-frame", "rate"])
    ap.add_argument("--format", default="HDR", choices=["HDR", "OPEN_EXR"])
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--root", default=HERE, help="the checkout whose package and scenes are measured")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    rr = importlib.import_module(PKG)
    out = a.out or tempfile.mkdtemp(prefix="hdr_measure_")
    os.makedirs(out, exist_ok=True)
    ctx = rr.RenderContext(0)
    try:
        if a.what == "per-frame":
            sys.path.insert(0, os.path.join(root, "tests"))
            import exr32_reader as X
            import hdr as H
            for which in ("04vs", "02"):
                for r in per_frame(rr, H, X, root, ctx, which, out):
                    print(json.dumps(r), flush=True)
            return
        s = ctx.load_scene(os.path.join(root, "scenes", SCENES["02"]))
        try:
            fps = rate(rr, ctx, s, rr.default_params(width=1920, height=1080), out, a.frames, a.format)
            print(json.dumps({"what": "rate", "scene": "02", "format": a.format, "label": a.label,
                              "frames": a.frames, "fps": round(fps, 3)}), flush=True)
        finally:
            s.close()
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
