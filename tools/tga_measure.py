#!/usr/bin/env python3
"""TARGA output measured (profiles/tga_device.md).

  per-frame: 1080p frames of the 04vs and 02 stand-ins written as TARGA and as
             TARGA_RAW with kernel profiling: coder time (kernel_ms[RR_K_PNG]),
             readback_ms, encode_ms; the file against the restatement of
             tests/tga.py (byte for byte), its size against PIL's own tga_rle
             writer on the same pixels and against the all-literal bound.
  rate:      frames per second of 02 with three frames in flight, written as
             --format TARGA, TARGA_RAW or PNG (device PNG). One figure per
             process, so that a caller can alternate processes (and, with
             --root, checkouts: the PNG figure of another commit comes from
             that commit's tree).

Needs the GPU; prints one JSON line per result.
    python tools/tga_measure.py per-frame [--out DIR]
    python tools/tga_measure.py rate --format TARGA [--frames 24] [--root TREE] [--out DIR]
"""
import argparse
import importlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "diploma_thesis-distributed_rendering_of_cgi_using_a_render_cluster_amd"
SCENES = {"04vs": "04_very-simple-standin.rrscene", "02": "02_physics-standin.rrscene"}


def pil_rle_bytes(px):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(px if px.shape[2] > 1 else px[..., 0]).save(buf, format="TGA", compression="tga_rle")
    return len(buf.getvalue())


def per_frame(rr, T, root, ctx, which, out, reps=5):
    s = ctx.load_scene(os.path.join(root, "scenes", SCENES[which]))
    try:
        p = rr.default_params(width=1920, height=1080, flags=rr.native.RR_FLAG_PROFILE_KERNELS)
        rgba8 = ctx.render_to_memory(s, 3, p)[1]
        res = []
        for fmt in ("TARGA", "TARGA_RAW"):
            rows = []
            for k in range(reps + 1):  # the first frame warms up
                _, st = ctx.render_frame(s, 3, p, os.path.join(out, f"{which}_{fmt}"), fmt)
                if k:
                    rows.append((st.kernel_ms[rr.native.RR_K_PNG], st.readback_ms, st.encode_ms, st.total_ms))
            data = open(os.path.join(out, f"{which}_{fmt}.tga"), "rb").read()
            assert data == T.encode(rgba8, 4, fmt == "TARGA"), "the file is not the restatement's"
            bound = T.HEADER + 1080 * (T.row_bound(1920, 4) if fmt == "TARGA" else 1920 * 4)
            assert len(data) <= bound, "a file above the all-literal bound"
            m = np.mean(rows, 0)
            r = {"what": "per-frame", "scene": which, "format": fmt, "spp": int(st.spp), "file_bytes": len(data),
                 "bound_bytes": bound, "coder_ms": round(m[0], 3), "coder_ms_min": round(min(x[0] for x in rows), 3),
                 "coder_ms_max": round(max(x[0] for x in rows), 3), "readback_ms": round(m[1], 3),
                 "encode_ms": round(m[2], 3), "total_ms": round(m[3], 3)}
            if fmt == "TARGA":
                pil = pil_rle_bytes(T.expected(rgba8, 4))
                r.update(pil_rle_bytes=pil, file_over_pil=round(len(data) / pil, 4))
                for mode, c in (("RGB", 3), ("BW", 1)):
                    mine, theirs = len(T.encode(rgba8, c, True)), pil_rle_bytes(T.expected(rgba8, c))
                    r[f"{mode}_file_bytes"], r[f"{mode}_pil_rle_bytes"] = mine, theirs
            res.append(r)
        return res
    finally:
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
    ap.add_argument("--format", default="TARGA", choices=["TARGA", "TARGA_RAW", "PNG"])
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--root", default=HERE, help="the checkout whose package and scenes are measured")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    rr = importlib.import_module(PKG)
    out = a.out or tempfile.mkdtemp(prefix="tga_measure_")
    os.makedirs(out, exist_ok=True)
    ctx = rr.RenderContext(0)
    try:
        if a.what == "per-frame":
            sys.path.insert(0, os.path.join(root, "tests"))
            import tga as T
            for which in ("04vs", "02"):
                for r in per_frame(rr, T, root, ctx, which, out):
                    print(json.dumps(r), flush=True)
            return
        s = ctx.load_scene(os.path.join(root, "scenes", SCENES["02"]))
        try:
            if a.format == "PNG":
                ctx.set_device_png(True)
            fps = rate(rr, ctx, s, rr.default_params(width=1920, height=1080), out, a.frames, a.format)
            print(json.dumps({"what": "rate", "scene": "02", "format": a.format, "label": a.label,
                              "frames": a.frames, "fps": round(fps, 3)}), flush=True)
        finally:
            s.close()
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
