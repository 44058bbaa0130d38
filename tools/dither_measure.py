#!/usr/bin/env python3
"""Measurements of profiles/dither.md: file sizes of frame 3 of the 04vs
stand-in at 1920x1080 (scene spp) as JPEG q90 and as 8-bit PNG with the host
and the device coder, at dither intensity 0 and 1, and the time of the view
pass the dither adds (kernel_ms[RR_K_ACCUM] with RR_FLAG_PROFILE_KERNELS: an
04vs frame without dither has no launch of that class). Mean of 5 serial
frames after a warm-up. Prints one JSON document.

    python tools/dither_measure.py
"""
import importlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
rr = importlib.import_module("diploma_thesis-distributed_rendering_of_cgi_using_a_render_cluster_amd")
S04 = os.path.join(ROOT, "scenes", "04_very-simple-standin.rrscene")
RR_K_ACCUM, RR_K_TILES = 4, 6


def main():
    out = {}
    tmp = tempfile.mkdtemp()
    with rr.RenderContext(0) as c:
        s = c.load_scene(S04)
        p = rr.default_params(flags=rr.native.RR_FLAG_PROFILE_KERNELS)
        for g in (0.0, 1.0):
            c.set_dither(g)
            row = {}
            for name, fmt, dev in (("jpeg_q90", "JPEG", False), ("png_host", "PNG", False),
                                   ("png_device", "PNG", True)):
                c.set_device_png(dev)
                c.render_frame(s, 3, p, os.path.join(tmp, "warm"), fmt, 90)
                view, trace = [], []
                for _ in range(5):
                    _, st = c.render_frame(s, 3, p, os.path.join(tmp, f"{name}_{g}"), fmt, 90)
                    view.append(st.kernel_ms[RR_K_ACCUM])
                    trace.append(st.trace_ms)
                row[name] = {"bytes": int(st.output_bytes), "view_pass_ms": sum(view) / 5,
                             "view_pass_launches": int(st.kernel_launches[RR_K_ACCUM]),
                             "trace_ms": sum(trace) / 5, "k_tiles_ms": st.kernel_ms[RR_K_TILES],
                             "size": [st.width, st.height], "spp": st.spp}
            out[str(g)] = row
        s.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
