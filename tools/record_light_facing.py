#!/usr/bin/env python3
"""Records tests/golden/light_facing_counters.json: the ray counters of every
case of tests/test_gpu_light_facing.py, rendered by a library built without
the light-facing rule (tools/ab_variants.sh lf0 "-DRR_LIGHT_FACING=0", the
parent commit's instructions), on the GPU box:

    RR_LIB_PATH=$PWD/ab_builds/lf0/librr.so python tools/record_light_facing.py OUT.json
"""
import importlib
import json
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PKG = "diploma_thesis-distributed_rendering_of_cgi_using_a_render_cluster_amd"


def main():
    rr = importlib.import_module(PKG)
    import test_gpu_light_facing as T

    out = {}
    tmp = pathlib.Path(tempfile.mkdtemp())
    with rr.RenderContext(0) as ctx:
        for name in T.CASES:
            _, _, _, st, cst = T.render_case(ctx, rr, tmp, name)
            out[name] = {"timed": T.TC.counters(st), "counting": T.TC.counters(cst)}
            print(name, out[name], flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
