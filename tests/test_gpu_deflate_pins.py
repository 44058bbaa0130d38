"""The three deflate-backed formats (8-bit PNG, 16-bit PNG, OPEN_EXR) write the
bytes they wrote before the coder was split into deflate.hip and one front-end
kernel template: SHA-256 and length of the files the debug entry points return,
recorded from the commit before the split in tests/golden/deflate_pins.json.

The inputs are the other tests' generators with seed 0. EXR: `bits` takes the
raw-chunk path (k_exr_raw); at W = 8193 the distance 4W leaves the 32 KB window.
16-bit PNG: at W = 4096 the row above (8W + 1) leaves it. 8-bit PNG: at
W = 8200 the row above (4W + 1) does.

    python tests/test_gpu_deflate_pins.py OUT.json   # records the running build's digests
"""
import hashlib
import json
import os
import sys

import pytest

if __name__ == "__main__":  # before the imports below: the repository root (the package, oracle/)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import exr_reader as X
import png16_reader as P
from oracle import png_cases

pytestmark = pytest.mark.gpu

PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate_pins.json")
PNG16_SCALE = 1.25  # exposure scale of the 16-bit cases (as tests/test_gpu_png16.py)
VIEWS = {"standard": 0, "raw": 1}

CASES = [("exr", kind, w, h) for kind in ("flat", "grey", "bits") for w, h in ((1, 1), (5, 33), (129, 16), (8193, 3))]
CASES += [(f"png16-{view}", kind, w, h) for kind in ("flat", "grey", "noise") for view in sorted(VIEWS)
          for w, h in ((1, 1), (3, 17), (513, 16), (4096, 17))]
CASES += [("png8", "noise", 17, 9), ("png8", "flat", 1, 300), ("png8", "gradient", 8200, 3)]


def case_id(case):
    return "%s-%s-%dx%d" % case


def encode(ctx, case):
    fmt, kind, w, h = case
    if fmt == "exr":
        return ctx.exr_device(X.make_image(kind, w, h, seed=0))
    if fmt == "png8":
        return ctx.png_device(png_cases.kind_image(kind, w, h, seed=0))
    return ctx.png16_device(P.make_image(kind, w, h, seed=0), VIEWS[fmt.split("-")[1]], PNG16_SCALE)


def digest(data):
    return [hashlib.sha256(data).hexdigest(), len(data)]


@pytest.fixture(scope="module")
def pins():
    with open(PINS) as f:
        return json.load(f)


def test_every_case_is_pinned(pins):
    assert sorted(pins) == sorted(case_id(c) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_file_bytes_are_the_pinned_ones(ctx, pins, case):
    got = digest(encode(ctx, case))
    print(f"{case_id(case)}: {got[1]} bytes, sha256 {got[0][:16]}")
    assert got == pins[case_id(case)]


if __name__ == "__main__":
    import importlib

    rr = importlib.import_module("diploma_thesis-distributed_rendering_of_cgi_using_a_render_cluster_amd")
    with rr.RenderContext(0) as c:
        out = {case_id(case): digest(encode(c, case)) for case in CASES}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
