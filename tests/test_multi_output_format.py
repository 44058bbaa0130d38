"""Several files from one frame, without a GPU: the ABI, RR_EXTRA_OUTPUTS' spellings, derived
paths, collisions and factors (tests/cpp/multi_output_check.cpp under ASan / UBSan), the scene's
render.use_preview, the exporter, and the host statement of csrc/reduce_rule.h against the
numpy restatement (tests/reduce.py)."""
import argparse
import ctypes
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import reduce as R
from conftest import PKG, ROOT

CSRC = os.path.join(ROOT, PKG, "csrc")
S04 = os.path.join(ROOT, "scenes", "04_very-simple-standin.rrscene")
S01 = os.path.join(ROOT, "scenes", "01_simple-animation.rrscene")
BLEND01 = os.path.join(ROOT, "blender-projects", "01_simple-animation", "01_simple-animation.blend")
NEW = ("rr_frame_submit_outputs", "rr_render_frame_outputs", "rr_last_output_bytes", "rr_set_extra_outputs",
       "rr_debug_film_reduce")


def test_abi_has_the_entry_points_and_keeps_its_version(rr):
    lib = rr.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in rr.EXPORTS
    assert lib.rr_abi_version() == 8
    assert rr.native.RR_MAX_FRAME_OUTPUTS == 4
    assert ctypes.sizeof(rr.native.FrameOutput) == 24
    assert [f for f, _ in rr.native.FrameOutput._fields_] == ["out_path", "format", "jpeg_quality", "reduce"]
    # NULL handles: RR_EINVAL, nothing dereferenced
    t = ctypes.c_uint64()
    assert lib.rr_frame_submit_outputs(None, None, 1, None, None, 1, ctypes.byref(t)) == -22
    assert lib.rr_render_frame_outputs(None, None, 1, None, None, 1, None, None) == -22
    assert lib.rr_last_output_bytes(None, 0, ctypes.byref(t)) == -22
    assert lib.rr_set_extra_outputs(None, b"JPEG:2") == -22


def test_header_documents_the_struct_and_the_limit():
    text = open(os.path.join(ROOT, "include", "rr.h")).read()
    assert "#define RR_MAX_FRAME_OUTPUTS 4\n" in text and "#define RR_ABI_VERSION 8\n" in text
    body = text[text.index("typedef struct rr_frame_output {"):text.index("} rr_frame_output;")]
    assert [ln.split(";")[0].split()[-1] for ln in body.splitlines()[1:] if ";" in ln] == \
        ["out_path", "format", "jpeg_quality", "reduce"]
    doc = text[text.index("Files every frame of ctx"):text.index("int rr_set_extra_outputs(")]
    assert "RR_EXTRA_OUTPUTS" in doc and "use_preview" in doc and "Not pinned" in doc


def test_multi_output_check_program(tmp_path):
    """Every spelling of RR_EXTRA_OUTPUTS, the derived paths, what a context and a scene add, the
    list's refusals and the rule header's host side: a stand-alone program of settings.cpp."""
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "multi_output_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "multi_output_check.cpp"), os.path.join(CSRC, "settings.cpp"), "-o", exe]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("RR_")}
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "multi_output_check: ok" in run.stdout


def test_rule_header_is_host_only():
    with open(os.path.join(CSRC, "reduce_rule.h")) as f:
        assert "hip/" not in f.read()


# ------------------------------------------------------------- the scene ---
def _scene_with(tmp_path, name, **render):
    doc = json.load(open(S04))
    doc["render"].update(render)
    p = tmp_path / (name + ".rrscene")
    p.write_text(json.dumps(doc))
    return str(p)


@pytest.mark.parametrize("value", [True, False])
def test_scene_field_is_parsed(rr, tmp_path, value):
    rr.Scene(_scene_with(tmp_path, "ok", use_preview=value)).close()


@pytest.mark.parametrize("bad", ["true", 1, 0, None, "JPEG", [True]])
def test_scene_field_of_another_type_is_refused(rr, tmp_path, bad):
    with pytest.raises(rr.RRError) as e:
        rr.Scene(_scene_with(tmp_path, "bad", use_preview=bad))
    assert e.value.code == -22 and "render.use_preview" in str(e.value)


def test_committed_scenes_have_no_preview():
    for f in sorted(os.listdir(os.path.join(ROOT, "scenes"))):
        if f.endswith(".rrscene") and not f.startswith("c5"):
            assert "use_preview" not in json.load(open(os.path.join(ROOT, "scenes", f)))["render"]


def test_exporter_writes_the_field_only_when_set(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import blend_export as B
    args = argparse.Namespace(samples=128, max_bounces=12, clamp_indirect=10.0, seed=0)
    assert json.loads(json.dumps(B.export(BLEND01, args))) == json.load(open(S01))  # the project's flag: clear
    real = B.BlendFile.read_struct_at

    def patched(self, at, struct, field):
        v = real(self, at, struct, field)
        return v | B.R_IMF_FLAG_PREVIEW_JPG if (struct, field) == ("ImageFormatData", "flag") else v
    monkeypatch.setattr(B.BlendFile, "read_struct_at", patched)
    assert B.export(BLEND01, args)["render"]["use_preview"] is True


# --------------------------------------------------------------- the rule ---
@pytest.mark.parametrize("k", R.FACTORS)
@pytest.mark.parametrize("w,h", R.SIZES)
def test_host_reduction_is_the_numpy_rule(rr, w, h, k):
    for name, img in R.images(w, h).items():
        want = R.reduce(img, k)
        assert want.shape == R.reduced_shape(h, w, k) + (4,)
        got = rr.native.film_reduce(img, k)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, w, h, k)
        assert np.all(np.isfinite(want))


@pytest.mark.parametrize("k", R.FACTORS)
def test_numpy_rule_is_the_rule_as_written(k):
    """The vectorised restatement against the pixel-by-pixel one, and against hand-worked blocks."""
    for w, h in R.SIZES:
        for img in R.images(w, h, seed=1).values():
            assert np.array_equal(R.reduce(img, k).view(np.uint32), R.reduce_scalar(img, k).view(np.uint32))
    img = np.arange(1, 10, dtype=np.float32).reshape(3, 3, 1).repeat(4, axis=2)
    assert R.reduce(img, 2)[..., 0].tolist() == [[3.0, 4.5], [7.5, 9.0]]
    assert R.reduce(img, 8)[..., 0].tolist() == [[5.0]]
    # the order of the sum shows: ((1e8 + 1) - 1e8) + 1 is 1 in float32
    row = np.zeros((1, 4, 4), np.float32)
    row[0, :, 0] = [1e8, 1.0, -1e8, 1.0]
    assert R.reduce(row, 4)[0, 0, 0] == np.float32(0.25)


def test_a_constant_image_reduces_to_itself_only_where_the_sum_is_exact(rr):
    """0.1 is not a sum-exact value: the mean of 64 of them differs from 0.1 in float32, and host
    and numpy agree on by how much. A power of two stays what it is."""
    img = np.full((16, 16, 4), np.float32(0.1), np.float32)
    assert np.array_equal(rr.native.film_reduce(img, 8), R.reduce(img, 8))
    two = np.full((9, 9, 4), np.float32(0.25), np.float32)
    for k in R.FACTORS:
        assert np.all(rr.native.film_reduce(two, k) == np.float32(0.25))


@pytest.mark.parametrize("bad", [0, 3, 5, 16, -2])
def test_factor_is_validated(rr, bad):
    with pytest.raises(rr.RRError) as e:
        rr.native.film_reduce(np.zeros((4, 4, 4), np.float32), bad)
    assert e.value.code == -22 and "1, 2, 4 or 8" in str(e.value)
