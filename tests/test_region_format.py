"""The render region without a GPU: the ABI and the header's text, the setter's range, RR_REGION's
spellings, the fraction-to-pixel rule and what a frame resolves to (tests/cpp/region_check.cpp under
ASan / UBSan, a stand-alone program of settings.cpp), the scene's render.border, and the exporter."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import PKG, ROOT

CSRC = os.path.join(ROOT, PKG, "csrc")
S04 = os.path.join(ROOT, "scenes", "04_very-simple-standin.rrscene")
BLENDS = {
    os.path.join(ROOT, "blender-projects", "01_simple-animation", "01_simple-animation.blend"):
        os.path.join(ROOT, "scenes", "01_simple-animation.rrscene"),
    os.path.join(ROOT, "blender-projects", "04_very-simple", "04_very-simple-standin.blend"): S04,
}
NEW = ("rr_set_region", "rr_set_region_off", "rr_set_region_from_scene", "rr_region_resolution",
       "rr_debug_film_window")


def test_abi_has_the_entry_points_and_keeps_its_version(rr):
    lib = rr.lib()
    for name in NEW:
        assert hasattr(lib, name) and name in rr.EXPORTS
    assert lib.rr_abi_version() == 8 == rr.native.RR_ABI_VERSION
    # NULL handles: RR_EINVAL, nothing dereferenced
    assert lib.rr_set_region(None, 0, 0, 1, 1, 0) == -22
    assert lib.rr_set_region_off(None) == -22
    assert lib.rr_set_region_from_scene(None, 1) == -22
    assert lib.rr_region_resolution(None, None, None, None, None) == -22
    assert lib.rr_debug_film_window(None, None, 1, 1, 0, 0, 1, 1, 0, 1.0, None) == -22


def test_header_documents_the_region():
    text = open(os.path.join(ROOT, "include", "rr.h")).read()
    assert re.search(r"#define RR_ABI_VERSION 8\b", text)
    doc = text[text.index("The render region: Blender's render border"):text.index("int rr_set_region(")]
    for word in ("half", "top first", "clamped", "RR_EINVAL", "rr_set_region_off", "crop", "(0, 0, 0, 0)",
                 "A = 0 outside", "dither", "OUTPUT image's own pixel coordinates", "render.border",
                 "rr_set_region_from_scene", "RR_REGION", "not pinned", "rr_region_resolution",
                 "rr_scene_resolution", "tile path", "split path"):
        assert word in doc, word
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, text), name


def test_rule_header_is_host_only_and_states_the_rule():
    text = open(os.path.join(CSRC, "region_rule.h")).read()
    assert "hip/" not in text
    assert "(int)(min_x * W)" in text and "BOTTOM" in text and "unpinned" in text
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "region_rule.h" in design and "render.border" in design


def test_region_check_program(tmp_path):
    """The setter's range, RR_REGION's spellings, the pixel rule at its edges, the clamp and what a
    frame resolves to: a stand-alone program of settings.cpp."""
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "region_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "region_check.cpp"), os.path.join(CSRC, "settings.cpp"), "-o", exe]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("RR_")}
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "region_check: ok" in run.stdout


# ------------------------------------------------------------- the scene ---
def _scene_with(tmp_path, name, border):
    doc = json.load(open(S04))
    doc["render"]["border"] = border
    p = tmp_path / (name + ".rrscene")
    p.write_text(json.dumps(doc))
    return str(p)


@pytest.mark.parametrize("border", [
    {"min_x": 0.1, "max_x": 0.5, "min_y": 0.0, "max_y": 0.2, "crop": True},
    {"min_x": 0.0, "max_x": 1.0, "min_y": 0.0, "max_y": 1.0, "crop": False},
    {"min_x": 0.3, "max_x": 0.3, "min_y": 0.5, "max_y": 0.5},  # empty: parsed; a frame that asks for it is refused
])
def test_scene_field_is_parsed(rr, tmp_path, border):
    rr.Scene(_scene_with(tmp_path, "ok", border)).close()


@pytest.mark.parametrize("bad", [
    True, [0.1, 0.5, 0.0, 0.2], "0.1,0.5,0,0.2",
    {"min_x": 0.1, "max_x": 0.5, "min_y": 0.0},
    {"min_x": "0.1", "max_x": 0.5, "min_y": 0.0, "max_y": 0.2},
    {"min_x": -0.1, "max_x": 0.5, "min_y": 0.0, "max_y": 0.2},
    {"min_x": 0.1, "max_x": 1.5, "min_y": 0.0, "max_y": 0.2},
    {"min_x": 0.1, "max_x": 0.5, "min_y": 0.0, "max_y": 0.2, "crop": 1},
])
def test_scene_field_of_another_shape_is_refused(rr, tmp_path, bad):
    with pytest.raises(rr.RRError) as e:
        rr.Scene(_scene_with(tmp_path, "bad", bad))
    assert e.value.code == -22 and "render.border" in str(e.value)


def test_committed_scenes_have_no_border():
    for f in sorted(os.listdir(os.path.join(ROOT, "scenes"))):
        if f.endswith(".rrscene") and not f.startswith("c5"):
            assert "border" not in json.load(open(os.path.join(ROOT, "scenes", f)))["render"]


@pytest.mark.parametrize("blend", list(BLENDS))
def test_exporter_writes_the_field_only_with_use_border(monkeypatch, blend):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import blend_export as B
    args = argparse.Namespace(samples=128, max_bounces=12, clamp_indirect=10.0, seed=0)
    committed = json.load(open(BLENDS[blend]))
    mine = json.loads(json.dumps(B.export(blend, args)))
    assert "border" not in mine["render"]  # the projects' use_border is clear
    # what the exporter controls is unchanged (a committed scene may carry its own sample settings)
    for key in ("resolution_x", "resolution_y", "resolution_percentage", "view_transform", "filter_width"):
        assert mine["render"][key] == committed["render"][key]
    real = B.BlendFile.read_struct_at

    def patched(self, at, struct, field):
        v = real(self, at, struct, field)
        return v | B.R_BORDER | B.R_CROP if (struct, field) == ("RenderData", "mode") else v
    monkeypatch.setattr(B.BlendFile, "read_struct_at", patched)
    border = B.export(blend, args)["render"]["border"]
    assert sorted(border) == ["crop", "max_x", "max_y", "min_x", "min_y"] and border["crop"] is True
    assert all(0.0 <= border[k] <= 1.0 for k in ("min_x", "max_x", "min_y", "max_y"))


def test_committed_blend_exports_to_its_committed_scene():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import blend_export as B
    blend = next(b for b in BLENDS if "01_simple" in b)
    args = argparse.Namespace(samples=128, max_bounces=12, clamp_indirect=10.0, seed=0)
    assert json.loads(json.dumps(B.export(blend, args))) == json.load(open(BLENDS[blend]))
