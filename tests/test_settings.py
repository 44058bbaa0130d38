"""The output settings without a GPU: tests/cpp/settings_check.cpp links csrc/settings.cpp alone
(host code, no HIP header), is built with the system C++ compiler under AddressSanitizer and
UBSan, and runs as a child process. It checks the RR_* variables' spellings, the setters'
ranges and resolve_output's table; this test passes when it exits 0."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

CSRC = os.path.join(ROOT, PKG, "csrc")


def test_settings_check_program(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path / "settings_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", CSRC, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "settings_check.cpp"), os.path.join(CSRC, "settings.cpp"), "-o", exe]
    # GCC links the sanitizers' runtimes as shared libraries unless told otherwise; inside the
    # program they do not depend on what else the process loads. (Clang's are static already and
    # it does not know these flags: then the plain command.)
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = {k: v for k, v in os.environ.items() if not k.startswith("RR_")}
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "settings_check: ok" in run.stdout


def test_settings_cpp_is_host_only():
    """settings.cpp and the headers it includes name no HIP header."""
    for name in ("settings.cpp", "settings.hpp", "looks.hpp", "scene.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            assert "hip/" not in f.read(), name
