"""The output settings without a GPU: tests/cpp/settings_check.cpp links csrc/settings.cpp alone
(host code, no HIP header), is built with the system C++ compiler under AddressSanitizer and
UBSan, and runs as a child process. It checks the RR_* variables' spellings, the setters'
ranges, resolve_output's table and the format table (csrc/formats.hpp) with the refusal texts
made from it; the first test passes when it exits 0. The second holds the package's Python
copy of the extensions to the table the program prints."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT

CSRC = os.path.join(ROOT, PKG, "csrc")


@pytest.fixture(scope="module")
def settings_check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    exe = str(tmp_path_factory.mktemp("settings") / "settings_check")
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
    return exe


def _run(exe, *args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RR_")}
    return subprocess.run([exe, *args], capture_output=True, text=True, env=env)


def test_settings_check_program(settings_check):
    run = _run(settings_check)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "settings_check: ok" in run.stdout


def test_python_extensions_are_the_tables(settings_check, rr):
    """naming.py's EXTENSIONS, the Python copy, names the formats of the C table in its order,
    each with the table's extension."""
    run = _run(settings_check, "--formats")
    assert run.returncode == 0, run.stdout + run.stderr
    table = [tuple(line.split(" ")) for line in run.stdout.splitlines()]
    assert len(table) == 8 and all(len(row) == 2 for row in table), run.stdout
    assert table == list(rr.EXTENSIONS.items())


def test_settings_cpp_is_host_only():
    """settings.cpp and the headers it includes name no HIP header."""
    for name in ("settings.cpp", "settings.hpp", "formats.hpp", "looks.hpp", "scene.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            assert "hip/" not in f.read(), name
