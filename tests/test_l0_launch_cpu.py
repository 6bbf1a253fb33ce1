"""What every exact-l0 entry's launch shares, without a GPU: the layout of the device block, the winner among the waves'
results and the way back to the caller's groups and columns (the end of csrc/l0_host.hpp, called by csrc/engine_l0.hip),
compiled with g++ and run on the CPU, plainly and under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/l0_launch_host_test.cpp)."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("sanitize", [False, True])
def test_l0_launch_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l0_launch_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "l0_launch_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "l0_launch_host_test: ok" in run.stdout
