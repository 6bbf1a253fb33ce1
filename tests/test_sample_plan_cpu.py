"""slm_host::sample_plan -- the (column block, row block) grid of the opening's sample product on the fp32 image of the
sample rows (csrc/host_logic.hpp, csrc/sample_kernels.hpp) -- walked on the CPU under AddressSanitizer +
UndefinedBehaviorSanitizer: tests/sample_plan_test.cpp, a stand-alone program with its own main."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_sample_plan_covers_every_entry_once(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "sample_plan_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "sample_plan_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "sample_plan_test: ok" in run.stdout
