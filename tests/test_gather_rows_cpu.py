"""slm_host::gather_row_blocks / xty_part_rows -- the row blocks of the working set's gather and the rows of partial sums of
X_W^T y it writes into the Gram's partial block (csrc/host_logic.hpp, csrc/ws_kernels.hpp) -- walked on the CPU under
AddressSanitizer + UndefinedBehaviorSanitizer: tests/gather_rows_test.cpp, a stand-alone program with its own main."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_gather_rows_cover_every_tile_and_fit_the_buffer(tmp_path):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "gather_rows_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "gather_rows_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "gather_rows_test: ok" in run.stdout
