"""The wide exact l0 search without a GPU (``solver_options={"wide": True}``, ``slm_solve_l0_wide``,
``slm_solve_l0_profile_wide``): the public surface (the header's entries, the ABI's symbol list and version, the binding,
the dataset methods); what is refused before any device is touched; the split of 128-bit ``need`` masks into words; and the
wide part of csrc/l0_host.hpp compiled with g++ and run on the CPU, plainly and under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/l0_wide_host_test.cpp).  The refusals the engine itself makes (129 columns, row-sharded
datasets, bad ``need`` bits) need a device and sit at the end, marked ``gpu``."""

import os
import shutil
import subprocess
import types

import numpy as np
import pytest
from sklearn.datasets import make_regression

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
WIDE = {"wide": True}


# ---- the public surface -------------------------------------------------------------------------------------------------------
def test_abi_names_the_wide_entries_and_keeps_its_version():
    from sparselm_amd import _engine

    assert _engine.ABI_VERSION == 24
    with open(os.path.join(ROOT, "include", "slm_engine.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "binding.cpp")) as fh:
        binding = fh.read()
    assert "#define SLM_ABI_VERSION 24" in header
    for name in ("solve_l0_wide", "solve_l0_profile_wide"):
        assert f"slm_{name}" in _engine.ABI_SYMBOLS and f"int slm_{name}(" in header and hasattr(_engine.Dataset, name)
        assert f"slm_{name}(" in binding and f'm.def("{name}"' in binding
    # the narrow entries are still there, as they were
    for name in ("slm_solve_l0", "slm_solve_l0_l1", "slm_solve_l0_profile"):
        assert name in _engine.ABI_SYMBOLS and f"int {name}(" in header


def test_the_limits_are_the_header_s():
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "l0_host.hpp")) as fh:
        host = fh.read()
    assert "constexpr int L0_PMAX = 64;" in host and "constexpr int L0_WIDE_PMAX = 128;" in host


def test_need_masks_are_split_into_two_words():
    from sparselm_amd import _engine

    ds = types.SimpleNamespace(n_groups=3)
    words = _engine.Dataset._need_words(ds, [0, (1 << 70) | 5, (1 << 127) | (1 << 63)])
    assert words.dtype == np.uint64 and words.shape == (3, 2) and words.flags.c_contiguous
    assert words.tolist() == [[0, 0], [5, 1 << 6], [1 << 63, 1 << 63]]
    assert _engine.Dataset._need_words(ds, None) is None
    for bad in ([0, 0], [0, 0, 1 << 128], [0, -1, 0]):
        with pytest.raises(ValueError):
            _engine.Dataset._need_words(ds, bad)


# ---- refusals before any device -----------------------------------------------------------------------------------------------
@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to open an engine fails the test: validation errors have to come first."""
    from sparselm_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were validated")

    monkeypatch.setattr(_engine, "get_engine", boom)


def test_l1l0_has_no_wide_mode(no_device):
    from sparselm_amd.miqp import L1L0

    X, y = make_regression(30, 8, n_informative=3, random_state=0)
    with pytest.raises(ValueError, match="no wide mode"):
        L1L0(alpha=1.0, eta=0.1, solver_options=WIDE).fit(X, y)
    with pytest.raises(ValueError, match="no wide mode"):
        L1L0(alpha=1.0, eta=0.0, solver_options=WIDE).fit(X, y)  # (whatever its eta)
    # ... and without the option it gets as far as the device
    with pytest.raises(AssertionError, match="device was touched"):
        L1L0(alpha=1.0, eta=0.1, solver_options={"wide": False}).fit(X, y)


def test_bad_wide_options_raise_before_any_device(no_device):
    from sparselm_amd import model
    from sparselm_amd.miqp import l0_profile

    X, y = make_regression(30, 8, n_informative=3, random_state=0)
    for name in ("BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L2L0"):
        with pytest.raises(ValueError, match="wide"):
            getattr(model, name)(solver_options={"wide": "yes"}).fit(X, y)
        with pytest.raises(ValueError, match="unknown solver_options"):
            getattr(model, name)(solver_options={"wide": True, "width": 128}).fit(X, y)
        with pytest.raises(AssertionError, match="device was touched"):
            getattr(model, name)(solver_options=WIDE).fit(X, y)
    with pytest.raises(ValueError, match="wide"):
        l0_profile(X, y, solver_options={"wide": 1})
    with pytest.raises(ValueError):
        l0_profile(X, y, hierarchy=[[1]] * 7, solver_options=WIDE)  # a wrong length, as before
    with pytest.raises(AssertionError, match="device was touched"):
        l0_profile(X, y, max_groups=2, solver_options=WIDE)


def test_hierarchy_masks_reach_the_high_word(no_device):
    """More than 64 groups: the masks of the hierarchy are Python integers with bits beyond 63 -- and a wrong length or an
    unknown label still raises before any device."""
    from sparselm_amd.model import BestSubsetSelection
    from sparselm_amd.model._miqp import _hierarchy_masks

    need = _hierarchy_masks([[79]] + [[] for _ in range(78)] + [[0, 64]], None, 80)
    assert need[0] == 1 << 79 and need[79] == (1 << 64) | 1 and not any(need[1:79])
    X, y = make_regression(100, 80, n_informative=3, random_state=0)
    with pytest.raises(ValueError):
        BestSubsetSelection(hierarchy=[[1]] * 79, solver_options=WIDE).fit(X, y)
    with pytest.raises(ValueError):
        BestSubsetSelection(hierarchy=[[80]] + [[]] * 79, solver_options=WIDE).fit(X, y)


# ---- the host side, on the CPU ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_l0_wide_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l0_wide_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "l0_wide_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "l0_wide_host_test: ok" in run.stdout


# ---- what the engine itself refuses (these need a device) ----------------------------------------------------------------------
@pytest.mark.gpu
def test_129_columns_are_refused_by_the_engine():
    from sparselm_amd.miqp import l0_profile
    from sparselm_amd.model import BestSubsetSelection, RegularizedL0

    X, y = make_regression(160, 129, n_informative=5, random_state=2)
    with pytest.raises(NotImplementedError, match="128"):
        BestSubsetSelection(sparse_bound=1, solver_options=WIDE).fit(X, y)
    with pytest.raises(NotImplementedError, match="128"):
        RegularizedL0(alpha=1.0, hierarchy=[[1]] + [[]] * 128, solver_options=WIDE).fit(X, y)
    with pytest.raises(NotImplementedError, match="128"):
        l0_profile(X, y, max_groups=1, solver_options=WIDE)
    with pytest.raises(NotImplementedError, match="64"):  # the wide profile keeps one size per lane
        l0_profile(X[:, :100], y, max_groups=65, solver_options=WIDE)


@pytest.mark.gpu
def test_row_sharded_datasets_and_bad_need_are_refused():
    from sparselm_amd import _engine
    from sparselm_amd import distributed as D

    X, y = make_regression(100, 70, n_informative=5, random_state=2)
    eng = _engine.Engine(0)
    try:
        D.init_row_sharding(eng, rank=0, world_size=1)
        with eng.dataset(X, y) as ds:
            ds.set_global_rows(len(y))
            with pytest.raises(NotImplementedError, match="row-sharded"):
                ds.solve_l0_wide(max_groups=2)
            with pytest.raises(NotImplementedError, match="row-sharded"):
                ds.solve_l0_profile_wide(max_groups=2)
    finally:
        eng.comm_destroy()
        eng.close()
    with _engine.get_engine().dataset(X, y) as ds:
        for route in (False, True):
            with pytest.raises(ValueError, match="need must have"):
                ds.solve_l0_wide(need=[0] * 69, binding=route)
            with pytest.raises(ValueError, match="need must have"):
                ds.solve_l0_profile_wide(need=[0] * 71, binding=route)
            with pytest.raises(ValueError, match="beyond n_groups"):
                ds.solve_l0_wide(need=[1 << 70] + [0] * 69, binding=route)  # a bit of the high word at the group count
            with pytest.raises(ValueError, match="beyond n_groups"):
                ds.solve_l0_profile_wide(need=[0] * 69 + [1 << 127], max_groups=2, binding=route)
