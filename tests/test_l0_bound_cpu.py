"""The exclusion bound of the exact l0 search without a GPU (``solver_options={"bound": "exclusion"}``, ``slm_solve_l0_xb``,
``slm_solve_l0_xb_wide``): the sequential restatement the GPU tests lean on against the brute force; the public surface (the
header's entries, the ABI's symbol list and version, the binding, the dataset methods); what is refused before any device
is touched, and that the option reaches the device on the four estimators; and the host side of csrc/l0_host.hpp compiled
with g++ and run on the CPU, plainly and under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/l0_bound_host_test.cpp)."""

import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.optimize import Bounds
from sklearn.datasets import make_regression

from _l0_bound_reference import bounded_search
from _l0_reference import brute_force

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
XB = {"bound": "exclusion"}
FOUR = ("BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L2L0")


# ---- the restatement against the brute force ----------------------------------------------------------------------------------
def same_optimum(got, ref):
    assert got["finished"]
    np.testing.assert_array_equal(got["active"], ref["active"])
    assert abs(got["objective"] - ref["objective"]) <= 1e-10 * abs(ref["objective"])
    assert np.max(np.abs(got["coef"] - ref["coef"])) <= 1e-9 * np.max(np.abs(ref["coef"]))


@pytest.mark.parametrize("n", [40, 10])
def test_restatement_on_the_twelve_column_designs(n):
    X, y = make_regression(n, 12, n_informative=5, noise=1.0, random_state=0)
    alpha = 1e-2 * float(np.var(y))
    W = np.random.default_rng(1).standard_normal((12, 12))
    hier = [[] for _ in range(12)]
    hier[3] = [0]
    for kw in (dict(K=1), dict(K=3), dict(K=5), dict(alpha=alpha), dict(alpha=1e-4 * float(np.var(y))), dict(alpha=alpha, eta=0.1, W=W),
               dict(K=5, big_M=50.0), dict(K=4, hierarchy=hier)):
        kw.setdefault("big_M", 1000.0)
        ref = brute_force(X, y, **kw)
        assert ref["gap"] > 1e-6
        got, plain = bounded_search(X, y, **kw), bounded_search(X, y, bound="q_all", **kw)
        print(f"{sorted(kw)}: nodes {got['nodes']} with the exclusion bound, {plain['nodes']} without")
        same_optimum(got, ref)
        same_optimum(plain, ref)
        assert got["nodes"] <= plain["nodes"]


def test_restatement_on_sixteen_grouped_columns_with_a_hierarchy():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((50, 16))
    groups = np.array([0, 0, 1, 2, 2, 2, 3, 4, 4, 5, 6, 6, 7, 8, 8, 9])
    y = X[:, [2, 6, 12]] @ np.array([2.0, -1.5, 1.0]) + 0.7 * X[:, 9] + 0.5 * rng.standard_normal(50)
    hier = [[] for _ in range(10)]
    hier[1], hier[7], hier[3] = [4], [1], [9]  # a chain 7 -> 1 -> 4, and 3 -> 9
    for kw in (dict(K=3), dict(K=5), dict(alpha=0.02 * float(np.var(y)))):
        ref = brute_force(X, y, groups=groups, hierarchy=hier, big_M=1000.0, **kw)
        free = brute_force(X, y, groups=groups, big_M=1000.0, **kw)
        assert ref["gap"] > 1e-6
        got = bounded_search(X, y, groups=groups, hierarchy=hier, big_M=1000.0, **kw)
        same_optimum(got, ref)
        print(f"{sorted(kw)}: nodes {got['nodes']}, the hierarchy changed the answer: {not np.array_equal(ref['active'], free['active'])}")
    assert not np.array_equal(brute_force(X, y, groups=groups, hierarchy=hier, K=3)["active"], brute_force(X, y, groups=groups, K=3)["active"])


# ---- the public surface -------------------------------------------------------------------------------------------------------
def test_abi_names_the_bound_entries_and_keeps_its_version():
    from sparselm_amd import _engine

    assert _engine.ABI_VERSION == 24
    with open(os.path.join(ROOT, "include", "slm_engine.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "binding.cpp")) as fh:
        binding = fh.read()
    assert "#define SLM_ABI_VERSION 24" in header
    for name in ("solve_l0_xb", "solve_l0_xb_wide"):
        assert f"slm_{name}" in _engine.ABI_SYMBOLS and f"int slm_{name}(" in header and hasattr(_engine.Dataset, name)
        assert f"slm_{name}(" in binding and f'm.def("{name}"' in binding
    for name in ("slm_solve_l0", "slm_solve_l0_wide", "slm_solve_l0_l1", "slm_solve_l0_profile", "slm_solve_l0_constrained"):
        assert name in _engine.ABI_SYMBOLS and f"int {name}(" in header
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "l0_host.hpp")) as fh:
        host = fh.read()
    assert "constexpr int L0_XCAP = " in host and "constexpr double l0_excl_bound(" in host


def test_the_library_exports_the_bound_entries():
    from sparselm_amd import _engine

    lib = _engine.load_library()
    assert lib.slm_abi_version() == 24
    for name in ("slm_solve_l0_xb", "slm_solve_l0_xb_wide"):
        assert hasattr(lib, name)
    b = _engine.load_binding()
    if b is not None:
        assert hasattr(b, "solve_l0_xb") and hasattr(b, "solve_l0_xb_wide")


# ---- refusals before any device -----------------------------------------------------------------------------------------------
@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to open an engine fails the test: validation errors have to come first."""
    from sparselm_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were validated")

    monkeypatch.setattr(_engine, "get_engine", boom)


def test_the_option_reaches_the_device_on_the_four_estimators(no_device):
    from sparselm_amd import model

    X, y = make_regression(30, 8, n_informative=3, random_state=0)
    for name in FOUR:
        for options in (XB, {"bound": "q_all"}, {"bound": "exclusion", "wide": True}):
            with pytest.raises(AssertionError, match="device was touched"):
                getattr(model, name)(solver_options=options).fit(X, y)


def test_bad_bound_options_raise_before_any_device(no_device):
    from sparselm_amd import model
    from sparselm_amd.miqp import L1L0, l0_profile

    X, y = make_regression(30, 8, n_informative=3, random_state=0)
    for name in FOUR:
        for bad in ("exclude", True, None, 1):
            with pytest.raises(ValueError, match="bound"):
                getattr(model, name)(solver_options={"bound": bad}).fit(X, y)
        est = getattr(model, name)(solver_options=XB).add_constraints(Bounds(-1.0, 1.0))
        with pytest.raises(ValueError, match="constraints and solver_options\\['bound'\\]"):
            est.fit(X, y)
    for eta in (0.1, 0.0):
        with pytest.raises(ValueError, match="no exclusion bound"):
            L1L0(alpha=1.0, eta=eta, solver_options=XB).fit(X, y)
    with pytest.raises(ValueError, match="l0_profile takes no solver_options\\['bound'\\]"):
        l0_profile(X, y, max_groups=2, solver_options=XB)
    with pytest.raises(ValueError, match="l0_profile takes no solver_options\\['bound'\\]"):
        l0_profile(X, y, max_groups=2, solver_options={"bound": "q_all"})
    with pytest.raises(AssertionError, match="device was touched"):  # ... and without the option they get as far as the device
        L1L0(alpha=1.0, eta=0.1).fit(X, y)
    with pytest.raises(AssertionError, match="device was touched"):
        l0_profile(X, y, max_groups=2)


def test_clone_carries_the_option():
    from sklearn.base import clone

    from sparselm_amd.model import L2L0

    est = L2L0(alpha=0.1, eta=0.2, solver_options=dict(XB))
    assert clone(est).solver_options == XB and clone(est).get_params()["solver_options"] == XB


# ---- the host side, on the CPU ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_l0_bound_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l0_bound_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "l0_bound_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "l0_bound_host_test: ok" in run.stdout and "worst overshoot" in run.stdout
