"""``l1l0_profile`` without a GPU: validation before any device is touched, the public surface (import path, the two C entries
in the header, ``ABI_SYMBOLS``, the ``Dataset`` methods, the binding), the arithmetic of ``L1L0Profile`` on a hand-made table --
a SATURATED one among them: under an l1 term the sizes beyond the lasso's own support tie in value --, the brute-force
reference the GPU tests compare against (tests/_l1l0_profile_reference.py) against ``brute_force_l1``, and the host side of the
l1 profile in csrc/l0_host.hpp compiled with g++ and run on the CPU, plainly and under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/l1l0_profile_host_test.cpp)."""

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
from sklearn.datasets import make_regression

from _l1l0_profile_reference import profile_table_l1
from _l1l0_reference import brute_force_l1

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRIES = ("slm_solve_l0_l1_profile", "slm_solve_l0_l1_profile_wide")


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to open an engine fails the test: validation errors have to come first."""
    from sparselm_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were validated")

    monkeypatch.setattr(_engine, "get_engine", boom)


# ---- validation ---------------------------------------------------------------------------------------------------------------
def test_bad_input_raises_before_any_device(no_device):
    from sparselm_amd.miqp import l1l0_profile

    X, y = make_regression(25, 6, n_informative=3, random_state=0)
    for bad in (dict(eta=-1.0), dict(eta=np.inf), dict(eta=np.nan), dict(eta="much"),
                dict(eta=0.1, alpha_min=-1.0), dict(eta=0.1, alpha_min=np.inf), dict(eta=0.1, alpha_min=np.nan),
                dict(eta=0.1, max_groups=7), dict(eta=0.1, max_groups=-1), dict(eta=0.1, big_M=-1),
                dict(eta=0.1, solver_options={"bound": "exclusion"}), dict(eta=0.1, solver_options={"bound": "q_all"}),
                dict(eta=0.1, solver_options={"tol": 1e-8}), dict(eta=0.1, solver_options={"wide": 1}),
                dict(eta=0.1, hierarchy=[[1]] * 5), dict(eta=0.1, hierarchy=[[9], [], [], [], [], []]), dict(eta=0.1, groups=[0, 0, 1]),
                dict(eta=0.1, fit_intercept="yes"), dict(eta=0.1, sample_weight=np.ones(24))):
        with pytest.raises(ValueError):
            l1l0_profile(X, y, **bad)
    with pytest.raises(ValueError):
        l1l0_profile(X, y[:-1], eta=0.1)
    with pytest.raises(ValueError, match="bound"):
        l1l0_profile(X, y, eta=0.1, solver_options={"bound": "exclusion"})
    # eta has no default and everything after y is keyword-only
    with pytest.raises(TypeError):
        l1l0_profile(X, y)
    with pytest.raises(TypeError):
        l1l0_profile(X, y, 0.1)


def test_signature():
    from sparselm_amd.miqp import l1l0_profile

    params = inspect.signature(l1l0_profile).parameters
    assert list(params) == ["X", "y", "eta", "groups", "max_groups", "alpha_min", "big_M", "hierarchy", "fit_intercept", "sample_weight",
                            "solver_options"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in params.items() if k not in ("X", "y"))
    assert params["eta"].default is inspect.Parameter.empty
    assert [params[k].default for k in list(params)[3:]] == [None, None, 0.0, 100, None, False, None, None]
    assert "l1 weight" in l1l0_profile.__doc__.lower() and "ridge" in l1l0_profile.__doc__.lower()


# ---- the public surface -------------------------------------------------------------------------------------------------------
def test_abi_names_the_two_entries_and_keeps_its_version():
    from sparselm_amd import _engine

    assert _engine.ABI_VERSION == 24
    with open(os.path.join(ROOT, "include", "slm_engine.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "binding.cpp")) as fh:
        binding = fh.read()
    assert "#define SLM_ABI_VERSION 24" in header
    for name in ENTRIES:
        assert name in _engine.ABI_SYMBOLS
        assert f"int {name}(" in header
        assert f"{name}(" in binding and f'm.def("{name[4:]}"' in binding
        assert hasattr(_engine.Dataset, name[4:])
    # the entries that were there are still there
    for name in ("slm_solve_l0_l1", "slm_solve_l0_profile", "slm_solve_l0_profile_wide", "slm_solve_l0_profile_batch"):
        assert name in _engine.ABI_SYMBOLS and f"int {name}(" in header
    # the arguments, as the issue states them: no ridge term and no T
    for name in ENTRIES:
        decl = header[header.index(f"int {name}("):]
        decl = decl[: decl.index(";")]
        for arg in ("alpha_min", "max_groups", "eta_l1", "big_M", "need", "max_nodes", "beta_out", "support_out", "value_out", "nodes_out",
                    "info"):
            assert arg in decl, (name, arg)
        assert "double eta," not in decl and "* T" not in decl


def test_import_path_and_all_is_unchanged():
    import sparselm_amd.miqp as miqp
    from sparselm_amd.model._l0_profile import L0Profile

    assert miqp.__all__ == ["BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L1L0", "L2L0"]
    assert callable(miqp.l1l0_profile) and issubclass(miqp.L1L0Profile, L0Profile)
    assert callable(miqp.l0_profile) and callable(miqp.l0_profile_cv)  # (what was there stays)


def test_pinned_refusals_stay(no_device):
    """``L1L0`` keeps refusing ``wide``, ``bound`` and constraints; ``l0_profile`` keeps refusing ``bound``: the new entry is
    beside them, not in their place."""
    from scipy.optimize import Bounds

    from sparselm_amd.miqp import L1L0, l0_profile

    X, y = make_regression(25, 6, n_informative=3, random_state=0)
    with pytest.raises(ValueError, match="no wide mode"):
        L1L0(solver_options={"wide": True}).fit(X, y)
    with pytest.raises(ValueError, match="exclusion bound"):
        L1L0(solver_options={"bound": "exclusion"}).fit(X, y)
    with pytest.raises(ValueError, match="constraints"):
        L1L0().add_constraints(Bounds(-1, 1)).fit(X, y)
    with pytest.raises(ValueError, match="bound"):
        l0_profile(X, y, solver_options={"bound": "exclusion"})


# ---- the table's arithmetic -----------------------------------------------------------------------------------------------------
def hand_made(values, alpha_min=0.0, eta=0.25):
    from sparselm_amd.miqp import L1L0Profile

    values = np.asarray(values, dtype=float)
    K = len(values) - 1
    supports = np.tril(np.ones((K + 1, K), dtype=bool), -1)  # row k: the first k groups
    supports[~np.isfinite(values)] = False
    coefs = supports * (np.arange(K + 1)[:, None] + 0.5)
    info = {"proven_optimal": True, "status": "optimal", "nodes": 0, "launches": 1, "q_all": float(np.min(values)), "descents": 0}
    return L1L0Profile(values, supports, coefs, np.arange(K + 1, dtype=float), alpha_min, eta, info)


def test_profile_arithmetic_on_a_saturated_table():
    # the lasso on all columns uses three groups: sizes 3, 4 and 5 tie exactly
    prof = hand_made([0.0, -5.0, -8.0, -9.0, -9.0, -9.0])
    assert prof.eta_ == 0.25 and prof.alpha_min_ == 0.0 and prof.max_groups_ == 5 and prof.proven_optimal_
    # ties go to the smaller size, at alpha = 0 and in best subset at every bound beyond the saturation
    assert prof.regularized_size(0.0) == 3
    assert [prof.best_subset_size(b) for b in range(6)] == [0, 1, 2, 3, 3, 3]
    assert prof.regularized_size(0.5) == 3 and prof.regularized_size(1.0) == 2  # (at 1.0 sizes 2 and 3 tie: the smaller)
    assert prof.regularized_size(2.0) == 2 and prof.regularized_size(3.0) == 1 and prof.regularized_size(4.0) == 1
    assert prof.regularized_size(5.0) == 0 and prof.regularized_size(100.0) == 0
    coef, intercept, active = prof.regularized(2.0)
    assert active.tolist() == [True, True, False, False, False] and intercept == 2.0 and coef.tolist() == [2.5, 2.5, 0, 0, 0]
    coef[0] = 99.0  # a copy: the table is not changed through what it hands out
    assert prof.coefs_[2, 0] == 2.5
    # the path: the saturated sizes are on no envelope
    alphas, sizes = prof.alpha_breakpoints()
    assert sizes.tolist() == [0, 1, 2, 3] and alphas.tolist() == [5.0, 3.0, 1.0]
    for bad in (-1, 6):
        with pytest.raises(ValueError):
            prof.best_subset_size(bad)
    with pytest.raises(ValueError):
        prof.regularized_size(np.nan)


def test_profile_arithmetic_on_a_pruned_table():
    prof = hand_made([0.0, -5.0, -8.0, np.inf, -9.0], alpha_min=0.75)
    assert prof.alpha_min_ == 0.75 and not prof.supports_[3].any()
    assert prof.regularized_size(0.75) == 2 and prof.regularized_size(3.5) == 1
    with pytest.raises(ValueError, match="alpha_min"):
        prof.regularized_size(0.5)
    with pytest.raises(ValueError, match="alpha_min"):
        prof.best_subset(2)
    alphas, sizes = prof.alpha_breakpoints()  # (the chord from size 2 to size 4 has slope 1/2 < alpha_min: left out)
    assert sizes.tolist() == [0, 1, 2] and alphas.tolist() == [5.0, 3.0]


# ---- the reference ------------------------------------------------------------------------------------------------------------
def test_reference_table_answers_brute_force_l1_and_saturates():
    X, y = make_regression(30, 7, n_informative=3, noise=5.0, random_state=4)
    n = 30
    cinf = float(np.max(np.abs(X.T @ y / n)))
    eta = 0.2 * cinf
    table = profile_table_l1(X, y, eta=eta, big_M=1000)
    assert table["n_supports"] == 2**7 and table["kkt"] <= 1e-10 * cinf and table["values"][0] == 0.0
    assert (np.diff(table["values"]) <= 1e-12 * abs(table["values"][-1])).all()  # the best of a size never rises with the size
    # saturation: the lasso on all columns leaves some coefficient at zero, and from its own size on the values tie
    lasso_nz = int(np.count_nonzero(table["coefs"][7]))
    assert 1 <= lasso_nz < 7
    tail = table["values"][lasso_nz:]
    assert np.max(np.abs(tail - tail[-1])) <= 1e-12 * abs(tail[-1]) and table["values"][lasso_nz - 1] > tail[-1]
    assert (table["gaps"][lasso_nz + 1: 7] <= 1e-12).all()  # a saturated size's support is not unique
    for rel in (1e-3, 5e-2, 0.5):
        alpha = rel * float(np.var(y))
        ref = brute_force_l1(X, y, alpha=alpha, eta=eta, big_M=1000)
        k = int(np.argmin(table["values"] + alpha * np.arange(8)))
        assert ref["active"].sum() == k and abs(table["values"][k] + alpha * k - ref["objective"]) <= 1e-12 * abs(ref["objective"])
        np.testing.assert_array_equal(table["actives"][k], ref["active"])
    # eta = 0 is the l0 profile's reference
    from _l0_profile_reference import profile_table

    a, b = profile_table_l1(X, y, K=3, eta=0.0, big_M=1000), profile_table(X, y, K=3, big_M=1000)
    np.testing.assert_array_equal(a["actives"], b["actives"])
    np.testing.assert_allclose(a["values"], b["values"], rtol=1e-12)
    # a hierarchy that admits no support of size 1 but the first group
    hier = [[]] + [[0]] * 6
    t = profile_table_l1(X, y, K=2, eta=eta, hierarchy=hier)
    assert t["n_supports"] == 1 + 1 + 6 and t["actives"][1].tolist() == [True] + [False] * 6 and t["actives"][2][0]


# ---- the host side, on the CPU ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_l1l0_profile_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l1l0_profile_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "l1l0_profile_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "l1l0_profile_host_test: ok" in run.stdout
