"""``l0_local_search`` without a GPU: the public surface (the C entry under ABI 24, ``ABI_SYMBOLS``, the binding, the
``Dataset`` method, the import path and the export lists that stay as they were), every refusal before a device is touched,
the numpy restatement of the rule (tests/_l0_local_reference.py) against ``_l0_reference.brute_force`` on a hard law, and the
host twin of the kernel in csrc/l0_host.hpp compiled with g++ and run on the CPU, plainly and under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/l0_local_host_test.cpp).

The law: n = 30, p = 14, AR(1) columns with correlation 0.9, 4 true columns, SNR 2 (``_l0_local_reference.hard_law``), seeds
0 - 23, alpha in {0.02, 0.05, 0.1} var y.  Measured with the committed restatement (profiles/l0_local.txt): the descent alone
reaches the exact optimum in 13 of the 72 cases, with swaps 32; swaps are strictly better in 39, never worse, and no result
is below the optimum.  ``SWAPS_REACH_OPTIMUM`` lists the cases where swaps are strictly better AND reach the optimum."""

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
from sklearn.datasets import make_regression

from _l0_local_reference import gram, hard_law, is_swap_inescapable, local_search, objective, polish
from _l0_reference import brute_force

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRIES = ("slm_solve_l0_local", "slm_solve_l0_local_descent")
RELS = (0.02, 0.05, 0.1)
# (seed, alpha / var y): derived with the committed restatement on the CPU; the swap counts are 1 - 3
SWAPS_REACH_OPTIMUM = [(1, 0.02), (1, 0.1), (3, 0.1), (5, 0.02), (6, 0.05), (7, 0.02), (7, 0.05), (7, 0.1), (10, 0.1), (11, 0.02), (12, 0.1),
                       (15, 0.02), (17, 0.02), (17, 0.1), (19, 0.02), (21, 0.02), (22, 0.1), (23, 0.05), (23, 0.1)]


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to open an engine fails the test: validation errors have to come first."""
    from sparselm_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were validated")

    monkeypatch.setattr(_engine, "get_engine", boom)


# ---- the public surface -------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_under_abi_24():
    from sparselm_amd import _engine

    assert _engine.ABI_VERSION == 24
    with open(os.path.join(ROOT, "include", "slm_engine.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "binding.cpp")) as fh:
        binding = fh.read()
    assert "#define SLM_ABI_VERSION 24" in header
    for name in ENTRIES:
        assert name in _engine.ABI_SYMBOLS and f"int {name}(" in header
        assert f"{name}(" in binding and f'm.def("{name[4:]}"' in binding
        decl = header[header.index(f"int {name}("):]
        decl = " ".join(decl[: decl.index(";")].split())
        for arg in ("slm_dataset* ds", "int32_t n_cells", "const double* alphas", "const double* etas", "double big_M", "int32_t n_starts",
                    "const double* starts", "double* beta_out", "double* objective_out", "int32_t* start_out", "slm_point_info* info"):
            assert arg in decl, (name, arg)
    assert hasattr(_engine.Dataset, "solve_l0_local")
    assert "#define SLM_L0_LOCAL_PMAX 1024" in header and _engine.L0_LOCAL_PMAX == 1024
    # the entries that were there are still there
    for name in ("slm_solve_l0", "slm_solve_l0_wide", "slm_solve_l0_l1", "slm_solve_l0_profile", "slm_solve_l0_profile_grid"):
        assert name in _engine.ABI_SYMBOLS and f"int {name}(" in header


def test_export_lists_are_unchanged():
    import sparselm_amd.miqp as miqp
    from sparselm_amd.model import _l0_cv, _l0_local, _l0_profile, _l1l0_profile

    assert miqp.__all__ == ["BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L1L0", "L2L0"]
    assert _l0_profile.__all__ == ["l0_profile", "L0Profile"]
    assert _l0_cv.__all__ == ["l0_profile_cv", "L0ProfileCV"]
    assert _l1l0_profile.__all__ == ["l1l0_profile", "L1L0Profile"]
    assert _l0_local.__all__ == ["l0_local_search", "L0LocalPath"]
    assert miqp.l0_local_search is _l0_local.l0_local_search and miqp.L0LocalPath is _l0_local.L0LocalPath
    assert miqp.L0LocalPath.proven_optimal_ is False


def test_signature():
    from sparselm_amd.miqp import l0_local_search

    params = inspect.signature(l0_local_search).parameters
    assert list(params) == ["X", "y", "alphas", "etas", "big_M", "fit_intercept", "sample_weight", "starts", "max_rounds", "solver_options"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in params.items() if k not in ("X", "y"))
    assert params["alphas"].default is inspect.Parameter.empty
    assert [params[k].default for k in list(params)[3:]] == [(0.0,), 100, False, None, None, 2, None]


# ---- refusals, all before a device ------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_device(no_device):
    from sparselm_amd.miqp import l0_local_search

    X, y = make_regression(25, 6, n_informative=3, random_state=0)
    for bad in (dict(alphas=[-1.0]), dict(alphas=[np.nan]), dict(alphas=[np.inf]), dict(alphas=[]), dict(alphas=[[0.1]]),
                dict(alphas=[0.1], etas=[-1.0]), dict(alphas=[0.1], etas=[np.inf]), dict(alphas=[0.1], etas=[]),
                dict(alphas=[0.1], big_M=-1), dict(alphas=[0.1], max_rounds=-1), dict(alphas=[0.1], max_rounds=1.5),
                dict(alphas=[0.1], solver_options={"max_nodes": 5}), dict(alphas=[0.1], solver_options={"swaps": 1}),
                dict(alphas=[0.1], solver_options=[("swaps", True)]), dict(alphas=[0.1], fit_intercept="yes"),
                dict(alphas=[0.1], sample_weight=np.ones(24)),
                dict(alphas=[0.1], starts=np.zeros((2, 5))), dict(alphas=[0.1, 0.2], starts=np.zeros((1, 1, 2, 6))),
                dict(alphas=[0.1], big_M=1.0, starts=np.full((1, 6), 1.5)), dict(alphas=[0.1], starts=np.full((1, 6), np.nan)),
                dict(alphas=np.full(5000, 0.1), etas=[0.0, 0.1]),                       # 10 000 cells x 4 starts of a round
                dict(alphas=np.full(5000, 0.1), starts=np.zeros((1, 6)), max_rounds=0)):  # 5 000 cells x 2 starts
        with pytest.raises(ValueError):
            l0_local_search(X, y, **bad)
    with pytest.raises(ValueError):
        l0_local_search(X, y[:-1], alphas=[0.1])
    with pytest.raises(TypeError):
        l0_local_search(X, y)
    with pytest.raises(TypeError):
        l0_local_search(X, y, [0.1])
    with pytest.raises(NotImplementedError, match="1024"):
        l0_local_search(np.zeros((3, 1025)), np.zeros(3), alphas=[0.1])


def test_the_engine_names_every_refusal_itself():
    """The C entry refuses each of these before it touches a device, each in its own words (the order and the codes are
    checked by tests/l0_local_host_test.cpp on ``l0_ls_check``; p = 1025 by the GPU tests on both routes)."""
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "engine_l0.hip")) as fh:
        unit = fh.read()
    body = unit[unit.index("int solve_l0_local_impl("):]
    body = body[: body.index("hipSetDevice")]
    for words in ("takes up to %d columns", "not built for groups", "not built for row-sharded datasets", "alphas[%lld] must be finite and >= 0",
                  "etas[%lld] must be finite and >= 0", "big_M must be >= 0", "n_cells must be >= 1", "n_starts must be >= 1",
                  "must be at most %d problems", "lies outside the box"):
        assert words in body, words


def test_the_estimators_keep_their_refusals(no_device):
    """The new search is beside the exact one, not in its place: beyond 128 columns the estimators still say so themselves
    (before the launch; the message itself is pinned by the GPU tests that were there)."""
    from sparselm_amd.miqp import L1L0

    X, y = make_regression(25, 6, n_informative=3, random_state=0)
    with pytest.raises(ValueError, match="no wide mode"):
        L1L0(solver_options={"wide": True}).fit(X, y)
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "engine_l0.hip")) as fh:
        assert "exact l0 search takes up to %d columns and %d groups" in fh.read()


# ---- the restatement against brute force ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_restatement_on_the_hard_law(seed):
    X, y = hard_law(seed)
    G, c, yy, _, _ = gram(X, y)
    for rel in RELS:
        alpha = rel * float(np.var(y))
        exact = brute_force(X, y, alpha=alpha, big_M=100.0)["objective"]
        tol = 1e-9 * max(abs(exact), alpha)
        runs = {}
        for swaps in (False, True):
            run = local_search(G, c, alpha, 100.0, yy, swaps=swaps)
            beta = polish(G, c, 100.0, run["beta"])
            F = objective(G, c, alpha, beta)
            assert run["status"] == 0 and abs(F - run["F"]) <= tol
            assert F >= exact - tol  # never below the optimum
            ok, why = is_swap_inescapable(G, c, alpha, 100.0, beta, 1e-8, swaps=swaps)
            assert ok, why
            runs[swaps] = F
        assert runs[True] <= runs[False] + tol  # swaps start from the descent's fixed point
        if (seed, rel) in SWAPS_REACH_OPTIMUM:
            assert runs[True] < runs[False] - tol and abs(runs[True] - exact) <= tol


def test_certificate_rejects_what_is_not_a_minimum():
    X, y = hard_law(12)
    G, c, yy, _, _ = gram(X, y)
    alpha = 0.1 * float(np.var(y))
    descent = polish(G, c, 100.0, local_search(G, c, alpha, 100.0, yy, swaps=False)["beta"])
    assert is_swap_inescapable(G, c, alpha, 100.0, descent, 1e-8, swaps=False)[0]
    assert not is_swap_inescapable(G, c, alpha, 100.0, descent, 1e-8, swaps=True)[0]  # (seed 12 is on the list: a swap helps)
    off = descent.copy()
    off[np.flatnonzero(off)[0]] *= 1.01
    assert not is_swap_inescapable(G, c, alpha, 100.0, off, 1e-8, swaps=False)[0]
    assert not is_swap_inescapable(G, c, alpha, 100.0, np.zeros(14), 1e-8, swaps=False)[0]  # some column's gain is above alpha


# ---- the host twin, on the CPU ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_l0_local_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l0_local_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "l0_local_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "l0_local_host_test: ok" in run.stdout
