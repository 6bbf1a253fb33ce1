"""``l0_local_group_search`` / ``l0_local_group_cv`` without a GPU: the public surface (the C entry under ABI 24, ``ABI_SYMBOLS``,
the binding, the ``Dataset`` method, the import path, the export lists that stay as they were), every refusal before a device
is touched, the numpy restatement of the rule (tests/_l0_local_groups_reference.py) against a brute force over all closed group
supports, its certificate, and the host twin of the kernel and the engine's check function (csrc/l0_host.hpp, "local groups")
compiled with g++ and run on the CPU as a child process, plainly and under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/l0_local_groups_host_test.cpp), on cases exported from the restatement.

The ground truth: 7 groups of 2 columns, n = 40, with a chain hierarchy (group g needs group g - 1) and without one, alpha in
{0.02, 0.05, 0.1} var y.  EASY law: AR(1) 0.1, SNR 20, the true groups first (closed under the chain) -- the restatement equals the optimum on every committed seed (checked
when the seeds were committed: all of 0 - 11).  HARD law: AR(1) 0.9, SNR 2 -- the restatement is never below the optimum, and the
share of cases on which it reaches it is printed, not asserted."""

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
from sklearn.datasets import make_regression

from _l0_local_groups_reference import (brute_force, close_hierarchy, closure, group_law, is_group_swap_inescapable, local_group_search,
                                        solve_group_cells)
from _l0_local_reference import gram, local_search

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRY = "slm_solve_l0_local_groups"
EASY_SEEDS = tuple(range(12))
HARD_SEEDS = tuple(range(12))
ALPHAS = (0.02, 0.05, 0.1)
CHAIN = [[]] + [[g - 1] for g in range(1, 7)]


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
    assert ENTRY in _engine.ABI_SYMBOLS and f"int {ENTRY}(" in header
    assert f"{ENTRY}(" in binding and f'm.def("{ENTRY[4:]}"' in binding
    decl = header[header.index(f"int {ENTRY}("):]
    decl = decl[: decl.index(");") + 1]
    # the issue's declaration: the same parameters in the same order
    names = ["ds", "count", "row_weights", "n_effs", "intercept", "n_cells", "alphas", "etas", "big_M", "need_ptr", "need_idx", "n_starts",
             "starts", "swaps", "beta_out", "intercept_out", "objective_out", "start_out", "group_support_out", "stat_out", "info"]
    at = [decl.index(f" {nm}") for nm in names]
    assert at == sorted(at)
    assert "const int32_t* need_ptr /* search groups + 1, or NULL */" in decl and "int32_t* group_support_out" in decl
    assert hasattr(_engine.Dataset, "solve_l0_local_groups")
    # the ctypes signature: the dataset, thirteen arguments, six outputs, the records
    assert len(_engine.load_library().slm_solve_l0_local_groups.argtypes) == 21
    # the entries that were there are still there, with the words the family's tests pin
    for name in ("slm_solve_l0_local", "slm_solve_l0_local_descent", "slm_solve_l0_local_folds", "slm_solve_l0_local_subsets"):
        assert name in _engine.ABI_SYMBOLS and f"int {name}(" in header
    assert "Not here: groups and a hierarchy, an l1 term" in header
    assert "Not here: groups, hierarchy, Tikhonov matrix, l1 term, constraints" in header
    assert header.count("slm_solve_l0_local_groups, below") >= 2


def test_export_lists_and_signatures():
    import sparselm_amd.miqp as miqp
    from sparselm_amd.model import _l0_local, _l0_local_groups, _l0_local_groups_cv

    assert _l0_local_groups.__all__ == ["l0_local_group_search", "L0LocalGroupPath"]
    assert _l0_local_groups_cv.__all__ == ["l0_local_group_cv", "L0LocalGroupCV"]
    for name in ("l0_local_group_search", "L0LocalGroupPath", "l0_local_group_cv", "L0LocalGroupCV"):
        assert hasattr(miqp, name) and name not in miqp.__all__
    assert miqp.__all__ == ["BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L1L0", "L2L0"]
    assert _l0_local.__all__ == ["l0_local_search", "L0LocalPath"]
    assert miqp.L0LocalGroupPath.proven_optimal_ is False and miqp.L0LocalGroupCV.proven_optimal_ is False
    params = inspect.signature(miqp.l0_local_group_search).parameters
    assert list(params) == ["X", "y", "alphas", "groups", "hierarchy", "etas", "big_M", "fit_intercept", "sample_weight", "starts", "max_rounds",
                            "solver_options"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in params.items() if k not in ("X", "y"))
    assert params["alphas"].default is inspect.Parameter.empty
    assert [params[k].default for k in list(params)[3:]] == [None, None, (0.0,), 100, False, None, None, 2, None]
    params = inspect.signature(miqp.l0_local_group_cv).parameters
    assert list(params) == ["X", "y", "alphas", "groups", "hierarchy", "etas", "cv", "big_M", "fit_intercept", "sample_weight", "starts",
                            "max_rounds", "scoring", "solver_options"]
    for doc in (_l0_local_groups.__doc__, _l0_local_groups_cv.__doc__, miqp.l0_local_group_search.__doc__):
        for words in ("cardinality form", "l1 term", "Tikhonov matrix", "constraints", "seeding the exact search"):
            assert words in doc, words
    assert "NOTHING IS PROVEN" in _l0_local_groups.__doc__ and "can miss" in miqp.l0_local_group_search.__doc__


def test_the_family_points_at_the_grouped_search_and_keeps_its_refusals():
    from sparselm_amd.model import _l0_local, _l0_local_cv, _l0_local_subsets

    assert "Not built: groups and a hierarchy" in _l0_local.__doc__ and "l0_local_group_search" in _l0_local.__doc__
    assert "l0_local_group_cv" in _l0_local_cv.__doc__ and "l0_local_group_search" in _l0_local_subsets.__doc__
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "engine_l0.hip")) as fh:
        unit = fh.read()
    assert f'extern "C" int {ENTRY}(' in unit
    body = unit[unit.index("int solve_l0_local_folds_impl("):]
    assert body.index("l0_lg_check(") < body.index("hipSetDevice")  # the grouped kind's refusals come before a device too
    body = body[: body.index("hipSetDevice")]
    for words in ("not built for groups", "the caller must order the columns", "need_ptr must start at 0 and never fall",
                  "need_idx[%lld] must name one of the %d search groups", "not built for row-sharded datasets"):
        assert words in body, words
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "l0_local_group_kernels.hpp")) as fh:
        kernel = fh.read()
    assert "l0_local_group_kernel" in kernel and "asm" not in kernel and "atomicAdd(&w.held" in kernel  # (integers only)
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "l0_local_kernels.hpp")) as fh:
        assert "template <bool CARD>\nstatic __global__" in fh.read()  # no third flag on the family's kernel
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        assert "**Local search with groups**" in fh.read()


# ---- refusals, all before a device ------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_device(no_device):
    from sparselm_amd.miqp import l0_local_group_cv, l0_local_group_search

    X, y = make_regression(25, 6, n_informative=3, random_state=0)
    groups = [0, 0, 1, 1, 2, 2]
    for bad in (dict(alphas=[-1.0]), dict(alphas=[np.nan]), dict(alphas=[]), dict(alphas=[[0.1]]), dict(alphas=[0.1], etas=[-1.0]),
                dict(alphas=[0.1], big_M=-1), dict(alphas=[0.1], max_rounds=-1), dict(alphas=[0.1], solver_options={"max_nodes": 5}),
                dict(alphas=[0.1], solver_options={"swaps": 1}), dict(alphas=[0.1], fit_intercept="yes"),
                dict(alphas=[0.1], sample_weight=np.ones(24)), dict(alphas=[0.1], starts=np.zeros((2, 5))),
                dict(alphas=[0.1], big_M=1.0, starts=np.full((1, 6), 1.5)),
                dict(alphas=[0.1], groups=[0, 0, 1, 1, 2]),                                # one label short
                dict(alphas=[0.1], groups=groups, hierarchy=[[], [0]]),                    # one entry short
                dict(alphas=[0.1], groups=groups, hierarchy=[[], [0], [7]]),               # an unknown label
                dict(alphas=[0.1], hierarchy=[[]] * 5),                                    # singleton groups: six entries
                dict(alphas=np.full(5000, 0.1), groups=groups)):                           # 5 000 cells x 2 starts of a round
        with pytest.raises(ValueError):
            l0_local_group_search(X, y, **bad)
    for bad in (dict(alphas=[0.1], scoring="r2"), dict(alphas=[0.1], cv=16), dict(alphas=[0.1], cv=1),
                dict(alphas=[0.1], groups=groups, hierarchy=[[], [0], [7]]), dict(alphas=np.full(1400, 0.1), max_rounds=0)):
        with pytest.raises(ValueError):
            l0_local_group_cv(X, y, **bad)
    with pytest.raises(TypeError):
        l0_local_group_search(X, y)
    with pytest.raises(TypeError):
        l0_local_group_search(X, y, [0.1])
    for call in (l0_local_group_search, l0_local_group_cv):
        with pytest.raises(NotImplementedError, match="1024"):
            call(np.zeros((6, 1025)), np.zeros(6), alphas=[0.1])


def test_the_plan_orders_the_columns_by_group():
    """Shuffled labels: the permutation makes every group contiguous, the need lists are in sorted-label order, and coefficients and
    group supports map back."""
    from sparselm_amd.model._l0_local_groups import _GroupPlan

    X, y = make_regression(20, 6, n_informative=3, random_state=1)
    labels = np.array([30, 10, 20, 10, 30, 20])
    plan = _GroupPlan(X, y, [0.1], labels, [[], [10], [20, 10]], (0.0,), 100, False, None, np.arange(6.0)[None, :], 2, None)
    assert list(plan.gidx) == [0, 0, 1, 1, 2, 2] and list(plan.gstart) == [0, 2, 4, 6] and plan.need == [[], [0], [0, 1]]
    assert np.array_equal(plan.X, X[:, plan.perm]) and sorted(plan.perm) == list(range(6))
    assert np.array_equal(labels[plan.perm], [10, 10, 20, 20, 30, 30])
    assert np.array_equal(plan.first[0, 0, 1], np.arange(6.0)[plan.perm]) and not plan.first[0, 0, 0].any()
    coefs = np.zeros((1, 1, 6))
    coefs[0, 0, 2] = 1.0  # a column of label 20 in the permuted order
    assert np.array_equal(plan.group_supports(coefs)[0, 0], [True, True, False])  # 20 needs 10
    back = plan.unpermute(coefs)
    assert labels[np.flatnonzero(back[0, 0])[0]] == 20
    single = _GroupPlan(X, y, [0.1], None, None, (0.0,), 100, False, None, None, 2, None)
    assert single.gidx is None and single.n_groups == 6 and list(single.gstart) == list(range(7)) and single.X is not None


# ---- the restatement against brute force ----------------------------------------------------------------------------------------------
def _truth_cases(seeds, easy):
    for seed in seeds:
        X, y, gstart = group_law(seed, rho=0.1, snr=20.0, spread=False) if easy else group_law(seed)
        G, c, yy, _, _ = gram(X, y)
        for need in (None, CHAIN):
            closed = close_hierarchy(7, need)
            for a in ALPHAS:
                yield seed, need is not None, G, c, yy, gstart, closed, a * float(np.var(y))


def _against_truth(seeds, easy):
    hits = total = 0
    for seed, chained, G, c, yy, gstart, closed, alpha in _truth_cases(seeds, easy):
        run = local_group_search(G, c, gstart, closed, alpha, 100.0, yy)
        best, support = brute_force(G, c, alpha, gstart, closed)
        scale = max(abs(best), alpha)
        assert run["status"] == 0 and run["F"] >= best - 1e-9 * scale, (seed, chained, alpha)   # never below the optimum
        assert np.array_equal(run["closed"], closure(run["beta"], gstart, closed))              # the tables say what beta says
        ok, why = is_group_swap_inescapable(G, c, alpha, 100.0, run["beta"], gstart, closed, 1e-8)
        assert ok, (seed, chained, alpha, why)
        hit = run["F"] <= best + 1e-9 * scale
        if easy:
            assert hit and np.array_equal(run["closed"], support), (seed, chained, alpha, run["F"], best)
        hits, total = hits + hit, total + 1
    return hits, total


def test_the_restatement_equals_the_optimum_on_the_easy_law():
    hits, total = _against_truth(EASY_SEEDS, True)
    assert hits == total == len(EASY_SEEDS) * 2 * len(ALPHAS)


def test_the_restatement_is_never_below_the_optimum_on_the_hard_law():
    hits, total = _against_truth(HARD_SEEDS, False)
    print(f"hard law (7 groups of 2, AR(1) 0.9, SNR 2), with and without a chain: the restatement reaches the optimum in {hits} of {total} cases")
    assert total == len(HARD_SEEDS) * 2 * len(ALPHAS)


def test_singleton_groups_without_a_hierarchy_are_the_local_search():
    """The same supports, swap counts and sweeps as the family's restatement, on the hard law of its tests."""
    from _l0_local_reference import hard_law

    for seed in range(8):
        X, y = hard_law(seed)
        G, c, yy, _, _ = gram(X, y)
        for a in ALPHAS:
            alpha = a * float(np.var(y))
            old = local_search(G, c, alpha, 100.0, yy)
            new = local_group_search(G, c, np.arange(15), close_hierarchy(14, None), alpha, 100.0, yy)
            if min(old["margin"], new["margin"]) < 1e-6:
                continue
            assert np.array_equal(old["beta"] != 0.0, new["beta"] != 0.0), (seed, a)
            assert (old["swaps"], old["sweeps"]) == (new["swaps"], new["sweeps"]), (seed, a)
            assert abs(old["F"] - new["F"]) <= 1e-10 * max(abs(old["F"]), alpha)


def test_the_certificate_rejects_a_non_minimum():
    X, y, gstart = group_law(0, rho=0.1, snr=20.0, spread=False)
    G, c, yy, _, _ = gram(X, y)
    closed = close_hierarchy(7, CHAIN)
    alpha = 0.05 * float(np.var(y))
    run = local_group_search(G, c, gstart, closed, alpha, 100.0, yy)
    assert is_group_swap_inescapable(G, c, alpha, 100.0, run["beta"], gstart, closed, 1e-8)[0]
    active = np.flatnonzero(run["closed"])
    assert active.size >= 2
    moved = run["beta"].copy()
    moved[gstart[active[0]]] *= 1.01                                 # a coefficient off its one-coordinate value
    assert not is_group_swap_inescapable(G, c, alpha, 100.0, moved, gstart, closed, 1e-8)[0]
    assert not is_group_swap_inescapable(G, c, alpha, 100.0, np.zeros(14), gstart, closed, 1e-8)[0]   # zero: a screened group pays
    dropped = run["beta"].copy()
    deepest = np.flatnonzero([np.any(run["beta"][gstart[g]:gstart[g + 1]] != 0.0) for g in range(7)])[-1]
    dropped[gstart[deepest]:gstart[deepest + 1]] = 0.0               # a paying group taken out (the others left where they were)
    assert not is_group_swap_inescapable(G, c, alpha, 100.0, dropped, gstart, closed, 1e-8)[0]
    outside = run["beta"].copy()
    outside[0] = 101.0
    assert not is_group_swap_inescapable(G, c, alpha, 100.0, outside, gstart, closed, 1e-8)[0]


# ---- the host twin and the check function, on the CPU --------------------------------------------------------------------------------
def _export(path):
    """Cases for tests/l0_local_groups_host_test.cpp, from the restatement: only those it decided with a margin >= 1e-6."""
    rng = np.random.default_rng(5)
    cases = []

    def add(G, c, yy, gstart, need, alpha, eta, big_M, swaps, start):
        ng = len(gstart) - 1
        H = G + 2.0 * eta * np.eye(len(c))
        run = local_group_search(H, c, gstart, close_hierarchy(ng, need), alpha, big_M, yy, start, swaps)
        if run["margin"] < 1e-6 or run["status"]:
            return
        lists = need if need is not None else [[] for _ in range(ng)]
        ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(int)
        words = [len(c), ng, repr(float(alpha)), repr(float(eta)), repr(float(big_M)), repr(float(yy)), int(swaps), int(start is not None)]
        words += list(gstart) + list(ptr) + [h for v in lists for h in v]
        words += [repr(float(v)) for v in G.ravel()] + [repr(float(v)) for v in c]
        words += [repr(float(v)) for v in (start if start is not None else [])]
        words += [run["sweeps"], run["swaps"], run["status"], int(run["closed"].sum()), run["nnz"], run["trials"], repr(run["F"])]
        words += [int(v != 0.0) for v in run["beta"]] + [int(v) for v in run["closed"]]
        cases.append(" ".join(str(w) for w in words))

    for seed in range(6):
        X, y, gstart = group_law(seed)
        G, c, yy, _, _ = gram(X, y)
        var = float(np.var(y))
        wrong = np.zeros(14)
        wrong[[0, 1, 12]] = 0.5  # a start whose support is not closed under the chain
        for need in (None, CHAIN, [[1], [0], [], [2], [3], [3], [4, 5]]):   # none; a chain; a two-cycle, a chain and a diamond
            for a in ALPHAS:
                add(G, c, yy, gstart, need, a * var, 0.0, 100.0, True, None)
            add(G, c, yy, gstart, need, 0.05 * var, 0.01, 100.0, True, wrong)
            add(G, c, yy, gstart, need, 0.05 * var, 0.0, 100.0, False, None)
            add(G, c, yy, gstart, need, 0.02 * var, 0.0, 0.6, True, None)   # the box binds
    swapped = 0
    for seed, k, need in ((2, 2, None), (34, 3, [[], [0], [0], [1, 2], [], [4], [1]])):   # seeds on which the scan accepts a swap
        X, y, gstart = group_law(seed, k=k)
        G, c, yy, _, _ = gram(X, y)
        for a in ALPHAS:
            add(G, c, yy, gstart, need, a * float(np.var(y)), 0.0, 100.0, True, None)
            swapped += int(cases[-1].split()[-(14 + 7 + 6)]) > 0
    assert swapped >= 2
    # uneven groups, a group of one column last, a dead column, singleton groups
    X = rng.standard_normal((30, 9))
    X[:, 4] = 0.0
    y = X[:, 0] - X[:, 1] + X[:, 8] + 0.3 * rng.standard_normal(30)
    G, c, yy, _, _ = gram(X, y)
    for gstart, need in (([0, 3, 4, 8, 9], None), ([0, 3, 4, 8, 9], [[], [0], [], [2]]), (list(range(10)), None), ([0, 9], None)):
        for a in (0.01, 0.1):
            add(G, c, yy, np.array(gstart), need, a * float(np.var(y)), 0.0, 100.0, True, None)
    assert len(cases) >= 80, len(cases)
    with open(path, "w") as fh:
        fh.write(f"{len(cases)}\n" + "\n".join(cases) + "\n")
    return len(cases)


@pytest.mark.parametrize("sanitize", [False, True])
def test_l0_local_groups_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l0_local_groups_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "l0_local_groups_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    count = _export(tmp_path / "cases.txt")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"l0_local_groups_host_test: ok ({count} cases)" in run.stdout


def test_the_restatement_runs_cells_and_starts():
    """``solve_group_cells``, what the GPU tests compare against: the winner by (F, lowest start), polished on cl(S)."""
    X, y, gstart = group_law(1, rho=0.1, snr=20.0, spread=False)
    var = float(np.var(y))
    starts = np.zeros((2, 2, 14))
    starts[:, 1, 12:] = 0.5
    cells = solve_group_cells(X, y, gstart, CHAIN, [0.02 * var, 0.05 * var], [0.0, 0.0], starts=starts)
    for cell, alpha in zip(cells, [0.02 * var, 0.05 * var]):
        assert cell["F"].shape == (2,) and cell["start"] == int(np.argmin(cell["F"]))
        assert cell["objective"] <= cell["F"][cell["start"]] + 1e-12 * var   # the polish does not raise it
        best, _ = brute_force(cell["H"], cell["c"], alpha, gstart, close_hierarchy(7, CHAIN))
        assert cell["objective"] >= best - 1e-9 * max(abs(best), alpha)
