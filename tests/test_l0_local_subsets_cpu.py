"""Local subsets (``l0_local_subsets`` / ``l0_local_subsets_cv``, ``slm_solve_l0_local_subsets``) without a GPU: the public
surface (the C entry under ABI 24, ``ABI_SYMBOLS``, the binding, the ``Dataset`` method, the import path, the export lists),
every refusal before a device is touched, the "not built" lists, the numpy restatement of the rule
(tests/_l0_local_subsets_reference.py) against enumeration of every support on a hard law, the selection rules of
``L0LocalSubsetsCV.search`` on a hand-made table, and the host twin of the kernel's rule in csrc/l0_host.hpp compiled with g++
and run on the CPU as a child process, plainly and under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/l0_local_subsets_host_test.cpp).

The law: n = 30, p = 14, AR(1) columns with correlation 0.9, 4 true columns, SNR 2 (``_l0_local_reference.hard_law``), seeds
0 - 23, k = 1 .. 6: 144 cases.  Measured with the committed restatement: greedy forward selection alone (``swaps=False``) is
at the optimum in 74 of the 144, the full rule from the zero start in 92, and the better of that and the chain from the kept
result of k - 1 in 104; no result is below the optimum and the swaps are never worse than greedy.  The smallest relative
margin of any shrink, grow or swap decision over all those runs is 2.6e-4 (descent steps take no decision that is counted).
``SWAPS_REACH_OPTIMUM`` lists the (seed, k) where the swaps from zero are strictly better than greedy AND at the optimum."""

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
from sklearn.datasets import make_regression
from sklearn.model_selection import KFold, ParameterGrid

from _l0_local_reference import gram, hard_law, polish
from _l0_local_subsets_reference import best_subsets, is_subset_inescapable, local_subsets, quadratic

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRY = "slm_solve_l0_local_subsets"
SIZES = range(1, 7)
GREEDY_HITS, ZERO_START_HITS, CHAIN_HITS, CASES = 74, 92, 104, 144
SWAPS_REACH_OPTIMUM = [(4, 2), (6, 3), (7, 2), (10, 3), (11, 4), (11, 5), (14, 3), (14, 4), (15, 2), (16, 2), (16, 3), (17, 4), (17, 6), (19, 5),
                       (20, 2), (20, 4), (20, 5), (22, 3)]


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
    decl = " ".join(decl[: decl.index(";")].split())
    args = ("slm_dataset* ds", "int32_t count", "const double* const* row_weights", "const int64_t* n_effs", "int32_t intercept",
            "int32_t n_cells", "const int32_t* sizes", "const double* etas", "double big_M", "int32_t n_starts", "const double* starts",
            "int32_t swaps", "double* beta_out", "double* intercept_out", "double* objective_out", "int32_t* start_out", "int32_t* stat_out",
            "slm_point_info* info")
    at = [decl.index(arg) for arg in args]
    assert at == sorted(at)  # every argument, in this order
    comment = header[: header.index(f"int {ENTRY}(")]
    comment = comment[comment.rindex("/*"):]
    for words in ("Shrink", "Descent on the support", "Grow", "Swap scan", "Refusals", "SIX ints",
                  "Not here: groups, hierarchy, Tikhonov matrix, l1 term, constraints"):
        assert words in comment, words
    assert hasattr(_engine.Dataset, "solve_l0_local_subsets")
    # the ctypes signature: the dataset, eleven arguments, five outputs, the records
    assert len(_engine.load_library().slm_solve_l0_local_subsets.argtypes) == 18
    # the entries that were there are still there, with the arguments they had
    for name in ("slm_solve_l0_local", "slm_solve_l0_local_descent", "slm_solve_l0_local_folds", "slm_solve_l0_profile"):
        assert name in _engine.ABI_SYMBOLS and f"int {name}(" in header
    assert len(_engine.load_library().slm_solve_l0_local_folds.argtypes) == 18


def test_export_lists():
    import sparselm_amd.miqp as miqp
    from sparselm_amd.model import _l0_local, _l0_local_cv, _l0_local_subsets, _l0_local_subsets_cv

    assert _l0_local_subsets.__all__ == ["l0_local_subsets", "L0LocalSubsets"]
    assert _l0_local_subsets_cv.__all__ == ["l0_local_subsets_cv", "L0LocalSubsetsCV"]
    for name, mod in (("l0_local_subsets", _l0_local_subsets), ("L0LocalSubsets", _l0_local_subsets),
                      ("l0_local_subsets_cv", _l0_local_subsets_cv), ("L0LocalSubsetsCV", _l0_local_subsets_cv)):
        assert getattr(miqp, name) is getattr(mod, name) and name not in miqp.__all__
    assert miqp.__all__ == ["BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L1L0", "L2L0"]
    assert _l0_local.__all__ == ["l0_local_search", "L0LocalPath"] and _l0_local_cv.__all__ == ["l0_local_cv", "L0LocalCV"]
    assert miqp.L0LocalSubsets.proven_optimal_ is False and miqp.L0LocalSubsetsCV.proven_optimal_ is False


def test_signatures():
    from sparselm_amd.miqp import l0_local_subsets, l0_local_subsets_cv

    params = inspect.signature(l0_local_subsets).parameters
    assert list(params) == ["X", "y", "sizes", "etas", "big_M", "fit_intercept", "sample_weight", "starts", "max_rounds", "solver_options"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in params.items() if k not in ("X", "y"))
    assert params["sizes"].default is inspect.Parameter.empty
    assert [params[k].default for k in list(params)[3:]] == [(0.0,), 100, False, None, None, 2, None]
    params = inspect.signature(l0_local_subsets_cv).parameters
    assert list(params) == ["X", "y", "sizes", "etas", "cv", "big_M", "fit_intercept", "sample_weight", "starts", "max_rounds", "scoring",
                            "solver_options"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in params.items() if k not in ("X", "y"))
    assert [params[k].default for k in list(params)[3:]] == [(0.0,), 5, 100, False, None, None, 2, "neg_root_mean_squared_error", None]


def test_the_result_carries_every_table():
    from sparselm_amd.miqp import L0LocalSubsets

    z = np.zeros((2, 1))
    coefs = np.array([[[0.0, 2.0, 0.0]], [[1.0, 2.0, 0.0]]])
    res = L0LocalSubsets([1, 2], [0.0], coefs, [[0.5], [0.25]], z, z, 1, z[None], z, z, z, z, np.ones((2, 1), bool))
    for name in ("sizes_", "etas_", "coefs_", "intercepts_", "supports_", "objectives_", "losses_", "rounds_", "round_objectives_", "swaps_",
                 "sweeps_", "grows_", "drops_", "converged_"):
        assert hasattr(res, name), name
    assert res.sizes_.dtype.kind == "i" and res.supports_.sum() == 3 and res.proven_optimal_ is False
    np.testing.assert_array_equal(res.predict(np.eye(3), 1), [1.25, 2.25, 0.25])
    with pytest.raises(ValueError):
        res.predict(np.eye(4), 0)


def test_the_docstrings_say_what_the_issue_asks():
    from sparselm_amd.model import _l0_local_subsets

    doc = " ".join(_l0_local_subsets.__doc__.split())
    assert 'RidgedBestSubsetSelection.solver_info_["objective"]' in doc and "_miqp.py" in doc
    assert "non-increasing in k" in doc and "NOTHING IS PROVEN" in doc
    assert "non-increasing in k" in " ".join(_l0_local_subsets.l0_local_subsets.__doc__.split())


def test_the_not_built_lists_no_longer_name_the_cardinality_form():
    from sparselm_amd.model import _l0_local

    with open(os.path.join(ROOT, "include", "slm_engine.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        design = fh.read()
    assert "a bound on the cardinality (best-subset form)" not in _l0_local.__doc__
    comment = header[header.index("The l0 LOCAL SEARCH"): header.index("int slm_solve_l0_local(")]
    assert "Not here: groups and a hierarchy, an l1 term" in comment and "slm_solve_l0_local_subsets" in comment
    for title in ("**Local search**", "**Local search over folds**"):
        para = design[design.index(title):]
        para = para[: para.index("\n\n**")] if "\n\n**" in para else para
        assert "a bound on the cardinality (the best-subset form)" not in para, title
    assert "**Local subsets**" in design


# ---- refusals, all before a device ------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_device(no_device):
    from sparselm_amd.miqp import l0_local_subsets, l0_local_subsets_cv

    X, y = make_regression(25, 6, n_informative=3, random_state=0)
    common = (dict(sizes=[0]), dict(sizes=[-2]), dict(sizes=[1.5]), dict(sizes=[np.nan]), dict(sizes=[]), dict(sizes=[[2]]), dict(sizes=[True]),
              dict(sizes=[2], etas=[-1.0]), dict(sizes=[2], etas=[np.inf]), dict(sizes=[2], etas=[]),
              dict(sizes=[2], big_M=-1), dict(sizes=[2], max_rounds=-1), dict(sizes=[2], max_rounds=1.5),
              dict(sizes=[2], solver_options={"max_nodes": 5}), dict(sizes=[2], solver_options={"swaps": 1}),
              dict(sizes=[2], solver_options=[("swaps", True)]), dict(sizes=[2], fit_intercept="yes"),
              dict(sizes=[2], sample_weight=np.ones(24)),
              dict(sizes=[2], starts=np.zeros((2, 5))), dict(sizes=[2, 3], starts=np.zeros((1, 1, 2, 6))),
              dict(sizes=[2], big_M=1.0, starts=np.full((1, 6), 1.5)), dict(sizes=[2], starts=np.full((1, 6), np.nan)))
    for fn in (l0_local_subsets, l0_local_subsets_cv):
        for bad in common:
            with pytest.raises(ValueError):
                fn(X, y, **bad)
        with pytest.raises(ValueError):
            fn(X, y[:-1], sizes=[2])
        with pytest.raises(TypeError):
            fn(X, y)
        with pytest.raises(TypeError):
            fn(X, y, [2])
    for bad in (dict(sizes=np.full(5000, 2), etas=[0.0, 0.1]),                       # 10 000 cells x 4 starts of a round
                dict(sizes=np.full(5000, 2), starts=np.zeros((1, 6)), max_rounds=0)):  # 5 000 cells x 2 starts
        with pytest.raises(ValueError):
            l0_local_subsets(X, y, **bad)
    for bad in (dict(sizes=[2], scoring="r2"), dict(sizes=[2], cv=16), dict(sizes=[2], cv=KFold(20)), dict(sizes=[2], cv=1),
                dict(sizes=np.full(700, 2), etas=[0.0, 0.1], cv=2),                    # 3 row sets x 1 400 cells x 4 starts of a round
                dict(sizes=np.full(1500, 2), starts=np.zeros((1, 6)), max_rounds=0),   # 6 row sets x 1 500 cells x 2 starts
                dict(sizes=np.full(1400, 2), max_rounds=0)):                           # 6 row sets x 1 400 cells
        with pytest.raises(ValueError):
            l0_local_subsets_cv(X, y, **bad)
    with pytest.raises(ValueError):  # the first fold trains on rows 5 .. 24, which hold no weight
        l0_local_subsets_cv(X, y, sizes=[2], sample_weight=np.r_[np.ones(5), np.zeros(20)], cv=KFold(5))
    with pytest.raises(NotImplementedError, match="1024"):
        l0_local_subsets(np.zeros((3, 1025)), np.zeros(3), sizes=[2])
    with pytest.raises(NotImplementedError, match="1024"):
        l0_local_subsets_cv(np.zeros((6, 1025)), np.zeros(6), sizes=[2], cv=2)


def test_the_engine_names_every_refusal_itself():
    """The C entry refuses each of these before it touches a device, each in its own words (the order and the codes are checked
    by tests/l0_local_subsets_host_test.cpp on ``l0_lc_check``; the messages by the GPU tests on both routes)."""
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "engine_l0.hip")) as fh:
        unit = fh.read()
    assert 'extern "C" int slm_solve_l0_local_subsets(' in unit
    body = unit[unit.index("int solve_l0_local_folds_impl("):]
    assert body.index("l0_lc_check(") < body.index("hipSetDevice")
    body = body[: body.index("hipSetDevice")]
    for words in ("sizes[%lld] must be >= 1", "etas[%lld] must be finite and >= 0", "takes up to %d columns", "not built for groups",
                  "not built for row-sharded datasets", "big_M must be >= 0", "n_cells must be >= 1", "n_starts must be >= 1",
                  "count * n_cells * n_starts must be at most %d problems", "lies outside the box", "count must be 1 .. %d",
                  "row_weights[%d][%lld] must be finite and >= 0", "the last column must be alone in the last group"):
        assert words in body, words


# ---- the restatement against enumeration ------------------------------------------------------------------------------------------
def _hard_law_runs(seed):
    """Per k: (optimum, greedy, the rule from zero, the better of that and the chain from the kept result of k - 1)."""
    X, y = hard_law(seed)
    G, c, yy, _, _ = gram(X, y)
    rows, prev, margin = [], None, np.inf
    optimum = best_subsets(G, c, max(SIZES))
    for k in SIZES:
        exact = float(optimum[k])
        runs = [local_subsets(G, c, k, 100.0, yy, swaps=False), local_subsets(G, c, k, 100.0, yy, swaps=True)]
        if prev is not None:
            runs.append(local_subsets(G, c, k, 100.0, yy, start=prev, swaps=True))
        Q = []
        for run, swaps in zip(runs, (False, True, True)):
            beta = polish(G, c, 100.0, run["beta"])
            Q.append(quadratic(G, c, beta))
            assert run["status"] == 0 and run["nnz"] == k and abs(Q[-1] - run["Q"]) <= 1e-9 * abs(exact)
            ok, why = is_subset_inescapable(G, c, k, 100.0, yy, beta, 1e-8, swaps=swaps)
            assert ok, why
            margin = min(margin, run["margin"])
        best = 1 + int(np.argmin([r["Q"] for r in runs[1:]]))
        prev = polish(G, c, 100.0, runs[best]["beta"])
        rows.append((k, exact, Q[0], Q[1], Q[best]))
    return rows, margin


@pytest.fixture(scope="module")
def hard_law_table():
    return {seed: _hard_law_runs(seed) for seed in range(24)}


@pytest.mark.parametrize("seed", range(24))
def test_restatement_on_the_hard_law(hard_law_table, seed):
    rows, _ = hard_law_table[seed]
    last = 0.0
    for k, exact, greedy, zero, chain in rows:
        tol = 1e-9 * abs(exact)
        assert min(greedy, zero, chain) >= exact - tol  # never below the optimum
        assert zero <= greedy + tol                      # swaps never worse than greedy: they start where it stops
        assert chain <= zero + tol and chain <= last + tol  # the chain keeps the better result, and Q does not rise with k
        last = chain
        if (seed, k) in SWAPS_REACH_OPTIMUM:
            assert zero < greedy - tol and abs(zero - exact) <= tol


def test_hit_counts_on_the_hard_law(hard_law_table):
    hits = np.zeros(3, dtype=int)
    strict, margin = [], np.inf
    for seed, (rows, m) in hard_law_table.items():
        margin = min(margin, m)
        for k, exact, greedy, zero, chain in rows:
            tol = 1e-9 * abs(exact)
            hits += [abs(greedy - exact) <= tol, abs(zero - exact) <= tol, abs(chain - exact) <= tol]
            if zero < greedy - tol and abs(zero - exact) <= tol:
                strict.append((seed, k))
    print(f"hits of {CASES}: greedy {hits[0]}, zero start {hits[1]}, chain {hits[2]}; smallest margin {margin:.3g}")
    assert len(hard_law_table) * len(SIZES) == CASES
    assert list(hits) == [GREEDY_HITS, ZERO_START_HITS, CHAIN_HITS]
    assert strict == SWAPS_REACH_OPTIMUM
    assert 2.6e-4 <= margin < 2.7e-4


def test_certificate_rejects_what_is_not_a_minimum():
    X, y = hard_law(4)
    G, c, yy, _, _ = gram(X, y)
    greedy = polish(G, c, 100.0, local_subsets(G, c, 2, 100.0, yy, swaps=False)["beta"])
    assert is_subset_inescapable(G, c, 2, 100.0, yy, greedy, 1e-8, swaps=False)[0]
    assert not is_subset_inescapable(G, c, 2, 100.0, yy, greedy, 1e-8, swaps=True)[0]  # ((4, 2) is on the list: a swap helps)
    assert not is_subset_inescapable(G, c, 1, 100.0, yy, greedy, 1e-8, swaps=False)[0]  # two columns are more than one
    assert not is_subset_inescapable(G, c, 3, 100.0, yy, greedy, 1e-8, swaps=False)[0]  # a third column could still enter
    off = greedy.copy()
    off[np.flatnonzero(off)[0]] *= 1.01
    assert not is_subset_inescapable(G, c, 2, 100.0, yy, off, 1e-8, swaps=False)[0]
    assert not is_subset_inescapable(G, c, 2, 100.0, yy, np.zeros(14), 1e-8, swaps=False)[0]


def test_shrink_grow_and_the_counts_of_the_restatement():
    X, y = hard_law(3)
    G, c, yy, _, _ = gram(X, y)
    full = local_subsets(G, c, 14, 100.0, yy)  # every column enters
    assert full["nnz"] == 14 and full["grows"] == 14 and full["drops"] == 0 and full["swaps"] == 0
    down = local_subsets(G, c, 3, 100.0, yy, start=full["beta"])
    assert down["nnz"] == 3 and down["drops"] == 11 and down["grows"] == 0
    up = local_subsets(G, c, 5, 100.0, yy, start=down["beta"])
    assert up["nnz"] == 5 and up["grows"] == 2 and up["drops"] == 0
    boxed = local_subsets(G, c, 4, 0.3, yy)
    assert boxed["nnz"] == 4 and np.abs(boxed["beta"]).max() == 0.3
    assert is_subset_inescapable(G, c, 4, 0.3, yy, boxed["beta"], 1e-8)[0]


# ---- the premises of the GPU comparisons, recomputed ----------------------------------------------------------------------------------
def test_premises_of_the_gpu_comparisons():
    """Every case of tests/_l0_local_subsets_cases.py: the restatement converges with every decision margin >= 1e-6 (the GPU
    test skips a case that does not; at most a tenth may, none does), a winner whose lead over another start is below 1e-6 shares
    its support with it, and each case reaches the path it is there for."""
    from _l0_local_subsets_cases import NAMES, case, reference

    failing = []
    for name in NAMES:
        c, ref = case(name), reference(name)
        assert len(ref) == len(c["weights"]) and all(len(cells) == len(c["sizes"]) for cells in ref)
        if not all(cell["status"] == 0 and cell["margin"] >= 1e-6 for cells in ref for cell in cells):
            failing.append(name)
        for cells in ref:
            for e, cell in enumerate(cells):
                assert np.count_nonzero(cell["beta"]) <= c["sizes"][e]
                if cell["lead"] < 1e-6:  # tied starts: one support, so that only the index is open
                    tied = np.flatnonzero(np.abs(cell["Q"] - cell["Q"][cell["start"]]) <= 1e-6 * abs(cell["Q"][cell["start"]]))
                    G = cell["H"]
                    for s in tied:
                        run = local_subsets(G, cell["c"], int(c["sizes"][e]), c["big_M"], cell["yy"], c["starts"][e][s], c["swaps"])
                        np.testing.assert_array_equal(run["beta"] != 0.0, cell["beta"] != 0.0)
    assert len(failing) <= len(NAMES) // 10, failing
    assert failing == []
    stats = {name: np.array([[cell["stats"] for cell in cells] for cells in reference(name)]) for name in NAMES}  # R x E x S x 6
    assert np.all(stats["dead_column"][..., 3] == 11) and max(case("dead_column")["sizes"]) > 12
    assert not stats["greedy"][..., 1].any() and np.all(stats["hard_swaps"][..., 1] >= 1)
    assert all(cell["start"] == 1 and cell["lead"] >= 1e-6 for cell in reference("second_start")[0])
    for name in ("p63", "p64", "p65"):
        assert stats[name][0, 0, 1, 5] == 9 and stats[name][0, 3, 1, 4] == 2 and case(name)["starts"][0, 1, -1] != 0.0
    assert case("p65")["starts"][0, 1, :64].any()  # the surplus and what stays sit in different slots
    assert np.abs(reference("box")[0][0]["beta"]).max() == case("box")["big_M"]
    assert len(set(np.flatnonzero(reference("p1024")[0][1]["beta"]) // 64)) == 16
    assert case("ridge_wide")["X"].shape == (20, 40) and stats["ridge_wide"][0, 1, 0, 3] == 25
    assert len(case("sixteen_sets")["weights"]) == 16 and all(len(np.unique(w)) > 2 for w in case("sixteen_sets")["weights"])


# ---- selection rules on a hand-made score table ---------------------------------------------------------------------------------
def _hand_made():
    from sparselm_amd.miqp import L0LocalSubsets, L0LocalSubsetsCV

    sizes, etas = np.array([1, 2, 4]), np.array([0.0, 1.0])
    coefs = np.arange(3 * 2 * 4, dtype=float).reshape(3, 2, 4)
    zeros = np.zeros((3, 2))
    path = L0LocalSubsets(sizes, etas, coefs, np.arange(6.0).reshape(3, 2), zeros, zeros, 1, zeros[None], zeros, zeros, zeros, zeros,
                          np.ones((3, 2), bool))
    # folds x K x E.  Means: (1, 0) -1.0, (1, 1) -1.1, (2, 0) -0.95 with a spread, (2, 1) -2, (4, 0) -1.02, (4, 1) -3
    scores = np.array([[[-1.0, -1.1], [-0.65, -2.0], [-1.02, -3.0]],
                       [[-1.0, -1.1], [-1.25, -2.0], [-1.02, -3.0]]])
    return L0LocalSubsetsCV([path, path], path, [(np.arange(2), np.arange(2, 4))] * 2, scores, "neg_root_mean_squared_error", {"launches": 1})


def test_selection_rules_on_a_hand_made_table():
    from sparselm_amd.model_selection import _format_results, select_best_index_onestd

    cv = _hand_made()
    res = cv.search()
    # ParameterGrid sorts the names: eta is the outer loop
    assert res.cv_results_["params"] == list(ParameterGrid({"sparse_bound": [1, 2, 4], "eta": [0.0, 1.0]}))
    for key in ("params", "split0_test_score", "split1_test_score", "mean_test_score", "std_test_score", "rank_test_score"):
        assert key in res.cv_results_, key
    np.testing.assert_allclose(res.cv_results_["mean_test_score"], [-1.0, -0.95, -1.02, -1.1, -2.0, -3.0])
    np.testing.assert_allclose(res.cv_results_["split1_test_score"], [-1.0, -1.25, -1.02, -1.1, -2.0, -3.0])
    # max_score: the best mean, cell (size 2, eta 0)
    assert res.best_index_ == 1 and res.best_params_ == {"eta": 0.0, "sparse_bound": 2}
    assert res.best_score_ == pytest.approx(-0.95) and res.best_score_std_ == pytest.approx(0.3)
    np.testing.assert_array_equal(res.coef_, cv.full_.coefs_[1, 0])
    assert res.intercept_ == cv.full_.intercepts_[1, 0] == 2.0 and res.proven_optimal_ is False
    np.testing.assert_array_equal(res.predict(np.eye(4)), cv.full_.coefs_[1, 0] + 2.0)
    # one_std_score: whatever the project's rule picks on the same table -- and it is not the best mean here
    one = cv.search(opt_selection_method="one_std_score")
    scores = cv.cell_scores_.transpose(0, 2, 1).reshape(2, 6).T
    want = select_best_index_onestd(_format_results(res.cv_results_["params"], scores, np.zeros_like(scores)))
    assert one.best_index_ == want != 1
    e, k = divmod(want, 3)
    np.testing.assert_array_equal(one.coef_, cv.full_.coefs_[k, e])
    assert one.cv_results_["params"] == res.cv_results_["params"]
    with pytest.raises(ValueError, match="opt_selection_method"):
        cv.search(opt_selection_method="median")


# ---- the host twin, on the CPU ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_l0_local_subsets_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l0_local_subsets_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "l0_local_subsets_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "l0_local_subsets_host_test: ok" in run.stdout
