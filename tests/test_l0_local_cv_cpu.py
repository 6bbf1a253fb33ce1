"""``l0_local_cv`` without a GPU: the public surface (the C entry under ABI 24, ``ABI_SYMBOLS``, the binding, the ``Dataset``
method, the import path and the export lists), every refusal before a device is touched, the selection rules on a hand-made
score table, the premises of the GPU comparisons recomputed (tests/_l0_local_cv_cases.py), and the host side in
csrc/l0_host.hpp compiled with g++ and run on the CPU, plainly and under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/l0_local_folds_host_test.cpp)."""

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
from sklearn.datasets import make_regression
from sklearn.model_selection import KFold, ParameterGrid

from _l0_local_cv_cases import RUNS, case, distinct_supports, reference
from test_l0_local_gpu import MARGIN_MIN

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRY = "slm_solve_l0_local_folds"


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
    decl = " ".join(decl[: decl.index(");") + 1].split())  # (a comment of the declaration holds a semicolon)
    # the issue's declaration, word for word
    want = """int slm_solve_l0_local_folds(slm_dataset* ds, int32_t count, const double* const* row_weights /* [count], entries may be NULL */,
                                 const int64_t* n_effs /* [count] */, int32_t intercept, int32_t n_cells, const double* alphas,
                                 const double* etas /* [n_cells] each */, double big_M, int32_t n_starts,
                                 const double* starts /* count * n_cells * n_starts * ps, or NULL: one zero start */, int32_t swaps,
                                 double* beta_out /* count * n_cells * ps */, double* intercept_out /* count * n_cells, or NULL */,
                                 double* objective_out /* count * n_cells */, int32_t* start_out /* or NULL */,
                                 int32_t* stat_out /* count * n_cells * n_starts * 4: sweeps, swaps, status word, non-zeros of EVERY problem; or NULL */,
                                 slm_point_info* info /* count * n_cells, or NULL */)"""
    assert decl == " ".join(want.split())
    assert hasattr(_engine.Dataset, "solve_l0_local_folds")
    # the ctypes signature: the dataset, eleven arguments, five outputs, the records
    assert len(_engine.load_library().slm_solve_l0_local_folds.argtypes) == 18
    # the entries that were there are still there
    for name in ("slm_solve_l0_local", "slm_solve_l0_local_descent", "slm_solve_l0_profile_batch", "slm_solve_l0_profile_grid"):
        assert name in _engine.ABI_SYMBOLS and f"int {name}(" in header


def test_export_lists():
    import sparselm_amd.miqp as miqp
    from sparselm_amd.model import _l0_local, _l0_local_cv

    assert _l0_local_cv.__all__ == ["l0_local_cv", "L0LocalCV"]
    assert miqp.l0_local_cv is _l0_local_cv.l0_local_cv and miqp.L0LocalCV is _l0_local_cv.L0LocalCV
    assert "l0_local_cv" not in miqp.__all__ and "L0LocalCV" not in miqp.__all__
    assert miqp.__all__ == ["BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L1L0", "L2L0"]
    assert _l0_local.__all__ == ["l0_local_search", "L0LocalPath"]
    assert miqp.L0LocalCV.proven_optimal_ is False


def test_signature():
    from sparselm_amd.miqp import l0_local_cv

    params = inspect.signature(l0_local_cv).parameters
    assert list(params) == ["X", "y", "alphas", "etas", "cv", "big_M", "fit_intercept", "sample_weight", "starts", "max_rounds", "scoring",
                            "solver_options"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in params.items() if k not in ("X", "y"))
    assert params["alphas"].default is inspect.Parameter.empty
    assert [params[k].default for k in list(params)[3:]] == [(0.0,), 5, 100, False, None, None, 2, "neg_root_mean_squared_error", None]


def test_the_not_built_lists_no_longer_name_cv_folds():
    from sparselm_amd.model import _l0_local

    with open(os.path.join(ROOT, "include", "slm_engine.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        design = fh.read()
    assert "cross-validation folds in the launch, handing" not in _l0_local.__doc__
    assert "constraints, row sets (CV\n * folds) in the launch." not in header
    assert "Local search over folds" in design


# ---- refusals, all before a device ------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_device(no_device):
    from sparselm_amd.miqp import l0_local_cv

    X, y = make_regression(25, 6, n_informative=3, random_state=0)
    for bad in (dict(alphas=[-1.0]), dict(alphas=[np.nan]), dict(alphas=[np.inf]), dict(alphas=[]), dict(alphas=[[0.1]]),
                dict(alphas=[0.1], etas=[-1.0]), dict(alphas=[0.1], etas=[np.inf]), dict(alphas=[0.1], etas=[]),
                dict(alphas=[0.1], big_M=-1), dict(alphas=[0.1], max_rounds=-1), dict(alphas=[0.1], max_rounds=1.5),
                dict(alphas=[0.1], solver_options={"max_nodes": 5}), dict(alphas=[0.1], solver_options={"swaps": 1}),
                dict(alphas=[0.1], solver_options=[("swaps", True)]), dict(alphas=[0.1], fit_intercept="yes"),
                dict(alphas=[0.1], sample_weight=np.ones(24)),
                dict(alphas=[0.1], starts=np.zeros((2, 5))), dict(alphas=[0.1, 0.2], starts=np.zeros((1, 1, 2, 6))),
                dict(alphas=[0.1], big_M=1.0, starts=np.full((1, 6), 1.5)), dict(alphas=[0.1], starts=np.full((1, 6), np.nan)),
                dict(alphas=[0.1], scoring="r2"), dict(alphas=[0.1], cv=16), dict(alphas=[0.1], cv=KFold(20)), dict(alphas=[0.1], cv=1),
                dict(alphas=np.full(700, 0.1), etas=[0.0, 0.1], cv=2),                    # 3 row sets x 1 400 cells x 4 starts of a round
                dict(alphas=np.full(1500, 0.1), starts=np.zeros((1, 6)), max_rounds=0),   # 6 row sets x 1 500 cells x 2 starts
                dict(alphas=np.full(1400, 0.1), max_rounds=0)):                           # 6 row sets x 1 400 cells
        with pytest.raises(ValueError):
            l0_local_cv(X, y, **bad)
    with pytest.raises(ValueError):  # the first fold trains on rows 5 .. 24, which hold no weight
        l0_local_cv(X, y, alphas=[0.1], sample_weight=np.r_[np.ones(5), np.zeros(20)], cv=KFold(5))
    with pytest.raises(ValueError):
        l0_local_cv(X, y[:-1], alphas=[0.1])
    with pytest.raises(TypeError):
        l0_local_cv(X, y)
    with pytest.raises(TypeError):
        l0_local_cv(X, y, [0.1])
    with pytest.raises(NotImplementedError, match="1024"):
        l0_local_cv(np.zeros((6, 1025)), np.zeros(6), alphas=[0.1], cv=2)


def test_the_engine_names_every_refusal_itself():
    """The C entry refuses each of these before it touches a device, each in its own words (the order and the codes are checked
    by tests/l0_local_folds_host_test.cpp on ``l0_lsf_check``; the messages by the GPU tests on both routes)."""
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "engine_l0.hip")) as fh:
        unit = fh.read()
    body = unit[unit.index("int solve_l0_local_folds_impl("):]
    assert body.index("l0_lsf_check(") < body.index("hipSetDevice")
    rest = body[body.index("hipSetDevice"):]
    body = body[: body.index("hipSetDevice")]
    for words in ("takes up to %d columns", "not built for groups", "not built for row-sharded datasets", "alphas[%lld] must be finite and >= 0",
                  "etas[%lld] must be finite and >= 0", "big_M must be >= 0", "n_cells must be >= 1", "n_starts must be >= 1",
                  "count * n_cells * n_starts must be at most %d problems", "lies outside the box", "count must be 1 .. %d",
                  "row_weights[%d][%lld] must be finite and >= 0", "the last column must be alone in the last group"):
        assert words in body, words
    assert "gives the last column no weight" in rest  # (after the Grams, as in the batch entry)


# ---- selection rules on a hand-made score table ---------------------------------------------------------------------------------
def _hand_made():
    from sparselm_amd.miqp import L0LocalCV, L0LocalPath

    alphas, etas = np.array([0.1, 0.2, 0.4]), np.array([0.0, 1.0])
    coefs = np.arange(3 * 2 * 4, dtype=float).reshape(3, 2, 4)
    zeros = np.zeros((3, 2))
    path = L0LocalPath(alphas, etas, coefs, np.arange(6.0).reshape(3, 2), zeros, zeros, 1, zeros[None], zeros, zeros, np.ones((3, 2), bool))
    # folds x A x E.  Means: (0.1, 0) -1.0, (0.1, 1) -1.1, (0.2, 0) -0.95 with a spread, (0.2, 1) -2, (0.4, 0) -1.02, (0.4, 1) -3
    scores = np.array([[[-1.0, -1.1], [-0.65, -2.0], [-1.02, -3.0]],
                       [[-1.0, -1.1], [-1.25, -2.0], [-1.02, -3.0]]])
    return L0LocalCV([path, path], path, [(np.arange(2), np.arange(2, 4))] * 2, scores, "neg_root_mean_squared_error", {"launches": 1})


def test_selection_rules_on_a_hand_made_table():
    from sparselm_amd.model_selection import _format_results, select_best_index_onestd

    cv = _hand_made()
    res = cv.search()
    assert res.cv_results_["params"] == list(ParameterGrid({"alpha": [0.1, 0.2, 0.4], "eta": [0.0, 1.0]}))
    for key in ("params", "split0_test_score", "split1_test_score", "mean_test_score", "std_test_score", "rank_test_score"):
        assert key in res.cv_results_, key
    np.testing.assert_allclose(res.cv_results_["mean_test_score"], [-1.0, -1.1, -0.95, -2.0, -1.02, -3.0])
    np.testing.assert_allclose(res.cv_results_["split1_test_score"], [-1.0, -1.1, -1.25, -2.0, -1.02, -3.0])
    # max_score: the best mean, cell (alpha 0.2, eta 0)
    assert res.best_index_ == 2 and res.best_params_ == {"alpha": 0.2, "eta": 0.0}
    assert res.best_score_ == pytest.approx(-0.95) and res.best_score_std_ == pytest.approx(0.3)
    np.testing.assert_array_equal(res.coef_, cv.full_.coefs_[1, 0])
    assert res.intercept_ == cv.full_.intercepts_[1, 0] == 2.0 and res.proven_optimal_ is False
    np.testing.assert_array_equal(res.predict(np.eye(4)), cv.full_.coefs_[1, 0] + 2.0)
    # one_std_score: whatever the project's rule picks on the same table -- and it is not the best mean here
    one = cv.search(opt_selection_method="one_std_score")
    scores = cv.cell_scores_.reshape(2, 6).T
    want = select_best_index_onestd(_format_results(res.cv_results_["params"], scores, np.zeros_like(scores)))
    assert one.best_index_ == want != 2
    a, e = divmod(want, 2)
    np.testing.assert_array_equal(one.coef_, cv.full_.coefs_[a, e])
    assert one.cv_results_["params"] == res.cv_results_["params"]
    with pytest.raises(ValueError, match="opt_selection_method"):
        cv.search(opt_selection_method="median")


# ---- the premises of the GPU comparisons, recomputed --------------------------------------------------------------------------------
# what each case is there to cover: (cell, distinct supports over the row sets) and (row sets, cells)
COVERS = {("two_slots", False): ([(0, 2), (1, 3)], (4, 3)), ("two_slots", True): ([(1, 3)], (4, 3)),
          ("sixteen_row_sets", False): ([], (16, 2)), ("sixteen_row_sets", True): ([], (16, 2)),
          ("three_slots", False): ([(0, 6)], (6, 2)), ("three_slots", True): ([], (6, 2)),
          ("sixteen_slots", True): ([(0, 3)], (3, 1)), ("hard_3", True): ([], (4, 3)), ("hard_7", True): ([], (4, 3))}


@pytest.mark.parametrize("name,intercept", RUNS)
def test_premises_of_the_gpu_comparisons(name, intercept):
    X, y, rows, alphas, etas = case(name, intercept)
    ref = reference(name, intercept)
    distinct, shape = COVERS[(name, intercept)]
    assert (len(rows), len(alphas)) == shape == (len(ref), len(ref[0]))
    worst = min(min(cell["margin"], cell["lead"]) for cells in ref for cell in cells)
    print(f"{name} intercept {intercept}: smallest margin {worst:.3e}")
    for cells in ref:
        for cell in cells:
            assert cell["status"] == 0 and cell["margin"] >= MARGIN_MIN and cell["lead"] >= MARGIN_MIN
    for cell, count in distinct:  # a problem that reads the wrong row set's Gram fails the comparison
        assert distinct_supports(ref, cell) == count
    swaps = np.array([[cell["swaps"] for cell in cells] for cells in ref])
    if name == "sixteen_slots":
        live = np.flatnonzero(ref[-1][0]["beta"])
        assert X.shape[1] == 1024 and live.size == 16 and set(live // 64) == set(range(16))  # every slot live on all rows
    if name == "hard_7":
        assert swaps.min() >= 1 and swaps.max() == 2  # one or two swaps in EVERY problem
    if name == "hard_3":
        assert swaps.max() == 3 and np.count_nonzero(swaps.max(axis=1)) == 4  # swaps are accepted in every row set
    if name == "two_slots":
        assert X.shape[1] == 65  # ld = 80 != p; with the ones column p = 66


def test_a_second_start_wins_in_one_row_set_only():
    """The case tests/test_l0_local_cv_gpu.py runs with two starts, chosen here under the lead premise."""
    from _l0_local_cv_cases import second_start_case

    _, _, _, _, _, ref, wins = second_start_case()
    print(wins)
    for cells in ref:
        for cell in cells:
            assert cell["status"] == 0 and cell["margin"] >= MARGIN_MIN and cell["lead"] >= MARGIN_MIN
    for e in range(3):  # at every alpha some row set keeps the first start and another takes the second
        assert sorted(set(wins[:, e])) == [0, 1]


# ---- the host side, on the CPU ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_l0_local_folds_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l0_local_folds_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "l0_local_folds_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "l0_local_folds_host_test: ok" in run.stdout
