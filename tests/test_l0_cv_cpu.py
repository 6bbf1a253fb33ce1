"""The batched exact l0 profile without a GPU (``sparselm_amd.miqp.l0_profile_cv``, ``slm_solve_l0_profile_batch``): the public
surface; what is refused before any device is touched; scores, ranks and both selection rules of a hand-built ``L0ProfileCV``
against numbers worked out here; and what the batch adds to csrc/l0_host.hpp -- the layout of several problems in one block,
the elimination of an intercept column -- compiled with g++ and run on the CPU, plainly and under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/l0_batch_host_test.cpp)."""

import os
import shutil
import subprocess

import numpy as np
import pytest
from sklearn.datasets import make_regression
from sklearn.model_selection import KFold

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- the host code --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_l0_batch_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l0_batch_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "l0_batch_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "l0_batch_host_test: ok" in run.stdout


# ---- the public surface -------------------------------------------------------------------------------------------------------
def test_abi_names_the_batched_entry_and_keeps_its_version():
    from sparselm_amd import _engine

    assert _engine.ABI_VERSION == 24
    with open(os.path.join(ROOT, "include", "slm_engine.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "binding.cpp")) as fh:
        binding = fh.read()
    assert "#define SLM_ABI_VERSION 24" in header
    name = "solve_l0_profile_batch"
    assert f"slm_{name}" in _engine.ABI_SYMBOLS and f"int slm_{name}(" in header and hasattr(_engine.Dataset, name)
    assert f"slm_{name}(" in binding and f'm.def("{name}"' in binding
    for old in ("slm_solve_l0", "slm_solve_l0_profile", "slm_solve_l0_profile_wide"):  # the single entries are still there
        assert old in _engine.ABI_SYMBOLS and f"int {old}(" in header


def test_the_pinned_export_lists_are_unchanged():
    import sparselm_amd.miqp as miqp
    from sparselm_amd.model import _l0_cv, _l0_profile

    assert _l0_profile.__all__ == ["l0_profile", "L0Profile"]
    assert miqp.__all__ == ["BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L1L0", "L2L0"]
    assert miqp.l0_profile_cv is _l0_cv.l0_profile_cv and miqp.L0ProfileCV is _l0_cv.L0ProfileCV
    assert _l0_cv.__all__ == ["l0_profile_cv", "L0ProfileCV"]


# ---- refusals before any device -----------------------------------------------------------------------------------------------
@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to open an engine fails the test: validation errors have to come first."""
    from sparselm_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were validated")

    monkeypatch.setattr(_engine, "get_engine", boom)


def test_what_is_refused_before_a_device_is_touched(no_device):
    from sparselm_amd.miqp import l0_profile_cv

    X, y = make_regression(40, 8, n_informative=3, random_state=0)
    with pytest.raises(ValueError, match="wide"):
        l0_profile_cv(X, y, solver_options={"wide": True})
    with pytest.raises(ValueError, match="wide"):
        l0_profile_cv(X, y, solver_options={"wide": False})  # (the option itself, whatever its value)
    with pytest.raises(ValueError, match="bound"):
        l0_profile_cv(X, y, solver_options={"bound": "exclusion"})
    with pytest.raises(ValueError, match="unknown solver_options"):
        l0_profile_cv(X, y, solver_options={"max_node": 10})
    with pytest.raises(ValueError, match="splits"):
        l0_profile_cv(X, y, cv=16)
    with pytest.raises(ValueError, match="scoring"):
        l0_profile_cv(X, y, scoring="r2")
    with pytest.raises(ValueError, match="scoring"):
        l0_profile_cv(X, y, scoring="neg_mean_absolute_error")
    with pytest.raises(ValueError, match="max_groups"):
        l0_profile_cv(X, y, max_groups=9)
    with pytest.raises(ValueError):
        l0_profile_cv(X, y, alpha_min=-1.0)
    # ... and what is admissible gets as far as the device: 15 splits, the other fast scoring
    with pytest.raises(AssertionError, match="device was touched"):
        l0_profile_cv(X, y, cv=15, scoring="neg_mean_squared_error", solver_options={"max_nodes": 10})


# ---- a hand-built table: scores, ranks, both selection rules ------------------------------------------------------------------
def hand_built(alpha_min=0.0):
    """Three folds and all rows, sizes 0 .. 3 over three single-column groups, every number chosen by hand.  The folds' values
    fall by 8, 3, 1 (fold 2: by 8, 1, 0.5), so fold f's regularised size is 3 below alpha = 1 (fold 2: 0.5), 2 below 3 (1), 1
    below 8 and 0 above."""
    from sparselm_amd.miqp import L0Profile, L0ProfileCV

    def table(values, tag):
        values = np.array(values, dtype=float)
        supports = np.tril(np.ones((4, 3), dtype=bool), -1)  # size k: the first k groups
        coefs = supports * (tag + np.arange(4)[:, None])
        info = {"nodes": 7, "launches": 1, "q_all": float(values[-1]), "status": "optimal", "proven_optimal": True, "box_tol": 1e-12}
        return L0Profile(values, supports, coefs.astype(float), np.arange(4) * 0.5 + tag, alpha_min, info)

    folds = [table([0, -8, -11, -12], 10), table([0, -8, -11, -12], 20), table([0, -8, -9, -9.5], 30)]
    full = table([0, -8, -11, -12], 40)
    size_scores = np.array([[-9.0, -4.0, -2.0, -3.0],
                            [-8.0, -5.0, -1.0, -2.5],
                            [-10.0, -3.0, -3.5, -6.0]])
    splits = [(np.arange(3), np.arange(3, 4))] * 3
    info = {"problems": [t.solver_info_ for t in folds + [full]], "launches": 1, "proven_optimal": True, "nodes": 28}
    return L0ProfileCV(folds, full, splits, size_scores, "neg_root_mean_squared_error", info)


def test_regularized_search_of_a_hand_built_table():
    cvp = hand_built()
    alphas = [0.25, 0.75, 2.0, 5.0, 9.0]
    # sizes per fold: alpha 0.25 -> 3, 3, 3;  0.75 -> 3, 3, 2;  2 -> 2, 2, 1;  5 -> 1, 1, 1;  9 -> 0, 0, 0
    want = np.array([[-3.0, -2.5, -6.0], [-3.0, -2.5, -3.5], [-2.0, -1.0, -3.0], [-4.0, -5.0, -3.0], [-9.0, -8.0, -10.0]])
    res = cvp.regularized_search(alphas)
    r = res.cv_results_
    assert r["params"] == [{"alpha": a} for a in alphas]
    for f in range(3):
        np.testing.assert_array_equal(r[f"split{f}_test_score"], want[:, f])
    np.testing.assert_allclose(r["mean_test_score"], want.mean(axis=1), rtol=1e-15)
    np.testing.assert_allclose(r["std_test_score"], want.std(axis=1), rtol=1e-15)
    # means: -3.833, -3, -2, -4, -9
    assert r["rank_test_score"].tolist() == [3, 2, 1, 4, 5]
    assert res.best_index_ == 2 and res.best_params_ == {"alpha": 2.0} and res.best_score_ == -2.0
    assert abs(res.best_score_std_ - np.sqrt(2.0 / 3.0)) <= 1e-15
    # the model comes from the table of ALL rows at the chosen value: size 2 there (values 0, -8, -11, -12 at alpha 2)
    assert res.active_groups_.tolist() == [True, True, False] and res.coef_.tolist() == [42.0, 42.0, 0.0] and res.intercept_ == 41.0
    np.testing.assert_array_equal(res.predict(np.eye(3)), np.array([83.0, 83.0, 41.0]))
    # one standard error: the best mean -2 has std sqrt(2/3) = 0.816, the target is -2.816; among alpha >= 2 the means are
    # -2, -4, -9 and -2 is the closest -- the rule stays; with the grid cut to the three smallest alphas the same
    onestd = cvp.regularized_search(alphas, opt_selection_method="one_std_score")
    assert onestd.best_index_ == 2
    # ... and it moves where a more regularised candidate lies closer to the target: scores of alpha = 3.5 equal those of
    # alpha = 5 (sizes 1, 1, 1), mean -4; put a candidate with mean -3 at a larger alpha than the best
    cvp.size_scores_[:, 1] = [-2.5, -3.5, -3.0]  # size 1 now scores a mean of -3, 0.18 from the target; the best's own -2 is 0.82 away
    moved = cvp.regularized_search(alphas, opt_selection_method="one_std_score")
    assert moved.cv_results_["rank_test_score"].argmin() == 2 and moved.best_index_ == 3 and moved.best_params_ == {"alpha": 5.0}
    assert moved.active_groups_.tolist() == [True, False, False]
    assert cvp.regularized_search(alphas).best_index_ == 2  # max_score is unmoved
    with pytest.raises(ValueError, match="opt_selection_method"):
        cvp.regularized_search(alphas, opt_selection_method="best")


def test_best_subset_search_of_a_hand_built_table():
    cvp = hand_built()
    res = cvp.best_subset_search([1, 2, 3])
    r = res.cv_results_
    # every table falls strictly, so the best support of at most K' groups has K' groups: the columns 1 .. 3 of the scores
    want = cvp.size_scores_[:, 1:].T
    for f in range(3):
        np.testing.assert_array_equal(r[f"split{f}_test_score"], want[:, f])
    assert r["params"] == [{"sparse_bound": 1}, {"sparse_bound": 2}, {"sparse_bound": 3}]
    # means -4, -2.1667, -3.8333
    assert r["rank_test_score"].tolist() == [3, 1, 2] and res.best_params_ == {"sparse_bound": 2}
    assert res.active_groups_.tolist() == [True, True, False]
    with pytest.raises(ValueError, match="outside the table"):
        cvp.best_subset_search([4])


def test_a_pruned_table_serves_its_own_alphas_only():
    cvp = hand_built(alpha_min=0.5)
    assert cvp.regularized_search([0.5, 2.0]).best_params_ == {"alpha": 2.0}
    with pytest.raises(ValueError, match="alpha_min"):
        cvp.regularized_search([0.4, 2.0])
    with pytest.raises(ValueError, match="alpha_min"):
        cvp.best_subset_search([2])


def test_the_problems_of_one_call(monkeypatch):
    """The row sets ``l0_profile_cv`` hands to the engine: the folds' training masks times the sample weights, each normalised
    to sum to its row count, and all rows last -- read from the call it makes on a stand-in dataset."""
    from sparselm_amd import _engine
    from sparselm_amd.miqp import l0_profile_cv

    X, y = make_regression(20, 4, n_informative=2, random_state=0)
    w = np.linspace(0.5, 2.0, 20)
    seen = {}

    class Stand:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def set_groups(self, gidx, n_groups):
            seen["groups"] = (gidx, n_groups)

        def solve_l0_profile_batch(self, row_weights, n_effs, **kw):
            seen.update(row_weights=row_weights, n_effs=n_effs, kw=kw)
            raise RuntimeError("far enough")

    class Eng:
        def dataset(self, Xd, yd, **kw):
            seen["X"] = Xd
            return Stand()

    monkeypatch.setattr(_engine, "get_engine", lambda device=None: Eng())
    with pytest.raises(RuntimeError, match="far enough"):
        l0_profile_cv(X, y, cv=KFold(4), fit_intercept=True, sample_weight=w, max_groups=3, solver_options={"max_nodes": 5})
    assert seen["X"].shape == (20, 5) and (seen["X"][:, 4] == 1.0).all() and np.array_equal(seen["X"][:, :4], X)
    assert seen["groups"] == (None, 5)  # single columns stay single columns, the ones column among them
    assert seen["n_effs"] == [15, 15, 15, 15, 20] and len(seen["row_weights"]) == 5
    for f, (tr, te) in enumerate(KFold(4).split(X)):
        m = seen["row_weights"][f]
        assert (m[te] == 0.0).all() and abs(m.sum() - 15.0) <= 1e-12
        np.testing.assert_allclose(m[tr] / m[tr][0], w[tr] / w[tr][0], rtol=1e-14)
    np.testing.assert_allclose(seen["row_weights"][4], w * (20 / w.sum()), rtol=1e-14)
    assert seen["kw"]["intercept"] is True and seen["kw"]["max_groups"] == 3 and seen["kw"]["max_nodes"] == 5
