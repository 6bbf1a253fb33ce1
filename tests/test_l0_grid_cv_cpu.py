"""The l0 profile grid without a GPU (``sparselm_amd.miqp.l1l0_profile_cv`` / ``l2l0_profile_cv``,
``slm_solve_l0_profile_grid``): the public surface; what is refused before any device is touched; ``search`` of a hand-built
``L0ProfileGridCV`` against numbers worked out here; the problems one call hands to the engine; and what the grid adds to
csrc/l0_host.hpp -- the problem index, the argument checks, the layout at up to 128 problems -- compiled with g++ and run on the
CPU, plainly and under AddressSanitizer + UndefinedBehaviorSanitizer (tests/l0_grid_host_test.cpp)."""

import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
from sklearn.datasets import make_regression
from sklearn.model_selection import KFold, ParameterGrid

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- the host code --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_l0_grid_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l0_grid_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "l0_grid_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "l0_grid_host_test: ok" in run.stdout


def test_the_host_test_knows_the_kernels_control_words():
    """tests/l0_grid_host_test.cpp repeats the kernel's control-word numbers (it compiles without HIP): they are the kernel's."""
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "l0_kernels.hpp")) as fh:
        kernels = fh.read()
    with open(os.path.join(ROOT, "tests", "l0_grid_host_test.cpp")) as fh:
        host = fh.read()
    words = {name: int(re.search(rf"\b{name} = (\d+)", kernels).group(1)) for name in ("L0_BATCH_QALL", "L0_BATCH_ETA", "L0_CTL_WORDS")}
    assert words == {"L0_BATCH_QALL": 9, "L0_BATCH_ETA": 10, "L0_CTL_WORDS": 11}
    assert "QALL_WORD = 9, ETA_WORD = 10, CTL_WORDS = 11" in host
    assert "L0_PROFILE_INC = L0_CTL_WORDS" in kernels  # (the incumbents follow the control words: the eta word moved them by one)


# ---- the public surface -------------------------------------------------------------------------------------------------------
def test_abi_names_the_grid_entry_and_keeps_its_version():
    from sparselm_amd import _engine

    assert _engine.ABI_VERSION == 24
    with open(os.path.join(ROOT, "include", "slm_engine.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "binding.cpp")) as fh:
        binding = fh.read()
    assert "#define SLM_ABI_VERSION 24" in header and "#define SLM_L0_GRID_MAX 128" in header
    name = "solve_l0_profile_grid"
    assert f"slm_{name}" in _engine.ABI_SYMBOLS and f"int slm_{name}(" in header and hasattr(_engine.Dataset, name)
    assert f"slm_{name}(" in binding and f'm.def("{name}"' in binding
    assert _engine.L0_GRID_MAX == 128
    for old in ("slm_solve_l0_profile_batch", "slm_solve_l0_l1_profile", "slm_solve_l0_profile"):  # what it generalises is still there
        assert old in _engine.ABI_SYMBOLS and f"int {old}(" in header


def test_the_pinned_export_lists_are_unchanged_and_the_new_names_are_attributes():
    import sparselm_amd.miqp as miqp
    from sparselm_amd.model import _l0_cv, _l0_grid_cv, _l0_profile, _l1l0_profile

    assert miqp.__all__ == ["BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L1L0", "L2L0"]
    assert _l0_cv.__all__ == ["l0_profile_cv", "L0ProfileCV"]
    assert _l0_profile.__all__ == ["l0_profile", "L0Profile"]
    assert _l1l0_profile.__all__ == ["l1l0_profile", "L1L0Profile"]
    assert miqp.l1l0_profile_cv is _l0_grid_cv.l1l0_profile_cv and miqp.l2l0_profile_cv is _l0_grid_cv.l2l0_profile_cv
    assert miqp.L0ProfileGridCV is _l0_grid_cv.L0ProfileGridCV
    assert _l0_grid_cv.MAX_PROBLEMS == 128


# ---- refusals before any device -----------------------------------------------------------------------------------------------
@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to open an engine fails the test: validation errors have to come first."""
    from sparselm_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were validated")

    monkeypatch.setattr(_engine, "get_engine", boom)


@pytest.mark.parametrize("which", ["l1l0_profile_cv", "l2l0_profile_cv"])
def test_what_is_refused_before_a_device_is_touched(no_device, which):
    import sparselm_amd.miqp as miqp

    fn = getattr(miqp, which)
    X, y = make_regression(40, 8, n_informative=3, random_state=0)
    etas = [0.1, 1.0]
    # what l0_profile_cv refuses
    with pytest.raises(ValueError, match="wide"):
        fn(X, y, etas=etas, solver_options={"wide": True})
    with pytest.raises(ValueError, match="wide"):
        fn(X, y, etas=etas, solver_options={"wide": False})  # (the option itself, whatever its value)
    with pytest.raises(ValueError, match="bound"):
        fn(X, y, etas=etas, solver_options={"bound": "exclusion"})
    with pytest.raises(ValueError, match="unknown solver_options"):
        fn(X, y, etas=etas, solver_options={"max_node": 10})
    with pytest.raises(ValueError, match="splits"):
        fn(X, y, etas=etas, cv=16)
    with pytest.raises(ValueError, match="scoring"):
        fn(X, y, etas=etas, scoring="r2")
    with pytest.raises(ValueError, match="max_groups"):
        fn(X, y, etas=etas, max_groups=9)
    with pytest.raises(ValueError):
        fn(X, y, etas=etas, alpha_min=-1.0)
    # the etas
    with pytest.raises(ValueError, match="empty"):
        fn(X, y, etas=[])
    with pytest.raises(ValueError, match="finite and >= 0"):
        fn(X, y, etas=[0.1, -0.2])
    with pytest.raises(ValueError, match="finite and >= 0"):
        fn(X, y, etas=[0.1, np.nan])
    with pytest.raises(ValueError, match="finite and >= 0"):
        fn(X, y, etas=[np.inf])
    # the cap: (5 + 1) x 22 = 132 problems, (15 + 1) x 9 = 144
    with pytest.raises(ValueError, match="at most 128 problems"):
        fn(X, y, etas=np.linspace(0.1, 1.0, 22), cv=5)
    with pytest.raises(ValueError, match="at most 128 problems"):
        fn(X, y, etas=np.linspace(0.1, 1.0, 9), cv=15)
    # ... and what is admissible gets as far as the device: (15 + 1) x 8 = 128 problems, the other fast scoring
    with pytest.raises(AssertionError, match="device was touched"):
        fn(X, y, etas=np.linspace(0.1, 1.0, 8), cv=15, scoring="neg_mean_squared_error", solver_options={"max_nodes": 10})
    with pytest.raises(AssertionError, match="device was touched"):
        fn(X, y, etas=[0.0])  # (a weight of zero is a weight)


def test_only_the_ridge_kind_takes_a_tikhonov_matrix(no_device):
    from sparselm_amd.miqp import l1l0_profile_cv, l2l0_profile_cv

    X, y = make_regression(40, 8, n_informative=3, random_state=0)
    with pytest.raises(TypeError):
        l1l0_profile_cv(X, y, etas=[0.1], tikhonov_w=np.eye(8))
    with pytest.raises(ValueError, match="tikhonov_w"):
        l2l0_profile_cv(X, y, etas=[0.1], tikhonov_w=np.eye(7))


# ---- a hand-built grid: ParameterGrid order, ranks, both selection rules, the model of the right eta ------------------------------
def hand_built(alpha_min=0.0):
    """Two etas, three folds and all rows, sizes 0 .. 2 over two single-column groups, every number chosen by hand.

    eta = 0.5: every table's values are 0, -6, -8, so the regularised size is 2 below alpha = 2, 1 below 6, 0 above.
    eta = 2.0: every table's values are 0, -4, -4.5: size 2 below alpha = 0.5, 1 below 4, 0 above.
    Held-out scores per (fold, size):  eta 0.5: [[-9, -3, -2], [-9, -5, -1], [-9, -4, -3]];  eta 2.0: [[-9, -2, -4], [-9, -2, -5], [-9, -2, -6]]."""
    from sparselm_amd.miqp import L0ProfileCV, L0ProfileGridCV, L1L0Profile

    def table(values, eta, tag):
        values = np.array(values, dtype=float)
        supports = np.tril(np.ones((3, 2), dtype=bool), -1)  # size k: the first k groups
        coefs = supports * (tag + np.arange(3)[:, None])
        info = {"nodes": 5, "launches": 1, "q_all": float(values[-1]), "status": "optimal", "proven_optimal": True, "box_tol": 1e-12,
                "descents": 3}
        return L1L0Profile(values, supports, coefs.astype(float), np.arange(3) * 0.5 + tag, alpha_min, eta, info)

    splits = [(np.arange(3), np.arange(3, 4))] * 3
    cvs = []
    for eta, values, scores, tag in ((0.5, [0, -6, -8], [[-9, -3, -2], [-9, -5, -1], [-9, -4, -3]], 100),
                                     (2.0, [0, -4, -4.5], [[-9, -2, -4], [-9, -2, -5], [-9, -2, -6]], 200)):
        folds = [table(values, eta, tag + 10 * f) for f in range(3)]
        full = table(values, eta, tag + 50)
        info = {"problems": [t.solver_info_ for t in folds + [full]], "launches": 1, "proven_optimal": True, "nodes": 20}
        cvs.append(L0ProfileCV(folds, full, splits, np.array(scores, dtype=float), "neg_root_mean_squared_error", info))
    problems = [cvs[e].solver_info_["problems"][r] for r in range(4) for e in range(2)]
    return L0ProfileGridCV([0.5, 2.0], cvs, splits, "neg_root_mean_squared_error",
                           {"problems": problems, "launches": 1, "proven_optimal": True, "nodes": 40})


def test_search_of_a_hand_built_grid():
    grid = hand_built()
    alphas = [0.25, 1.0, 3.0, 7.0]
    res = grid.search(alphas)
    r = res.cv_results_
    assert r["params"] == list(ParameterGrid({"alpha": alphas, "eta": [0.5, 2.0]}))
    assert r["params"][:3] == [{"alpha": 0.25, "eta": 0.5}, {"alpha": 0.25, "eta": 2.0}, {"alpha": 1.0, "eta": 0.5}]
    # sizes (eta 0.5, eta 2.0): alpha 0.25 -> 2, 2;  1 -> 2, 1;  3 -> 1, 1;  7 -> 0, 0
    want = np.array([[-2, -1, -3], [-4, -5, -6], [-2, -1, -3], [-2, -2, -2], [-3, -5, -4], [-2, -2, -2], [-9, -9, -9], [-9, -9, -9]], dtype=float)
    for f in range(3):
        np.testing.assert_array_equal(r[f"split{f}_test_score"], want[:, f])
    np.testing.assert_allclose(r["mean_test_score"], want.mean(axis=1), rtol=1e-15)
    np.testing.assert_allclose(r["std_test_score"], want.std(axis=1), rtol=1e-15)
    # means: -2, -5, -2, -2, -4, -2, -9, -9: four candidates tie at -2, scikit-learn's "min" ranks give them all 1
    assert r["rank_test_score"].tolist() == [1, 6, 1, 1, 5, 1, 7, 7]
    # max_score: the first of the best, (alpha 0.25, eta 0.5) -- size 2 of the all-rows table of eta 0.5 (tag 150)
    assert res.best_index_ == 0 and res.best_params_ == {"alpha": 0.25, "eta": 0.5} and res.best_score_ == -2.0
    assert res.active_groups_.tolist() == [True, True] and res.coef_.tolist() == [152.0, 152.0] and res.intercept_ == 151.0
    np.testing.assert_array_equal(res.predict(np.eye(2)), np.array([303.0, 303.0]))
    # with the first candidate spoiled the best is (alpha 1, eta 0.5); then only eta 2.0 keeps a mean of -2: the model moves tables
    grid.cvs_[0].size_scores_[:, 2] = [-2.5, -3.5, -3.0]  # eta 0.5, size 2: mean -3
    moved = grid.search(alphas)
    assert moved.cv_results_["mean_test_score"].tolist() == [-3.0, -5.0, -3.0, -2.0, -4.0, -2.0, -9.0, -9.0]
    assert moved.best_index_ == 3 and moved.best_params_ == {"alpha": 1.0, "eta": 2.0}
    # ... size 1 of the all-rows table of eta 2.0 (tag 250)
    assert moved.active_groups_.tolist() == [True, False] and moved.coef_.tolist() == [251.0, 0.0] and moved.intercept_ == 250.5
    with pytest.raises(ValueError, match="opt_selection_method"):
        grid.search(alphas, opt_selection_method="best")
    with pytest.raises(ValueError, match="no alpha"):
        grid.search([])


def test_one_std_selection_of_a_hand_built_grid():
    from sparselm_amd.model_selection import select_best_index_onestd

    grid = hand_built()
    grid.cvs_[0].size_scores_[:, 2] = [-2.5, -3.5, -3.0]
    grid.cvs_[1].size_scores_[:, 1] = [-1.0, -2.0, -3.0]  # eta 2.0, size 1: mean -2, std sqrt(2/3)
    alphas = [0.25, 1.0, 3.0, 7.0]
    best = grid.search(alphas)
    onestd = grid.search(alphas, opt_selection_method="one_std_score")
    # the rule is model_selection's own, applied to the same results
    assert onestd.best_index_ == select_best_index_onestd(best.cv_results_)
    assert onestd.cv_results_["params"] == best.cv_results_["params"]
    np.testing.assert_array_equal(onestd.cv_results_["mean_test_score"], best.cv_results_["mean_test_score"])
    e = [0.5, 2.0].index(onestd.best_params_["eta"])
    size = grid.cvs_[e].full_.regularized_size(onestd.best_params_["alpha"])
    np.testing.assert_array_equal(onestd.coef_, grid.cvs_[e].full_.coefs_[size])
    assert onestd.intercept_ == grid.cvs_[e].full_.intercepts_[size]
    # every eta's own one-parameter search still works as it is
    one = grid.cvs_[1].regularized_search(alphas)
    assert one.cv_results_["params"] == [{"alpha": a} for a in alphas]
    np.testing.assert_array_equal(one.cv_results_["mean_test_score"], best.cv_results_["mean_test_score"][1::2])


def test_a_pruned_grid_serves_its_own_alphas_only():
    grid = hand_built(alpha_min=0.5)
    assert grid.search([0.5, 3.0]).best_params_["alpha"] in (0.5, 3.0)
    with pytest.raises(ValueError, match="alpha_min"):
        grid.search([0.4, 3.0])


# ---- the problems of one call ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,kind", [("l1l0_profile_cv", 1), ("l2l0_profile_cv", 0)])
def test_the_problems_of_one_call(monkeypatch, which, kind):
    """The row sets and weights the functions hand to the engine: the folds' training masks times the sample weights, each
    normalised to sum to its row count, all rows last, the whole list of etas and its kind -- in exactly one call."""
    import sparselm_amd.miqp as miqp
    from sparselm_amd import _engine

    X, y = make_regression(20, 4, n_informative=2, random_state=0)
    w = np.linspace(0.5, 2.0, 20)
    seen = {"calls": 0}

    class Stand:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def set_groups(self, gidx, n_groups):
            seen["groups"] = (gidx, n_groups)

        def solve_l0_profile_grid(self, row_weights, n_effs, etas, **kw):
            seen["calls"] += 1
            seen.update(row_weights=row_weights, n_effs=n_effs, etas=etas, kw=kw)
            raise RuntimeError("far enough")

        def __getattr__(self, name):  # (no other entry is an acceptable route)
            raise AssertionError(f"the grid went through {name}")

    class Eng:
        def dataset(self, Xd, yd, **kw):
            seen["X"] = Xd
            return Stand()

    monkeypatch.setattr(_engine, "get_engine", lambda device=None: Eng())
    with pytest.raises(RuntimeError, match="far enough"):
        getattr(miqp, which)(X, y, etas=[0.3, 0.0, 1.5], cv=KFold(4), fit_intercept=True, sample_weight=w, max_groups=3,
                             solver_options={"max_nodes": 5})
    assert seen["calls"] == 1
    assert seen["X"].shape == (20, 5) and (seen["X"][:, 4] == 1.0).all() and np.array_equal(seen["X"][:, :4], X)
    assert seen["groups"] == (None, 5)
    assert seen["n_effs"] == [15, 15, 15, 15, 20] and len(seen["row_weights"]) == 5
    for f, (tr, te) in enumerate(KFold(4).split(X)):
        m = seen["row_weights"][f]
        assert (m[te] == 0.0).all() and abs(m.sum() - 15.0) <= 1e-12
        np.testing.assert_allclose(m[tr] / m[tr][0], w[tr] / w[tr][0], rtol=1e-14)
    np.testing.assert_allclose(seen["row_weights"][4], w * (20 / w.sum()), rtol=1e-14)
    assert np.asarray(seen["etas"]).tolist() == [0.3, 0.0, 1.5]  # in the caller's order, not sorted
    kw = seen["kw"]
    assert kw["eta_kind"] == kind and kw["intercept"] is True and kw["max_groups"] == 3 and kw["max_nodes"] == 5 and kw["T"] is None


def test_the_tables_and_the_warning_of_one_call(monkeypatch):
    """From a stand-in engine's outputs: problem r * n_eta + e goes to ``cvs_[e]``'s row set r, l1 tables carry their eta, the
    held-out scores are numpy's, and ONE warning names the starved problems."""
    from sklearn.exceptions import ConvergenceWarning

    from sparselm_amd import _engine
    from sparselm_amd.miqp import L0Profile, L1L0Profile, l1l0_profile_cv, l2l0_profile_cv

    X, y = make_regression(12, 2, n_informative=2, random_state=1)
    etas, n_sets, K = [0.25, 4.0], 4, 2

    class Stand:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def set_groups(self, gidx, n_groups):
            pass

        def solve_l0_profile_grid(self, row_weights, n_effs, etas, eta_kind, **kw):
            P = len(row_weights) * len(etas)
            b = np.arange(P, dtype=float)
            values = np.stack([np.array([0.0, -1.0 - v, -2.0 - v]) for v in b])
            masks = np.tile(np.array([0, 1, 3], dtype=np.uint64), (P, 1))
            coefs = np.zeros((P, K + 1, 2))
            coefs[:, 1, 0] = 1.0 + b
            coefs[:, 2, :] = (1.0 + b)[:, None]
            icpts = np.stack([np.array([0.5, 0.25, 0.125]) * (v + 1) for v in b])
            infos = [{"nodes": 10 + i, "launches": 1, "q_all": -3.0, "status": "node_budget" if i in (1, 6) else "optimal",
                      "proven_optimal": i not in (1, 6), "box_tol": 1e-12, **({"descents": i} if eta_kind == 1 else {})} for i in range(P)]
            return coefs, icpts, masks, values, infos

    class Eng:
        def dataset(self, Xd, yd, **kw):
            return Stand()

    monkeypatch.setattr(_engine, "get_engine", lambda device=None: Eng())
    for fn, kind in ((l1l0_profile_cv, L1L0Profile), (l2l0_profile_cv, L0Profile)):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            grid = fn(X, y, etas=etas, cv=KFold(3), fit_intercept=True)
        mine = [c for c in caught if issubclass(c.category, ConvergenceWarning)]
        assert len(mine) == 1
        text = str(mine[0].message)
        assert "2 of 8 problems" in text and "fold 0 at eta = 4" in text and "all rows at eta = 0.25" in text
        assert grid.etas_.tolist() == etas and len(grid.cvs_) == 2 and len(grid.splits_) == 3
        info = grid.solver_info_
        assert info["launches"] == 1 and not info["proven_optimal"] and info["nodes"] == sum(10 + i for i in range(8))
        assert [p["nodes"] for p in info["problems"]] == [10 + i for i in range(8)]  # the engine's order
        for e in range(2):
            cv = grid.cvs_[e]
            tables = cv.profiles_ + [cv.full_]
            for r, t in enumerate(tables):
                b = r * 2 + e
                assert type(t) is kind and t.values_.tolist() == [0.0, -1.0 - b, -2.0 - b] and t.solver_info_["nodes"] == 10 + b
                assert t.supports_.tolist() == [[False, False], [True, False], [True, True]]
                if kind is L1L0Profile:
                    assert t.eta_ == etas[e] and t.solver_info_["descents"] == b
            assert cv.solver_info_["proven_optimal"] is False  # (problem 1 is fold 0 at eta 4, problem 6 all rows at eta 0.25)
            for f, (_, te) in enumerate(grid.splits_):
                for k in range(K + 1):
                    resid = y[te] - (X[te] @ cv.profiles_[f].coefs_[k] + cv.profiles_[f].intercepts_[k])
                    assert cv.size_scores_[f, k] == -np.sqrt(np.mean(resid * resid))
            assert cv.regularized_search([0.5, 50.0]).cv_results_["params"] == [{"alpha": 0.5}, {"alpha": 50.0}]
