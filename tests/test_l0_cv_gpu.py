"""The batched exact l0 profile on the GPU (``sparselm_amd.miqp.l0_profile_cv``, ``slm_solve_l0_profile_batch``, the BATCH
instantiation of csrc/l0_kernels.hpp): the profile of every cross-validation fold's training rows and of all rows from ONE
launch, against the per-size brute force of tests/_l0_profile_reference.py on each fold's own rows, against the single
``l0_profile`` and against the project's ``GridSearchCV`` going fit by fit.

Tolerances and the well-posedness premise are those of tests/test_l0_gpu.py, imported, per fold and per size: the
reference's best-to-second gap is >= 1e-6 and the condition number of its winner's block <= 1e4 -- asserted on the reference's
numbers first -- and then identical supports, objectives to 1e-10, coefficients to 1e-9.  No size and no fold is skipped.
With an intercept a fold's reference rows are centred by that fold's own means; with sample weights by the weighted means,
and scaled by sqrt(w), as tests/test_l0_profile_gpu.py does for one row set.

Designs, with ``KFold(5, shuffle=True, random_state=0)``: ``make_regression(50, 12, n_informative=5, noise=30.0, bias=-15.0,
random_state=0)`` in singletons and the same call at 50 x 24 in 12 groups of 2 (every fold's table falls strictly, smallest
gap 4.0e-6); below the ticket prefix ``suppressor(20)`` of tests/test_l0_search_gpu.py with K = 4 (6 196 supports per fold,
gaps >= 3.0e-3)."""

import functools
import warnings

import numpy as np
import pytest
from sklearn.datasets import make_regression
from sklearn.exceptions import ConvergenceWarning
from sklearn.model_selection import KFold

from _l0_profile_reference import profile_table, regularized_of
from _l0_reference import objective_of, search_rank
from test_l0_gpu import COEF_RTOL, GAP_MIN, KAPPA_MAX, OBJ_RTOL
from test_l0_profile_gpu import compare_table
from test_l0_profile_gpu import design as single_design
from test_l0_search_gpu import HIER, PREFIX, expected_nodes, suppressor

pytestmark = pytest.mark.gpu

CV = KFold(5, shuffle=True, random_state=0)
REL_ALPHAS = (1e-4, 1e-3, 1e-2, 0.1, 0.5)  # the grid of test 7, times var y
WEIGHT_SEED = 5


# ---- designs and references, computed once -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def design(grouped):
    X, y = make_regression(50, 24 if grouped else 12, n_informative=5, noise=30.0, bias=-15.0, random_state=0)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y, (np.repeat(np.arange(12), 2) if grouped else None)


@functools.lru_cache(maxsize=None)
def sample_weight():
    w = np.random.default_rng(WEIGHT_SEED).uniform(0.5, 2.0, 50)
    w.setflags(write=False)
    return w


def row_sets(n):
    """The folds' training rows, then all rows: the problems of one call, in its order."""
    return [tr for tr, _ in CV.split(np.zeros((n, 1)))] + [np.arange(n)]


def centred(X, y, rows, w=None):
    """The rows of one problem as its reference sees them: centred by their own (weighted) means, scaled by sqrt(w)."""
    Xr, yr = X[rows], y[rows]
    if w is None:
        xm, ym = Xr.mean(axis=0), yr.mean()
        return Xr - xm, yr - ym, xm, ym
    wn = w[rows] * (len(rows) / w[rows].sum())
    xm, ym = np.average(Xr, axis=0, weights=wn), np.average(yr, weights=wn)
    return (Xr - xm) * np.sqrt(wn)[:, None], (yr - ym) * np.sqrt(wn), xm, ym


@functools.lru_cache(maxsize=None)
def fold_tables(grouped, weighted=False):
    """Per problem (five folds, then all rows): (rows, centred X, centred y, x mean, y mean, brute-force table)."""
    X, y, groups = design(grouped)
    out = []
    for rows in row_sets(len(y)):
        Xp, yp, xm, ym = centred(X, y, rows, sample_weight() if weighted else None)
        out.append((rows, Xp, yp, xm, ym, profile_table(Xp, yp, groups=groups, K=12, big_M=1000)))
    return out


@functools.lru_cache(maxsize=None)
def deep_tables(hierarchy=False):
    """suppressor(20) (with the hierarchy: HIER's three pairs and three needs across the prefix), K = 4, no intercept: per
    problem (rows, table), and the hierarchy in the caller's labels."""
    if hierarchy:
        X, y, groups, _, _ = suppressor(HIER["ng"], **HIER["design"])
        at = np.argsort(search_rank(X, y))  # (the order of ALL rows: the needs are fixed labels, every fold ranks them its own way)
        need = [[] for _ in range(HIER["ng"])]
        need[at[16]] = [int(at[0])]
        need[at[2]] = [int(at[19])]
        need[at[18]] = [int(at[19])]
    else:
        X, y, groups, _, _ = suppressor(20)
        need = None
    assert groups is None
    return X, y, need, [(rows, profile_table(X[rows], y[rows], K=4, big_M=1000, hierarchy=need)) for rows in row_sets(len(y))]


def assert_all_finished(cvp, count):
    info = cvp.solver_info_
    assert info["launches"] == 1 and info["proven_optimal"] and len(info["problems"]) == count
    for prob in info["problems"]:
        assert prob["proven_optimal"] and prob["status"] == "optimal" and prob["launches"] == 1 and prob["nodes"] >= 0
    assert all(prof.proven_optimal_ for prof in cvp.profiles_) and cvp.full_.proven_optimal_


# ---- 1. one problem equals the single entry -------------------------------------------------------------------------------------
def test_one_problem_is_the_single_profile():
    from sparselm_amd import _engine

    if _engine.load_binding() is None:
        pytest.fail("the compiled binding is not built")
    X, y, _ = single_design(0)
    with _engine.get_engine().dataset(X, y) as ds:
        single = ds.solve_l0_profile(max_groups=12, big_M=1000.0)
        for route in (False, True):
            betas, icpts, masks, values, infos = ds.solve_l0_profile_batch([None], [0], max_groups=12, big_M=1000.0, binding=route)
            assert betas.shape == (1, 13, 12) and masks.shape == values.shape == icpts.shape == (1, 13) and len(infos) == 1
            assert np.array_equal(values[0], single[2]) and np.array_equal(masks[0], single[1]) and np.array_equal(betas[0], single[0])
            assert not icpts.any() and infos[0]["proven_optimal"] and infos[0]["launches"] == 1
            assert infos[0]["q_all"] == single[3]["q_all"]


# ---- 2. per-fold tables against the brute force --------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped,weighted", [(False, False), (True, False), (False, True)])
def test_every_fold_equals_enumeration(grouped, weighted):
    from sparselm_amd.miqp import l0_profile_cv

    X, y, groups = design(grouped)
    problems = fold_tables(grouped, weighted)
    for b, (_, _, _, _, _, table) in enumerate(problems):  # the premise, every problem and every size
        print(f"problem {b}: smallest gap {table['gaps'][1:12].min():.3e}, largest kappa {table['kappas'].max():.3e}")
        assert (table["gaps"][1:12] >= GAP_MIN).all() and (np.diff(table["values"]) < 0).all() and (table["kappas"] <= KAPPA_MAX).all()
    cvp = l0_profile_cv(X, y, cv=CV, groups=groups, max_groups=12, big_M=1000, fit_intercept=True,
                        sample_weight=sample_weight() if weighted else None)
    assert_all_finished(cvp, 6)
    assert len(cvp.profiles_) == 5 and cvp.size_scores_.shape == (5, 13) and np.isfinite(cvp.size_scores_).all()
    for b, (prof, (rows, Xp, yp, xm, ym, table)) in enumerate(zip(cvp.profiles_ + [cvp.full_], problems)):
        print(f"--- problem {b}")
        if b < 5:
            np.testing.assert_array_equal(cvp.splits_[b][0], rows)
        compare_table(prof, table, Xp, yp)
        for k in range(13):
            # ybar - xbar^T coef at the engine's own coefficients: the means are sums of at most 50 terms, so they and the dot
            # product round at a few 50 * 2^-53 of their terms' magnitudes -- 1e-12 of them is two orders above that
            want = ym - xm @ prof.coefs_[k]
            assert abs(prof.intercepts_[k] - want) <= 1e-12 * (abs(ym) + np.abs(xm) @ np.abs(prof.coefs_[k]))
    # the held-out scores are what numpy gives for those coefficients
    for f, (tr, te) in enumerate(cvp.splits_):
        for k in range(13):
            r = y[te] - (X[te] @ cvp.profiles_[f].coefs_[k] + cvp.profiles_[f].intercepts_[k])
            assert cvp.size_scores_[f, k] == -np.sqrt(np.mean(r * r))


# ---- 3. folds have different search orders --------------------------------------------------------------------------------------
def test_every_problem_searches_in_its_own_order():
    from sparselm_amd.miqp import l0_profile_cv

    X, y, need, problems = deep_tables(hierarchy=True)
    ranks = [tuple(search_rank(X[rows], y[rows])) for rows, _ in problems]
    print(f"distinct search orders among the six problems: {len(set(ranks))}")
    assert len(set(ranks[:5])) >= 2  # the premise: one order (or one set of masks, or group starts) for all would be wrong for some fold
    free = profile_table(X[problems[0][0]], y[problems[0][0]], K=4, big_M=1000)
    assert any(not np.array_equal(free["actives"][k], problems[0][1]["actives"][k]) for k in range(1, 5))  # the hierarchy changes a table
    cvp = l0_profile_cv(X, y, cv=CV, max_groups=4, hierarchy=need, big_M=1000)
    assert_all_finished(cvp, 6)
    for b, (prof, (rows, table)) in enumerate(zip(cvp.profiles_ + [cvp.full_], problems)):
        print(f"--- problem {b}")
        compare_table(prof, table, X[rows], y[rows])
        assert (prof.intercepts_ == 0.0).all()
        for k in range(1, 5):
            for i in np.flatnonzero(prof.supports_[k]):
                assert all(prof.supports_[k][q] for q in need[i])


# ---- 4. below the ticket prefix ---------------------------------------------------------------------------------------------------
def test_below_the_ticket_prefix_every_problem_counts_its_own_nodes():
    from sparselm_amd.miqp import l0_profile, l0_profile_cv

    X, y, _, problems = deep_tables()
    for b, (rows, table) in enumerate(problems):  # the premises: well-posed, deep, and nothing prunes but the cardinality
        rank = search_rank(X[rows], y[rows])
        deep = [k for k in range(1, 5) if (rank[np.flatnonzero(table["actives"][k])] >= PREFIX).any()]
        print(f"problem {b}: supports {table['n_supports']}, smallest gap {table['gaps'][1:].min():.3e}, deep sizes {deep}")
        assert deep == [2, 3, 4] and table["n_supports"] == 6196
        assert np.linalg.matrix_rank(X[rows]) == 20 and len(rows) > 20
    cvp = l0_profile_cv(X, y, cv=CV, max_groups=4, big_M=1000)
    assert_all_finished(cvp, 6)
    for b, (prof, (rows, table)) in enumerate(zip(cvp.profiles_ + [cvp.full_], problems)):
        print(f"--- problem {b}: nodes {prof.solver_info_['nodes']}, expected {expected_nodes(20, 4)}")
        compare_table(prof, table, X[rows], y[rows])
        assert prof.solver_info_["nodes"] == expected_nodes(20, 4)
        single = l0_profile(X[rows], y[rows], max_groups=4, big_M=1000)
        assert single.solver_info_["nodes"] == prof.solver_info_["nodes"]
        assert np.array_equal(single.supports_, prof.supports_)


# ---- 5. starved budget ------------------------------------------------------------------------------------------------------------
def test_starved_budget_stops_every_problem_with_its_incumbents():
    from sparselm_amd.miqp import l0_profile_cv

    X, y, _, problems = deep_tables()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        cvp = l0_profile_cv(X, y, cv=CV, max_groups=4, big_M=1000, solver_options={"max_nodes": 1000})
    assert len([w for w in caught if issubclass(w.category, ConvergenceWarning)]) == 1
    info = cvp.solver_info_
    assert info["launches"] == 1 and not info["proven_optimal"]
    for b, (prof, (rows, table)) in enumerate(zip(cvp.profiles_ + [cvp.full_], problems)):
        print(f"problem {b}: {prof.solver_info_}")
        assert not prof.proven_optimal_ and prof.solver_info_["status"] == "node_budget" and prof.solver_info_["nodes"] >= 1000
        assert prof.solver_info_["nodes"] < expected_nodes(20, 4)
        for k in np.flatnonzero(np.isfinite(prof.values_)):
            assert prof.supports_[k].sum() == k and np.count_nonzero(prof.coefs_[k]) <= k
            at_coef = objective_of(X[rows], y[rows], prof.coefs_[k], k)
            assert abs(at_coef - prof.values_[k]) <= 1e-9 * max(abs(prof.values_[k]), np.finfo(float).tiny)
            assert prof.values_[k] >= table["values"][k] - OBJ_RTOL * abs(table["values"][k])  # an incumbent is never below the optimum


# ---- 6. alpha_min > 0 -------------------------------------------------------------------------------------------------------------
def test_pruned_tables_are_exact_from_alpha_min_up():
    from sparselm_amd.miqp import l0_profile_cv

    X, y, _ = design(False)
    problems = fold_tables(False)
    var = float(np.var(y))
    alpha_min = 1e-3 * var
    cvp = l0_profile_cv(X, y, cv=CV, big_M=1000, fit_intercept=True, alpha_min=alpha_min)
    full = l0_profile_cv(X, y, cv=CV, big_M=1000, fit_intercept=True)
    assert_all_finished(cvp, 6)
    for b, (prof, (rows, Xp, yp, _, _, table)) in enumerate(zip(cvp.profiles_ + [cvp.full_], problems)):
        top = 1.01 * float(yp @ yp) / (2 * len(yp))  # above what any support gains: the optimum is empty
        assert prof.alpha_min_ == alpha_min and prof.solver_info_["nodes"] <= (full.profiles_ + [full.full_])[b].solver_info_["nodes"]
        sizes = []
        for alpha in (alpha_min, 1e-2 * var, 0.05 * var, 0.2 * var, top):
            k = regularized_of(table, alpha)
            obj = table["values"] + alpha * np.arange(13)
            others = np.delete(obj, k)
            # the premise: the optimum over ALL supports is the best of size k, separated from the runner-up of its size (the
            # table's gap) and from every other size
            assert table["gaps"][k] >= GAP_MIN or k == 0
            assert (others.min() - obj[k]) >= GAP_MIN * max(abs(obj[k]), np.finfo(float).tiny) and table["kappas"][k] <= KAPPA_MAX
            coef, intercept, active = prof.regularized(alpha)
            sizes.append(int(active.sum()))
            np.testing.assert_array_equal(active, table["actives"][k])
            assert abs(prof.values_[k] - table["values"][k]) <= OBJ_RTOL * abs(table["values"][k])
            assert abs(objective_of(Xp, yp, coef, k, alpha=alpha) - obj[k]) <= OBJ_RTOL * max(abs(obj[k]), np.finfo(float).tiny)
            if k:
                assert np.max(np.abs(coef - table["coefs"][k])) <= COEF_RTOL * np.max(np.abs(table["coefs"][k]))
        print(f"problem {b}: sizes along the alphas {sizes}, nodes {prof.solver_info_['nodes']}")
        assert sizes[-1] == 0 and len(set(sizes)) >= 3
    with pytest.raises(ValueError, match="alpha_min"):
        cvp.regularized_search([0.999 * alpha_min])
    with pytest.raises(ValueError, match="alpha_min"):
        cvp.best_subset_search([3])


# ---- 7. against today's route ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["max_score", "one_std_score"])
def test_regularized_search_is_the_grid_search_fit_by_fit(method):
    from sparselm_amd.miqp import l0_profile_cv
    from sparselm_amd.model import RegularizedL0
    from sparselm_amd.model_selection import GridSearchCV

    X, y, groups = design(True)
    problems = fold_tables(True)
    grid = [r * float(np.var(y)) for r in REL_ALPHAS]
    for b, (_, _, _, _, _, table) in enumerate(problems):  # the premise: every (problem, alpha) optimum is separated
        for alpha in grid:
            obj = table["values"] + alpha * np.arange(13)
            k = int(np.argmin(obj))
            assert (np.delete(obj, k).min() - obj[k]) >= GAP_MIN * abs(obj[k]) and (table["gaps"][k] >= GAP_MIN or k == 0)
    cvp = l0_profile_cv(X, y, cv=CV, groups=groups, big_M=1000, fit_intercept=True)
    assert_all_finished(cvp, 6)
    mine = cvp.regularized_search(grid, opt_selection_method=method)
    theirs = GridSearchCV(RegularizedL0(groups=groups, fit_intercept=True, big_M=1000), {"alpha": grid}, cv=CV,
                          opt_selection_method=method).fit(X, y)
    print(f"{method}: mean scores {mine.cv_results_['mean_test_score']}, best {mine.best_params_}")
    assert mine.best_params_ == theirs.best_params_ and mine.best_index_ == theirs.best_index_
    assert [c["alpha"] for c in mine.cv_results_["params"]] == grid
    row_norm = float(np.max(np.sum(np.abs(X), axis=1)))
    for f, (tr, te) in enumerate(cvp.splits_):
        for i, alpha in enumerate(grid):
            est = RegularizedL0(groups=groups, alpha=alpha, fit_intercept=True, big_M=1000).fit(X[tr], y[tr])
            coef, intercept, active = cvp.profiles_[f].regularized(alpha)
            np.testing.assert_array_equal(active, est.active_groups_)
            top = float(np.max(np.abs(est.coef_))) if active.any() else 0.0
            assert np.max(np.abs(coef - est.coef_)) <= COEF_RTOL * top
            # predictions move by at most ||x_i||_1 ||coef - coef'||_inf, and a root mean square by no more than its terms
            a, b = mine.cv_results_[f"split{f}_test_score"][i], theirs.cv_results_[f"split{f}_test_score"][i]
            assert abs(a - b) <= COEF_RTOL * row_norm * max(top, np.finfo(float).tiny), (f, alpha, a, b)
    assert abs(mine.best_score_ - theirs.best_score_) <= COEF_RTOL * row_norm * float(np.max(np.abs(theirs.best_estimator_.coef_)))
    assert np.max(np.abs(mine.coef_ - theirs.best_estimator_.coef_)) <= COEF_RTOL * np.max(np.abs(theirs.best_estimator_.coef_))
    np.testing.assert_array_equal(mine.active_groups_, theirs.best_estimator_.active_groups_)
    np.testing.assert_allclose(mine.predict(X), theirs.predict(X), rtol=0, atol=COEF_RTOL * row_norm * float(np.max(np.abs(mine.coef_))))
    if method == "max_score":  # the winner the brute force's numbers give: alpha = 1e-2 var y, by a wide margin
        assert mine.best_index_ == 2 and np.sort(mine.cv_results_["mean_test_score"])[-1] - np.sort(mine.cv_results_["mean_test_score"])[-2] > 5.0


# ---- 8. refusals by both routes -------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_both_routes():
    from sparselm_amd import _engine
    from sparselm_amd import distributed as D

    if _engine.load_binding() is None:
        pytest.fail("the compiled binding is not built")
    X, y, _ = single_design(0)
    wide = np.random.default_rng(0).standard_normal((80, 66))
    with _engine.get_engine().dataset(X, y) as ds, _engine.get_engine().dataset(wide, wide[:, 0]) as ds66:
        for route in (False, True):
            with pytest.raises(ValueError, match="count"):
                ds.solve_l0_profile_batch([], [], binding=route)
            with pytest.raises(ValueError, match="count"):
                ds.solve_l0_profile_batch([None] * 17, [0] * 17, max_groups=1, binding=route)
            with pytest.raises(ValueError, match="need"):
                ds.solve_l0_profile_batch([None], [0], need=[1 << 12] + [0] * 11, binding=route)
            with pytest.raises(ValueError, match="need"):  # with an intercept there are 11 search groups: bit 11 is the group count
                ds.solve_l0_profile_batch([None], [0], intercept=True, need=[1 << 11] + [0] * 10, binding=route)
            with pytest.raises(ValueError, match="alpha_min"):
                ds.solve_l0_profile_batch([None], [0], alpha_min=-1.0, binding=route)
            with pytest.raises(NotImplementedError, match="64"):  # 66 columns: 65 search columns even with an intercept
                ds66.solve_l0_profile_batch([None], [0], intercept=True, max_groups=1, binding=route)
    eng = _engine.Engine(0)
    try:
        D.init_row_sharding(eng, rank=0, world_size=1)
        with eng.dataset(X, y) as ds:
            ds.set_global_rows(len(y))
            for route in (False, True):
                with pytest.raises(NotImplementedError, match="row-sharded"):
                    ds.solve_l0_profile_batch([None], [0], max_groups=3, binding=route)
    finally:
        eng.comm_destroy()
        eng.close()
