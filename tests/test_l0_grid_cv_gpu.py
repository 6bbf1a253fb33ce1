"""The l0 profile grid on the GPU (``sparselm_amd.miqp.l1l0_profile_cv`` / ``l2l0_profile_cv``, ``slm_solve_l0_profile_grid``: the
BATCH instantiations of csrc/l0_kernels.hpp with and without L1, one problem per (row set, eta)): every (fold, eta) table from ONE
launch, against the per-size brute force of tests/_l1l0_profile_reference.py on each problem's own centred rows, against the
single entries it generalises, against ``l0_profile_cv`` per eta, and against the project's ``GridSearchCV`` going fit by fit.

Tolerances are those of tests/test_l1l0_gpu.py, imported (gap >= 1e-6, kappa <= 1e4, objectives to 1e-10, coefficients to
1e-9), and every premise is asserted on the reference's numbers first.  Under an l1 term a table saturates; every test names
the rows that MUST be compared in full per problem (``compare_table`` of tests/test_l1l0_profile_gpu.py fails if one is
skipped), saturated rows are compared by value.

Base design: ``design(False)`` of tests/test_l0_cv_gpu.py (50 x 12), ``KFold(5, shuffle=True, random_state=0)``, an intercept,
``big_M = 1000``, ``max_groups = 6``, three l1 weights ``rel * ||Xc^T yc / 50||_inf`` of the centred all-rows data,
``rel = 0.02, 0.1, 0.3``: 18 problems.  Below the ticket prefix: ``suppressor(20)`` of tests/test_l0_search_gpu.py with K = 4,
no intercept, two l1 weights (relative 0.05 and 0.3) and THREE folds (``KFold(3, shuffle=True, random_state=0)``) -- eight
tables of 6 196 supports each; five folds would be twelve, and a table takes the reference five seconds.  At 0.05 the best
supports of every row set reach beyond the 16-group prefix (asserted); at 0.3 they do not (asserted too: the l1 weight is above
the hidden columns' correlation with y), and the search below the prefix has to find nothing better there."""

import functools
import warnings

import numpy as np
import pytest
from sklearn.exceptions import ConvergenceWarning
from sklearn.model_selection import KFold, ParameterGrid

from _l0_profile_reference import profile_table, regularized_of
from _l0_reference import search_rank
from _l1l0_profile_reference import profile_table_l1
from _l1l0_reference import objective_of_l1, solve_support_l1
from test_l0_cv_gpu import CV, centred, design, row_sets, sample_weight
from test_l0_profile_gpu import compare_table as compare_table_ridge
from test_l0_profile_gpu import design as single_design
from test_l0_search_gpu import PREFIX, suppressor
from test_l1l0_gpu import COEF_RTOL, GAP_MIN, KAPPA_MAX, OBJ_RTOL
from test_l1l0_profile_gpu import compare_table

pytestmark = pytest.mark.gpu

RELS = (0.02, 0.1, 0.3)
K = 6
BIG_M = 1000
CV3 = KFold(3, shuffle=True, random_state=0)
DEEP_RELS = (0.05, 0.3)
RIDGE_RELS = (0.01, 0.1, 0.5)  # times the mean diagonal of the centred all-rows Gram
# the lasso on all 12 columns uses this many columns (folds 0 - 4, then all rows), per rel: worked out with the reference alone
LASSO_NZ = {0.02: (9, 11, 10, 10, 12, 10), 0.1: (5, 5, 6, 6, 5, 5), 0.3: (4, 5, 4, 3, 4, 4)}


# ---- designs and references, computed once -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def l1_etas():
    X, y, _ = design(False)
    Xc, yc, _, _ = centred(X, y, np.arange(50))
    c = float(np.max(np.abs(Xc.T @ yc / 50)))
    return tuple(rel * c for rel in RELS)


@functools.lru_cache(maxsize=None)
def ridge_etas():
    X, y, _ = design(False)
    Xc, _, _, _ = centred(X, y, np.arange(50))
    d = float(np.trace(Xc.T @ Xc / 50) / 12)
    return tuple(rel * d for rel in RIDGE_RELS)


@functools.lru_cache(maxsize=None)
def l1_tables(weighted=False):
    """Per problem in the engine's order (row sets outermost, etas innermost): a dict with the rows, the centred data, the
    means, eta, the brute-force table to K = 6, and the lasso on all columns (its value f_all and the columns it uses)."""
    X, y, _ = design(False)
    out = []
    for rows in row_sets(50):
        Xp, yp, xm, ym = centred(X, y, rows, sample_weight() if weighted else None)
        for eta in l1_etas():
            b_all, f_all, _ = solve_support_l1(Xp, yp, np.arange(12), eta, BIG_M)
            out.append({"rows": rows, "X": Xp, "y": yp, "xm": xm, "ym": ym, "eta": eta, "f_all": float(f_all), "nz": int(np.count_nonzero(b_all)),
                        "table": profile_table_l1(Xp, yp, K=K, eta=eta, big_M=BIG_M)})
    return out


def full_rows(prob):
    """The rows that MUST be compared in full: 1 .. nz - 1, up to K."""
    return range(1, min(prob["nz"] - 1, K) + 1)


@functools.lru_cache(maxsize=None)
def ridge_tables():
    """Per problem in the engine's order for the three ridge weights: rows, centred data, eta, the brute-force table (all sizes)."""
    X, y, _ = design(False)
    out = []
    for rows in row_sets(50):
        Xp, yp, xm, ym = centred(X, y, rows)
        for eta in ridge_etas():
            out.append({"rows": rows, "X": Xp, "y": yp, "eta": eta, "table": profile_table(Xp, yp, K=12, eta=eta, big_M=BIG_M)})
    return out


def deep_row_sets(n):
    return [tr for tr, _ in CV3.split(np.zeros((n, 1)))] + [np.arange(n)]


@functools.lru_cache(maxsize=None)
def deep_tables():
    X, y, groups, _, _ = suppressor(20)
    assert groups is None
    c = float(np.max(np.abs(X.T @ y / len(y))))
    etas = tuple(rel * c for rel in DEEP_RELS)
    out = []
    for rows in deep_row_sets(len(y)):
        for eta in etas:
            out.append({"rows": rows, "eta": eta, "table": profile_table_l1(X[rows], y[rows], K=4, eta=eta, big_M=BIG_M)})
    return X, y, etas, out


def tables_of(grid):
    """The tables of a result in the engine's order: problem r * n_eta + e is row set r (the folds, then all rows) at etas_[e]."""
    n_sets = len(grid.splits_) + 1
    return [(grid.cvs_[e].profiles_ + [grid.cvs_[e].full_])[r] for r in range(n_sets) for e in range(len(grid.etas_))]


def assert_all_finished(grid, problems, l1=True):
    info = grid.solver_info_
    assert info["launches"] == 1 and info["proven_optimal"] and len(info["problems"]) == problems
    for prob, table in zip(info["problems"], tables_of(grid)):
        assert prob["proven_optimal"] and prob["status"] == "optimal" and prob["launches"] == 1 and prob["nodes"] >= 1
        assert table.solver_info_ is prob and table.proven_optimal_
        assert not l1 or prob["descents"] > 0
    assert info["nodes"] == sum(prob["nodes"] for prob in info["problems"])


def same_table(a, b):
    return (a.values_.tobytes() == b.values_.tobytes() and a.coefs_.tobytes() == b.coefs_.tobytes() and np.array_equal(a.supports_, b.supports_)
            and a.intercepts_.tobytes() == b.intercepts_.tobytes())


# ---- 1. every (fold, eta) table equals enumeration -----------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_every_fold_and_eta_equals_enumeration(weighted):
    from sparselm_amd.miqp import L1L0Profile, l1l0_profile_cv

    X, y, _ = design(False)
    problems = l1_tables(weighted)
    assert len(problems) == 18
    for b, prob in enumerate(problems):  # the premises, every problem
        table, full = prob["table"], list(full_rows(prob))
        print(f"problem {b} (row set {b // 3}, rel {RELS[b % 3]}): lasso columns {prob['nz']}, rows in full {full}, smallest gap "
              f"{table['gaps'][full].min():.3e}, largest kappa {table['kappas'][full].max():.3e}")
        if not weighted:
            assert prob["nz"] == LASSO_NZ[RELS[b % 3]][b // 3]
        assert len(full) >= 2 and (len(full) >= 5 or RELS[b % 3] != 0.02)
        assert (table["gaps"][full] >= GAP_MIN).all() and (table["kappas"][full] <= KAPPA_MAX).all() and table["n_supports"] == 2510
        assert (np.diff(table["values"][: full[-1] + 1]) < 0).all()
    grid = l1l0_profile_cv(X, y, etas=l1_etas(), cv=CV, max_groups=K, big_M=BIG_M, fit_intercept=True,
                           sample_weight=sample_weight() if weighted else None)
    assert_all_finished(grid, 18)
    assert grid.etas_.tolist() == list(l1_etas()) and len(grid.cvs_) == 3 and len(grid.splits_) == 5
    for b, (prof, prob) in enumerate(zip(tables_of(grid), problems)):
        print(f"--- problem {b}")
        assert type(prof) is L1L0Profile
        if b // 3 < 5:
            np.testing.assert_array_equal(grid.splits_[b // 3][0], prob["rows"])
        compare_table(prof, prob["table"], prob["X"], prob["y"], prob["eta"], full_rows(prob))
        for k in range(K + 1):
            # ybar - xbar^T coef at the engine's own coefficients (the bound of tests/test_l0_cv_gpu.py)
            want = prob["ym"] - prob["xm"] @ prof.coefs_[k]
            assert abs(prof.intercepts_[k] - want) <= 1e-12 * (abs(prob["ym"]) + np.abs(prob["xm"]) @ np.abs(prof.coefs_[k]))
    # the held-out scores are what numpy gives for those coefficients
    for e, cv in enumerate(grid.cvs_):
        assert cv.size_scores_.shape == (5, K + 1) and np.isfinite(cv.size_scores_).all()
        for f, (tr, te) in enumerate(grid.splits_):
            for k in range(K + 1):
                r = y[te] - (X[te] @ cv.profiles_[f].coefs_[k] + cv.profiles_[f].intercepts_[k])
                assert cv.size_scores_[f, k] == -np.sqrt(np.mean(r * r))


# ---- 2. one problem is the single entry ------------------------------------------------------------------------------------------
def test_one_problem_is_the_single_entry():
    from sparselm_amd import _engine

    if _engine.load_binding() is None:
        pytest.fail("the compiled binding is not built")
    X, y, _ = single_design(0)
    eta_l1 = 0.05 * float(np.max(np.abs(X.T @ y / 40)))
    eta_ridge = 0.1
    with _engine.get_engine().dataset(X, y) as ds:
        single_l1 = ds.solve_l0_l1_profile(max_groups=12, eta_l1=eta_l1, big_M=1000.0)
        single_ridge = ds.solve_l0_profile(max_groups=12, eta=eta_ridge, big_M=1000.0)
        assert single_l1[3]["descents"] > 0 and not np.array_equal(single_l1[2], single_ridge[2])  # (two different problems)
        for route in (False, True):
            for kind, eta, single in ((1, eta_l1, single_l1), (0, eta_ridge, single_ridge)):
                betas, icpts, masks, values, infos = ds.solve_l0_profile_grid([None], [0], [eta], eta_kind=kind, max_groups=12, big_M=1000.0,
                                                                              binding=route)
                assert betas.shape == (1, 13, 12) and masks.shape == values.shape == icpts.shape == (1, 13) and len(infos) == 1
                assert np.array_equal(values[0], single[2]) and np.array_equal(masks[0], single[1]) and np.array_equal(betas[0], single[0])
                assert not icpts.any() and infos[0]["proven_optimal"] and infos[0]["launches"] == 1
                assert infos[0]["q_all"] == single[3]["q_all"]
                assert ("descents" in infos[0]) == (kind == 1)


# ---- 3. the ridge grid is l0_profile_cv per eta ----------------------------------------------------------------------------------
def test_the_ridge_grid_is_l0_profile_cv_per_eta():
    from sparselm_amd.miqp import L0Profile, l0_profile_cv, l2l0_profile_cv

    X, y, _ = design(False)
    etas = ridge_etas()
    # the premise: at every size >= 1 the values of two etas differ by far more than OBJ_RTOL -- a grid that reused one H would fail
    full = [prob["table"] for prob in ridge_tables()[15:18]]  # all rows, the three etas
    for i in range(3):
        for j in range(i + 1, 3):
            rel = np.abs(full[i]["values"][1:] - full[j]["values"][1:]) / np.abs(full[i]["values"][1:])
            print(f"etas {i}, {j}: the values differ by at least {rel.min():.3e} (relative)")
            assert (rel >= 1e4 * OBJ_RTOL).all()
    grid = l2l0_profile_cv(X, y, etas=etas, cv=CV, big_M=BIG_M, fit_intercept=True)
    assert_all_finished(grid, 18, l1=False)
    for e, eta in enumerate(etas):
        one = l0_profile_cv(X, y, cv=CV, eta=eta, big_M=BIG_M, fit_intercept=True)
        mine = grid.cvs_[e]
        for a, b in zip(mine.profiles_ + [mine.full_], one.profiles_ + [one.full_]):
            assert type(a) is L0Profile and same_table(a, b) and a.solver_info_["q_all"] == b.solver_info_["q_all"]
        assert mine.size_scores_.tobytes() == one.size_scores_.tobytes()
        alphas = [r * float(np.var(y)) for r in (1e-3, 1e-2, 0.1)]
        assert mine.regularized_search(alphas).best_params_ == one.regularized_search(alphas).best_params_
    for a, prob in zip(tables_of(grid), ridge_tables()):  # ... and the tables are the brute force's
        compare_table_ridge(a, prob["table"], prob["X"], prob["y"], eta=prob["eta"])


# ---- 4. order and independence ---------------------------------------------------------------------------------------------------
def test_every_problem_is_its_own():
    from sparselm_amd.miqp import l1l0_profile, l1l0_profile_cv

    X, y, _ = design(False)
    problems = l1_tables()
    ranks = [tuple(search_rank(prob["X"], prob["y"])) for prob in problems[::3]]
    print(f"distinct search orders among the six row sets: {len(set(ranks))}")
    assert len(set(ranks)) >= 2  # the premise: one order for all would be wrong for some fold
    etas = l1_etas()
    grid = l1l0_profile_cv(X, y, etas=etas, cv=CV, max_groups=K, big_M=BIG_M, fit_intercept=True)
    assert_all_finished(grid, 18)
    bounds = []
    for b, (prof, prob) in enumerate(zip(tables_of(grid), problems)):
        single = l1l0_profile(X[prob["rows"]], y[prob["rows"]], eta=prob["eta"], max_groups=K, big_M=BIG_M, fit_intercept=True)
        mine, theirs = prof.solver_info_, single.solver_info_
        print(f"problem {b}: q_all {mine['q_all']:.12e} (single {theirs['q_all']:.12e}), nodes {mine['nodes']} ({theirs['nodes']}), "
              f"descents {mine['descents']} ({theirs['descents']})")
        # the l1 bound the cut used is this problem's own: below its lasso on all columns, and the single call's on the same rows
        assert abs(mine["q_all"] - theirs["q_all"]) <= OBJ_RTOL * abs(theirs["q_all"])
        assert mine["q_all"] <= prob["f_all"] * (1 - 1e-12) and mine["nodes"] >= 1 and mine["descents"] >= 1
        np.testing.assert_array_equal(prof.supports_[list(full_rows(prob))], single.supports_[list(full_rows(prob))])
        bounds.append(theirs["q_all"])
    gaps = np.diff(np.sort(bounds)) / np.abs(np.sort(bounds)[1:])
    assert (gaps >= 1e4 * OBJ_RTOL).all()  # (the premise: 18 different bounds -- a problem that read another's would show)
    # the etas reversed: the same tables, reversed
    back = l1l0_profile_cv(X, y, etas=etas[::-1], cv=CV, max_groups=K, big_M=BIG_M, fit_intercept=True)
    assert back.etas_.tolist() == list(etas[::-1])
    for e in range(3):
        a, b = grid.cvs_[e], back.cvs_[2 - e]
        for ta, tb in zip(a.profiles_ + [a.full_], b.profiles_ + [b.full_]):
            assert same_table(ta, tb) and ta.eta_ == tb.eta_ == etas[e]
        assert a.size_scores_.tobytes() == b.size_scores_.tobytes()


# ---- 5. below the ticket prefix --------------------------------------------------------------------------------------------------
def test_below_the_ticket_prefix():
    from sparselm_amd.miqp import l1l0_profile_cv

    X, y, etas, problems = deep_tables()
    assert len(problems) == 8
    for b, prob in enumerate(problems):  # the premises: well-posed, and the best supports reach beyond the 16-group prefix
        table, rows = prob["table"], prob["rows"]
        rank = search_rank(X[rows], y[rows])
        deep = [k for k in range(1, 5) if (rank[np.flatnonzero(table["actives"][k])] >= PREFIX).any()]
        print(f"problem {b}: supports {table['n_supports']}, gaps {table['gaps'][1:]}, kappas {table['kappas'][1:]}, deep sizes {deep}")
        # at 0.05 every best support of two groups or more holds a hidden pair, ranked beyond the prefix; at 0.3 the l1 weight is above
        # what a hidden column correlates with y and the best supports are decoys of the prefix: one launch holds both kinds
        assert table["n_supports"] == 6196 and deep == ([2, 3, 4] if b % 2 == 0 else [])
        assert (table["gaps"][1:] >= GAP_MIN).all() and (table["kappas"][1:] <= KAPPA_MAX).all()
    grid = l1l0_profile_cv(X, y, etas=etas, cv=CV3, max_groups=4, big_M=BIG_M)
    assert_all_finished(grid, 8)
    for b, (prof, prob) in enumerate(zip(tables_of(grid), problems)):
        print(f"--- problem {b}: nodes {prof.solver_info_['nodes']}, descents {prof.solver_info_['descents']}")
        compare_table(prof, prob["table"], X[prob["rows"]], y[prob["rows"]], prob["eta"], range(1, 5))
        assert (prof.intercepts_ == 0.0).all()


# ---- 6. starved budget -----------------------------------------------------------------------------------------------------------
def test_starved_budget_stops_every_problem_with_its_incumbents():
    from sparselm_amd.miqp import l1l0_profile_cv

    X, y, etas, problems = deep_tables()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        grid = l1l0_profile_cv(X, y, etas=etas, cv=CV3, max_groups=4, big_M=BIG_M, solver_options={"max_nodes": 1000})
    assert len([w for w in caught if issubclass(w.category, ConvergenceWarning)]) == 1
    info = grid.solver_info_
    assert info["launches"] == 1 and not info["proven_optimal"] and len(info["problems"]) == 8
    for b, (prof, prob) in enumerate(zip(tables_of(grid), problems)):
        print(f"problem {b}: {prof.solver_info_}")
        rows, table = prob["rows"], prob["table"]
        assert not prof.proven_optimal_ and prof.solver_info_["status"] == "node_budget" and prof.solver_info_["nodes"] >= 1000
        for k in np.flatnonzero(np.isfinite(prof.values_)):
            assert prof.supports_[k].sum() == k and np.count_nonzero(prof.coefs_[k]) <= k
            at_coef = objective_of_l1(X[rows], y[rows], prof.coefs_[k], k, eta=prob["eta"])
            assert abs(at_coef - prof.values_[k]) <= 1e-9 * max(abs(prof.values_[k]), np.finfo(float).tiny)
            assert prof.values_[k] >= table["values"][k] - OBJ_RTOL * abs(table["values"][k])  # an incumbent is never below the optimum
    assert all(not cv.solver_info_["proven_optimal"] for cv in grid.cvs_)


# ---- 7. alpha_min > 0 ------------------------------------------------------------------------------------------------------------
def test_pruned_tables_are_exact_from_alpha_min_up():
    from sparselm_amd.miqp import l1l0_profile_cv

    X, y, _ = design(False)
    problems = l1_tables()
    var = float(np.var(y))
    alpha_min = 1e-3 * var
    grid = l1l0_profile_cv(X, y, etas=l1_etas(), cv=CV, max_groups=K, big_M=BIG_M, fit_intercept=True, alpha_min=alpha_min)
    assert_all_finished(grid, 18)
    for b, (prof, prob) in enumerate(zip(tables_of(grid), problems)):
        table, Xp, yp = prob["table"], prob["X"], prob["y"]
        assert prof.alpha_min_ == alpha_min
        sizes = []
        for alpha in (alpha_min, 1e-2 * var, 0.05 * var, 0.2 * var):
            k = regularized_of(table, alpha)
            obj = table["values"] + alpha * np.arange(K + 1)
            # the premise: the optimum over the supports of at most K groups is the best of size k, separated from the runner-up
            # of its size (the table's gap) and from every other size
            assert table["gaps"][k] >= GAP_MIN or k == 0
            assert (np.delete(obj, k).min() - obj[k]) >= GAP_MIN * max(abs(obj[k]), np.finfo(float).tiny) and table["kappas"][k] <= KAPPA_MAX
            coef, intercept, active = prof.regularized(alpha)
            sizes.append(int(active.sum()))
            np.testing.assert_array_equal(active, table["actives"][k])
            assert abs(prof.values_[k] - table["values"][k]) <= OBJ_RTOL * abs(table["values"][k]) or k == 0
            assert abs(objective_of_l1(Xp, yp, coef, k, alpha=alpha, eta=prob["eta"]) - obj[k]) <= OBJ_RTOL * max(abs(obj[k]), np.finfo(float).tiny)
            if k:
                assert np.max(np.abs(coef - table["coefs"][k])) <= COEF_RTOL * np.max(np.abs(table["coefs"][k]))
        print(f"problem {b}: sizes along the alphas {sizes}, nodes {prof.solver_info_['nodes']}")
        assert len(set(sizes)) >= 2
    with pytest.raises(ValueError, match="alpha_min"):
        grid.search([0.999 * alpha_min, 1e-2 * var])
    assert grid.search([alpha_min, 1e-2 * var]).best_params_["alpha"] in (alpha_min, 1e-2 * var)


# ---- 8. against today's route ----------------------------------------------------------------------------------------------------
REL_ALPHAS = (2e-3, 1e-2, 0.03, 0.05)  # times var y: from 0.1 var y on some fold is best left empty, at 1e-3 var y some optimum has 6 groups


def check_against_grid_search(mine, theirs, grid, X, alphas, etas):
    assert mine.best_params_ == theirs.best_params_ and mine.best_index_ == theirs.best_index_
    assert mine.cv_results_["params"] == list(ParameterGrid({"alpha": alphas, "eta": list(etas)})) == list(theirs.cv_results_["params"])
    row_norm = float(np.max(np.sum(np.abs(X), axis=1)))
    for i, params in enumerate(mine.cv_results_["params"]):
        e = list(etas).index(params["eta"])
        for f in range(len(grid.splits_)):
            coef = grid.cvs_[e].profiles_[f].regularized(params["alpha"])[0]
            top = float(np.max(np.abs(coef)))
            assert top > 0.0  # (the premise asserted on the reference: no cell is the empty model)
            # predictions move by at most ||x_i||_1 ||coef - coef'||_inf, and a root mean square by no more than its terms
            a, b = mine.cv_results_[f"split{f}_test_score"][i], theirs.cv_results_[f"split{f}_test_score"][i]
            assert abs(a - b) <= COEF_RTOL * row_norm * top, (f, params, a, b)
    best = theirs.best_estimator_
    np.testing.assert_array_equal(mine.active_groups_, best.active_groups_)
    assert np.max(np.abs(mine.coef_ - best.coef_)) <= COEF_RTOL * np.max(np.abs(best.coef_))
    assert abs(mine.best_score_ - theirs.best_score_) <= COEF_RTOL * row_norm * float(np.max(np.abs(best.coef_)))


@pytest.mark.parametrize("method", ["max_score", "one_std_score"])
def test_search_is_the_grid_search_fit_by_fit(method):
    from sparselm_amd.miqp import L1L0, l1l0_profile_cv
    from sparselm_amd.model_selection import GridSearchCV

    X, y, _ = design(False)
    problems = l1_tables()
    etas = l1_etas()
    alphas = [r * float(np.var(y)) for r in REL_ALPHAS]
    for b, prob in enumerate(problems):  # the premise: every (problem, alpha, eta) optimum is separated, not empty, and of at most K groups
        table = prob["table"]
        for alpha in alphas:
            obj = table["values"] + alpha * np.arange(K + 1)
            k = int(np.argmin(obj))
            assert k >= 1 and (np.delete(obj, k).min() - obj[k]) >= GAP_MIN * abs(obj[k]) and table["gaps"][k] >= GAP_MIN
            # L1L0 has no bound on the size: a support of more than K groups is worth at least f(all columns) + alpha (K + 1)
            assert prob["f_all"] + alpha * (K + 1) - obj[k] >= GAP_MIN * abs(obj[k])
    grid = l1l0_profile_cv(X, y, etas=etas, cv=CV, max_groups=K, big_M=BIG_M, fit_intercept=True)
    assert_all_finished(grid, 18)
    mine = grid.search(alphas, opt_selection_method=method)
    theirs = GridSearchCV(L1L0(fit_intercept=True, big_M=BIG_M), {"alpha": alphas, "eta": list(etas)}, cv=CV, opt_selection_method=method).fit(X, y)
    print(f"{method}: mean scores {mine.cv_results_['mean_test_score']}, best {mine.best_params_}")
    check_against_grid_search(mine, theirs, grid, X, alphas, etas)


def test_ridge_search_is_the_grid_search_fit_by_fit():
    from sparselm_amd.miqp import L2L0, l2l0_profile_cv
    from sparselm_amd.model_selection import GridSearchCV

    X, y, _ = design(False)
    etas = ridge_etas()
    alphas = [r * float(np.var(y)) for r in REL_ALPHAS]
    for prob in ridge_tables():  # the premise: every (problem, alpha, eta) optimum is separated and not empty
        table = prob["table"]
        for alpha in alphas:
            obj = table["values"] + alpha * np.arange(13)
            k = int(np.argmin(obj))
            assert k >= 1 and (np.delete(obj, k).min() - obj[k]) >= GAP_MIN * abs(obj[k]) and table["gaps"][k] >= GAP_MIN
            assert table["kappas"][k] <= KAPPA_MAX
    grid = l2l0_profile_cv(X, y, etas=etas, cv=CV, big_M=BIG_M, fit_intercept=True)
    assert_all_finished(grid, 18, l1=False)
    mine = grid.search(alphas)
    theirs = GridSearchCV(L2L0(fit_intercept=True, big_M=BIG_M), {"alpha": alphas, "eta": list(etas)}, cv=CV).fit(X, y)
    print(f"ridge: mean scores {mine.cv_results_['mean_test_score']}, best {mine.best_params_}")
    check_against_grid_search(mine, theirs, grid, X, alphas, etas)


# ---- 9. refusals by both routes --------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_by_both_routes():
    from sparselm_amd import _engine
    from sparselm_amd import distributed as D

    if _engine.load_binding() is None:
        pytest.fail("the compiled binding is not built")
    X, y, _ = single_design(0)
    wide = np.random.default_rng(0).standard_normal((80, 66))
    with _engine.get_engine().dataset(X, y) as ds, _engine.get_engine().dataset(wide, wide[:, 0]) as ds66:
        for route in (False, True):
            with pytest.raises(ValueError, match="n_eta"):
                ds.solve_l0_profile_grid([None], [0], [], eta_kind=1, max_groups=2, binding=route)
            with pytest.raises(ValueError, match=r"etas\[1\]"):
                ds.solve_l0_profile_grid([None], [0], [0.1, -0.1], eta_kind=1, max_groups=2, binding=route)
            with pytest.raises(ValueError, match=r"etas\[0\]"):
                ds.solve_l0_profile_grid([None], [0], [np.nan], eta_kind=0, max_groups=2, binding=route)
            with pytest.raises(ValueError, match="eta_kind"):
                ds.solve_l0_profile_grid([None], [0], [0.1], eta_kind=2, max_groups=2, binding=route)
            with pytest.raises(ValueError, match="T goes with the ridge"):
                ds.solve_l0_profile_grid([None], [0], [0.1], eta_kind=1, T=np.eye(12), max_groups=2, binding=route)
            with pytest.raises(ValueError, match="at most 128 problems"):  # 3 x 43 = 129
                ds.solve_l0_profile_grid([None] * 3, [0] * 3, np.full(43, 0.1), eta_kind=1, max_groups=1, binding=route)
            with pytest.raises(ValueError, match="count"):
                ds.solve_l0_profile_grid([None] * 17, [0] * 17, [0.1], eta_kind=1, max_groups=1, binding=route)
            with pytest.raises(ValueError, match="count"):
                ds.solve_l0_profile_grid([], [], [0.1], eta_kind=0, max_groups=1, binding=route)
            with pytest.raises(ValueError, match="need"):  # what the entries it generalises refuse
                ds.solve_l0_profile_grid([None], [0], [0.1], eta_kind=1, need=[1 << 12] + [0] * 11, binding=route)
            with pytest.raises(ValueError, match="alpha_min"):
                ds.solve_l0_profile_grid([None], [0], [0.1], eta_kind=0, alpha_min=-1.0, binding=route)
            with pytest.raises(NotImplementedError, match="64"):  # 66 columns: 65 search columns even with an intercept
                ds66.solve_l0_profile_grid([None], [0], [0.1], eta_kind=1, intercept=True, max_groups=1, binding=route)
            with pytest.raises(ValueError, match="count"):  # the batched entry keeps its own limit
                ds.solve_l0_profile_batch([None] * 17, [0] * 17, max_groups=1, binding=route)
            # ... and the cap itself is in: 16 x 8 = 128 problems of one size each
            out = ds.solve_l0_profile_grid([None] * 16, [0] * 16, np.linspace(0.1, 0.8, 8), eta_kind=0, max_groups=1, big_M=1000.0, binding=route)
            assert out[3].shape == (128, 2) and all(info["proven_optimal"] for info in out[4])
            assert all(np.array_equal(out[3][b], out[3][b % 8]) for b in range(128))  # (sixteen times the same row set)
    eng = _engine.Engine(0)
    try:
        D.init_row_sharding(eng, rank=0, world_size=1)
        with eng.dataset(X, y) as ds:
            ds.set_global_rows(len(y))
            for route in (False, True):
                with pytest.raises(NotImplementedError, match="row-sharded"):
                    ds.solve_l0_profile_grid([None], [0], [0.1], eta_kind=1, max_groups=3, binding=route)
    finally:
        eng.comm_destroy()
        eng.close()
