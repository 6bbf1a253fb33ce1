"""The exclusion bound of the exact l0 search on the GPU (``solver_options={"bound": "exclusion"}``, ``slm_solve_l0_xb``,
``slm_solve_l0_xb_wide``; DESIGN 4d "Exclusion bound").

A subtree is cut against the value on every column the path has not excluded.  An overshooting bound would cut the optimum,
so the tests put the optimum where the path to it excludes the most: behind higher-scoring decoys, below the ticket prefix,
beyond the first mask word -- and compare with the brute force of ``_l0_reference`` (or, where that is impossible, with the
sequential restatement of ``_l0_bound_reference``, which takes q(all \\ E) straight from X).  Where both searches finish, the
bounded one returns the plain one's bits.
"""

import functools
import os
import re
import types
import warnings

import numpy as np
import pytest
from sklearn.datasets import make_regression

from _l0_bound_reference import bounded_search
from _l0_reference import brute_force, group_columns, objective_of, search_rank, solve_support
from test_l0_gpu import COEF_RTOL, GAP_MIN, KAPPA_MAX, OBJ_RTOL, assert_parents_active, compare, draw
from test_l0_search_gpu import HIER, PREFIX, THREES, assert_below_prefix, expected_nodes, hierarchy_ref, suppressor, suppressor_ref, winner_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
XB = {"bound": "exclusion"}
XB_WIDE = {"bound": "exclusion", "wide": True}
MAX_SUPPORTS = 60000
with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "l0_host.hpp")) as _fh:
    XCAP = int(re.search(r"constexpr int L0_XCAP = (\d+);", _fh.read()).group(1))  # rows of the exclusion factor


def assert_exclusion(info):
    assert info["bound"] == "exclusion" and 0.0 < info["bound_margin"] < 0.5 and "bound_reason" not in info


def namespace(beta, support, info, ng):
    """A dataset call's result in the shape ``compare`` takes."""
    return types.SimpleNamespace(coef_=beta, solver_info_=info, active_groups_=np.array([(support >> i) & 1 for i in range(ng)], dtype=bool))


def assert_same_result(a, b):
    """(beta, support, info) of two calls: the same bits."""
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2]["objective"] == b[2]["objective"]
    assert a[2]["proven_optimal"] and b[2]["proven_optimal"] and a[2]["lower_bound"] == b[2]["lower_bound"]


# ---- 1. the same bits as the plain search -----------------------------------------------------------------------------------
def twelve_column_calls(y):
    alpha = 1e-2 * float(np.var(y))
    W = np.random.default_rng(1).standard_normal((12, 12))
    need = [0] * 12
    need[3] = 1 << 0
    calls = (dict(max_groups=1), dict(max_groups=3), dict(max_groups=5), dict(alpha=alpha), dict(alpha=1e-4 * float(np.var(y))),
             dict(alpha=alpha, eta=0.1, T=W.T @ W), dict(max_groups=5, big_M=50.0), dict(max_groups=4, need=need))
    for kw in calls:
        kw.setdefault("big_M", 1000.0)
    return calls


def test_same_bits_as_the_plain_search():
    from sparselm_amd import _engine

    X, y = draw(40)
    plain_keys = None
    with _engine.get_engine().dataset(X, y) as ds:
        for kw in twelve_column_calls(y):
            plain = ds.solve_l0(**kw)
            plain_keys = set(plain[2])
            for name in ("solve_l0_xb", "solve_l0_xb_wide"):
                for route in (False, True):
                    got = getattr(ds, name)(binding=route, **kw)
                    print(f"{sorted(kw)} {name} binding={route}: objective {got[2]['objective']:.12e}, nodes {got[2]['nodes']} "
                          f"(plain {plain[2]['nodes']}), margin {got[2]['bound_margin']:.3e}")
                    assert_same_result(plain, got)
                    assert_exclusion(got[2])
                    assert got[2]["status"] == "optimal" and got[2]["launches"] == 1
        # the plain entries keep their keys
        assert "bound" not in plain_keys and "bound" not in ds.solve_l0_wide(max_groups=2)[2]
        for route in (False, True):
            with pytest.raises(ValueError):
                ds.solve_l0_xb(alpha=-1.0, binding=route)
            with pytest.raises(ValueError):
                ds.solve_l0_xb_wide(need=[1 << 12] + [0] * 11, binding=route)
    # ... and it is the optimum
    ref = brute_force(X, y, K=3, big_M=1000)
    with _engine.get_engine().dataset(X, y) as ds:
        compare(namespace(*ds.solve_l0_xb(max_groups=3, big_M=1000.0), 12), ref, X, y)


def test_fewer_rows_than_columns_fall_back_to_the_plain_bound():
    from sparselm_amd import _engine

    X, y = draw(10)  # n < p: the Gram is singular, there is no P
    with _engine.get_engine().dataset(X, y) as ds:
        for kw in twelve_column_calls(y):
            if kw.get("eta"):
                continue  # (a ridge term makes H definite: covered above)
            plain = ds.solve_l0(**kw)
            for name in ("solve_l0_xb", "solve_l0_xb_wide"):
                got = getattr(ds, name)(**kw)
                assert_same_result(plain, got)
                assert got[2]["bound"] == "q_all" and "positive definite" in got[2]["bound_reason"] and "bound_margin" not in got[2]
        # with a ridge term the same data takes the exclusion bound
        got = ds.solve_l0_xb(alpha=1e-2 * float(np.var(y)), eta=0.1, big_M=1000.0)
        assert_exclusion(got[2])
        assert_same_result(ds.solve_l0(alpha=1e-2 * float(np.var(y)), eta=0.1, big_M=1000.0), got)


# ---- 2. against the brute force below the ticket prefix ---------------------------------------------------------------------
@pytest.mark.parametrize("ng,K,design", [(17, 4, {}), (20, 4, {}), (24, 4, {}), (32, 3, dict(pairs=1, tau=0.3))])
def test_optimum_behind_the_decoys(ng, K, design):
    from sparselm_amd.model import BestSubsetSelection

    X, y, _, hidden, _ = suppressor(ng, **design)
    ref = suppressor_ref(ng, K, **design)
    assert set(hidden) <= set(np.flatnonzero(ref["active"]))
    assert_below_prefix(ref, search_rank(X, y), ng)
    est = BestSubsetSelection(sparse_bound=K, big_M=1000, solver_options=XB).fit(X, y)
    compare(est, ref, X, y)
    assert_exclusion(est.solver_info_)


@pytest.mark.parametrize("case", ["prefix_needs_deep", "deep_needs_excluded_prefix", "chain_of_three"])
def test_hierarchy_across_the_prefix(case):
    from sparselm_amd.model import BestSubsetSelection

    ng, K = HIER["ng"], HIER["K"]
    X, y, _, _, _ = suppressor(ng, **HIER["design"])
    rank = search_rank(X, y)
    at = np.argsort(rank)
    free = hierarchy_ref(None)
    won = set(np.flatnonzero(free["active"]))
    need = [[] for _ in range(ng)]
    if case == "prefix_needs_deep":
        need[next(j for j in at[:PREFIX] if j in won)] = [next(j for j in at[PREFIX:] if j not in won)]
    elif case == "deep_needs_excluded_prefix":
        need[next(j for j in at[PREFIX:] if j in won)] = [next(j for j in at[:PREFIX] if j not in won)]
    else:
        need[at[16]] = [at[18]]
        need[at[18]] = [at[19]]
    ref = hierarchy_ref(tuple(tuple(int(v) for v in row) for row in need))
    assert not np.array_equal(ref["active"], free["active"]) and ref["n_supports"] <= MAX_SUPPORTS
    assert np.count_nonzero(winner_ranks(ref, rank) >= PREFIX) >= 1
    est = BestSubsetSelection(sparse_bound=K, hierarchy=need, big_M=1000, solver_options=XB).fit(X, y)
    compare(est, ref, X, y)
    assert_parents_active(est.active_groups_, need, list(range(ng)))
    assert_exclusion(est.solver_info_)


@functools.lru_cache(maxsize=None)
def mixed_groups():
    """The 40-column suppressor design with its 36 decoys merged into groups of 1, 2 and 3 columns in turn (18 groups) and
    the four hidden columns left alone: 22 groups."""
    X, y, _, hidden, _ = suppressor(40)
    groups = np.full(40, -1)
    groups[hidden] = np.arange(4)
    decoys = [j for j in range(40) if j not in set(hidden)]
    g, at = 4, 0
    while at < len(decoys):
        width = 1 + (g - 4) % 3
        groups[decoys[at:at + width]] = g
        at += width
        g += 1
    return X, y, groups, np.arange(4)


def test_groups_of_one_to_three_columns():
    from sparselm_amd.model import BestSubsetSelection

    X, y, groups, hidden = mixed_groups()
    ng = len(np.unique(groups))
    assert ng == 22 and sorted(set(np.bincount(groups))) == [1, 2, 3]
    ref = brute_force(X, y, groups=groups, K=4, big_M=1000)
    assert set(hidden) <= set(np.flatnonzero(ref["active"]))
    assert_below_prefix(ref, search_rank(X, y, groups=groups), ng)
    est = BestSubsetSelection(groups=groups, sparse_bound=4, big_M=1000, solver_options=XB).fit(X, y)
    compare(est, ref, X, y)
    assert_exclusion(est.solver_info_)
    # ... and groups of three throughout
    X, y, groups, hidden, _ = suppressor(THREES["ng"], **THREES["design"])
    ref = suppressor_ref(THREES["ng"], THREES["K"], **THREES["design"])
    assert_below_prefix(ref, search_rank(X, y, groups=groups), THREES["ng"])
    est = BestSubsetSelection(groups=groups, sparse_bound=THREES["K"], big_M=1000, solver_options=XB).fit(X, y)
    compare(est, ref, X, y)


def test_a_binding_box_below_the_prefix():
    """The bound is on the unboxed value: the box only raises what lies below a node."""
    from sparselm_amd.model import BestSubsetSelection

    X, y, _, _, _ = suppressor(20)
    big_M = 0.6 * float(np.max(np.abs(suppressor_ref(20, 4)["coef"])))
    ref = suppressor_ref(20, 4, big_M=big_M)
    assert np.isclose(np.max(np.abs(ref["coef"])), big_M, rtol=1e-9, atol=0)  # it binds
    assert_below_prefix(ref, search_rank(X, y), 20)
    est = BestSubsetSelection(sparse_bound=4, big_M=big_M, solver_options=XB).fit(X, y)
    compare(est, ref, X, y)
    assert np.max(np.abs(est.coef_)) <= big_M


# ---- 3. node counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ng", [17, 20])
def test_fewer_nodes_where_only_the_cardinality_prunes(ng):
    """The design of ``test_every_support_is_visited_once``: alpha = 0 and q_all below every value the search can hold, so
    the plain search visits ``expected_nodes`` nodes exactly.  With three of ``ng`` columns allowed the value on everything
    not excluded rises above the incumbent long before the path ends."""
    from sparselm_amd.model import BestSubsetSelection

    K, n = 3, 60
    rng = np.random.default_rng(30 + ng)
    X = rng.standard_normal((n, ng))
    y = X @ rng.standard_normal(ng) + rng.standard_normal(n)
    ref = brute_force(X, y, K=K, big_M=1000)
    est = BestSubsetSelection(sparse_bound=K, big_M=1000, solver_options=XB).fit(X, y)
    compare(est, ref, X, y)
    assert_exclusion(est.solver_info_)
    nodes, plain = est.solver_info_["nodes"], expected_nodes(ng, K)
    print(f"nodes {nodes} with the exclusion bound, {plain} without: {plain / max(nodes, 1):.1f} times fewer")
    assert 0 < nodes < plain


# ---- 4. ill-conditioned designs ---------------------------------------------------------------------------------------------
def ar1(n, p, rho, seed):
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, p))
    X = np.empty((n, p))
    X[:, 0] = Z[:, 0]
    for j in range(1, p):
        X[:, j] = rho * X[:, j - 1] + np.sqrt(1 - rho * rho) * Z[:, j]
    return X, rng


def compare_ill_conditioned(est, ref, X, y, alpha=0.0):
    """Support and objective at the tolerances of ``compare``; the coefficients at COEF_RTOL times the winner's condition
    number over KAPPA_MAX where that is above one (both sides solve a block that ill-conditioned)."""
    info = est.solver_info_
    print(f"reference: gap {ref['gap']:.3e} kappa {ref['kappa']:.3e} objective {ref['objective']:.12e}; engine: objective "
          f"{info['objective']:.12e} nodes {info['nodes']} margin {info.get('bound_margin')}")
    assert ref["gap"] >= GAP_MIN
    assert info["proven_optimal"] and info["lower_bound"] == info["objective"]
    np.testing.assert_array_equal(est.active_groups_, ref["active"])
    assert abs(info["objective"] - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])
    at_coef = objective_of(X, y, est.coef_, int(est.active_groups_.sum()), alpha=alpha)
    assert abs(at_coef - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])
    err = np.max(np.abs(est.coef_ - ref["coef"])) / np.max(np.abs(ref["coef"]))
    assert err <= COEF_RTOL * max(1.0, ref["kappa"] / KAPPA_MAX)


def test_ar1_design():
    from sparselm_amd.model import BestSubsetSelection, RegularizedL0

    X, rng = ar1(40, 14, 0.99, 3)
    beta = np.zeros(14)
    beta[[2, 7, 11]] = [3.0, -2.0, 1.5]
    y = X @ beta + 0.1 * rng.standard_normal(40)
    est = BestSubsetSelection(sparse_bound=3, big_M=1000, solver_options=XB).fit(X, y)
    compare_ill_conditioned(est, brute_force(X, y, K=3, big_M=1000), X, y)
    assert_exclusion(est.solver_info_)
    alpha = 1e-3 * float(np.var(y))
    est = RegularizedL0(alpha=alpha, big_M=1000, solver_options=XB).fit(X, y)
    compare_ill_conditioned(est, brute_force(X, y, alpha=alpha, big_M=1000), X, y, alpha=alpha)
    assert_exclusion(est.solver_info_)


def test_two_columns_that_differ_by_1e_5():
    from sparselm_amd.model import BestSubsetSelection, RegularizedL0

    X, y, coef = make_regression(40, 10, n_informative=4, noise=1.0, random_state=3, coef=True)
    idle = np.flatnonzero(coef == 0.0)  # the twins carry no signal: the optimum is unique, the Gram next to singular
    X[:, idle[1]] = X[:, idle[0]] * (1.0 + 1e-5 * np.random.default_rng(0).standard_normal(40))
    kappa = np.linalg.cond(X.T @ X / 40)
    print(f"kappa of the Gram {kappa:.3e}")
    assert 1e8 < kappa < 1e13
    est = BestSubsetSelection(sparse_bound=3, big_M=1e6, solver_options=XB).fit(X, y)
    compare_ill_conditioned(est, brute_force(X, y, K=3, big_M=1e6), X, y)
    assert_exclusion(est.solver_info_)
    alpha = 1e-2 * float(np.var(y))
    est = RegularizedL0(alpha=alpha, big_M=1e6, solver_options=XB).fit(X, y)
    compare_ill_conditioned(est, brute_force(X, y, alpha=alpha, big_M=1e6), X, y, alpha=alpha)
    assert_exclusion(est.solver_info_)


def test_a_duplicated_column_falls_back():
    from sparselm_amd.model import BestSubsetSelection

    X, y = make_regression(20, 8, n_informative=4, noise=1.0, random_state=1)
    X[:, 5] = X[:, 3]
    est = BestSubsetSelection(sparse_bound=4, big_M=1000, solver_options=XB).fit(X, y)
    plain = BestSubsetSelection(sparse_bound=4, big_M=1000).fit(X, y)
    info = est.solver_info_
    assert info["bound"] == "q_all" and "positive definite" in info["bound_reason"] and "bound_margin" not in info
    assert info["proven_optimal"] and np.array_equal(est.coef_, plain.coef_) and info["objective"] == plain.solver_info_["objective"]
    assert "bound" not in plain.solver_info_
    ref = brute_force(X, y, K=4, big_M=1000)
    assert abs(info["objective"] - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])


# ---- 5. wide ----------------------------------------------------------------------------------------------------------------
def test_seventy_singletons():
    """Best subset K = 2 over 70 columns (2 486 supports).  The hidden pair sits at the last two search ranks: the path to it
    excludes 68 columns -- more than the exclusion factor has rows, and groups of the second state slot among them."""
    from sparselm_amd.model import BestSubsetSelection

    X, y, _, hidden, _ = suppressor(70, pairs=1, tau=0.3, n=100)
    ref = brute_force(X, y, K=2, big_M=1000)
    rank = search_rank(X, y)
    ranks = np.sort(rank[np.flatnonzero(ref["active"])])
    print(f"supports {ref['n_supports']}, winner's search ranks {ranks.tolist()}, L0_XCAP {XCAP}")
    assert ref["n_supports"] == 2486 and set(np.flatnonzero(ref["active"])) == set(hidden)
    assert ranks.min() >= 64 and ranks.min() > XCAP
    est = BestSubsetSelection(sparse_bound=2, big_M=1000, solver_options=XB_WIDE).fit(X, y)
    compare(est, ref, X, y)
    assert_exclusion(est.solver_info_)
    assert est.solver_info_["capacity_cut"] is None
    print(f"nodes {est.solver_info_['nodes']} (only the cardinality would leave {expected_nodes(70, 2)})")


@functools.lru_cache(maxsize=None)
def sixty_six_groups():
    """100 columns in 66 groups: the hidden pair of the 100-singleton design alone, its 98 decoys as 34 pairs and 30 singles."""
    X, y, _, hidden, _ = suppressor(100, pairs=1, tau=0.3, n=150)
    groups = np.full(100, -1)
    groups[hidden] = [0, 1]
    decoys = [j for j in range(100) if j not in set(hidden)]
    groups[decoys[:68]] = 2 + np.arange(68) // 2
    groups[decoys[68:]] = 36 + np.arange(30)
    return X, y, groups


def test_sixty_six_groups_with_a_hierarchy_in_the_high_word():
    from sparselm_amd.model import BestSubsetSelection

    X, y, groups = sixty_six_groups()
    assert len(np.unique(groups)) == 66
    rank = search_rank(X, y, groups=groups)
    at = np.argsort(rank)
    assert sorted(rank[[0, 1]]) == [64, 65]  # the hidden pair comes last
    need = [[] for _ in range(66)]
    need[at[65]] = [at[3]]  # the group of rank 65 needs the decoy of rank 3 ...
    need[at[3]] = [at[64]]  # ... which needs the group of rank 64: a bit of the high word
    ref = brute_force(X, y, groups=groups, K=3, big_M=1000, hierarchy=need)
    ranks = np.sort(rank[np.flatnonzero(ref["active"])])
    # (without the hierarchy the pair's best companion is another group: the hierarchy decides the third)
    _, gcols = group_columns(groups, 100)
    third = 2 + int(np.argmin([solve_support(X, y, np.concatenate([gcols[0], gcols[1], gcols[g]]))[1] for g in range(2, 66)]))
    print(f"supports {ref['n_supports']}, winner's ranks {ranks.tolist()}, the pair's best companion has rank {rank[third]}")
    assert ref["n_supports"] <= MAX_SUPPORTS and ranks.tolist() == [3, 64, 65] and rank[third] != 3
    est = BestSubsetSelection(groups=groups, sparse_bound=3, hierarchy=need, big_M=1000, solver_options=XB_WIDE).fit(X, y)
    compare(est, ref, X, y)
    assert_parents_active(est.active_groups_, need, list(range(66)))
    assert_exclusion(est.solver_info_)


# ---- 6. the reference's own data: 290 x 66 ----------------------------------------------------------------------------------
def test_reference_data_is_proven_optimal():
    """``L2L0`` at alpha = 1e-5, eta = 1.66e-6 on the reference's 290 x 66 example: proven under the default budget, and the
    restatement's support and objective (831 nodes there; the plain search exhausts 2^30 nodes at a smaller alpha,
    profiles/l0_wide.txt)."""
    from sparselm_amd.model import L2L0

    X = np.load(os.path.join(ROOT, "tests", "golden", "reference_examples", "corr.npy"))
    y = np.load(os.path.join(ROOT, "tests", "golden", "reference_examples", "energy.npy"))
    assert X.shape == (290, 66)
    alpha, eta = 1e-5, 1.66e-6
    est = L2L0(fit_intercept=True, alpha=alpha, eta=eta, solver_options=XB_WIDE).fit(X, y)
    info = est.solver_info_
    print(info, int(est.active_groups_.sum()))
    assert info["proven_optimal"] and info["status"] == "optimal" and info["lower_bound"] == info["objective"]
    assert_exclusion(info)
    Xc, yc = X - X.mean(axis=0), y - y.mean()
    ref = bounded_search(Xc, yc, alpha=alpha, eta=eta)
    print(f"restatement: objective {ref['objective']:.12e}, {int(ref['active'].sum())} columns, {ref['nodes']} nodes; engine {info['nodes']}")
    assert ref["finished"]
    np.testing.assert_array_equal(est.active_groups_, ref["active"])
    assert abs(info["objective"] - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])
    at_coef = objective_of(Xc, yc, est.coef_, int(est.active_groups_.sum()), alpha=alpha, eta=eta)
    assert abs(at_coef - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])
    assert np.max(np.abs(est.coef_ - ref["coef"])) <= COEF_RTOL * np.max(np.abs(ref["coef"]))


# ---- 7. the estimator path --------------------------------------------------------------------------------------------------
def test_intercept_sample_weight_clone_and_grid_search():
    from sklearn.base import clone
    from sklearn.model_selection import GridSearchCV

    from sparselm_amd.model import BestSubsetSelection, RidgedBestSubsetSelection

    X, y = draw(40)
    X = X + 3.0
    y = y + 10.0
    w = np.random.default_rng(5).uniform(0.5, 2.0, 40)
    est = clone(BestSubsetSelection(sparse_bound=3, big_M=1000, fit_intercept=True, solver_options=dict(XB))).fit(X, y, sample_weight=w)
    wn = w * (40 / w.sum())
    xm, ym = np.average(X, axis=0, weights=wn), np.average(y, weights=wn)
    Xp, yp = (X - xm) * np.sqrt(wn)[:, None], (y - ym) * np.sqrt(wn)
    ref = brute_force(Xp, yp, K=3, big_M=1000)
    compare(est, ref, Xp, yp)
    assert_exclusion(est.solver_info_)
    assert abs(est.intercept_ - (ym - xm @ ref["coef"])) <= 1e-9 * max(1.0, abs(ym))
    # a grid search carries the option to every candidate and fold, and gives the plain search's scores
    grid = {"sparse_bound": [2, 4]}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        a = GridSearchCV(BestSubsetSelection(big_M=1000, solver_options=dict(XB)), grid, cv=3).fit(X, y)
        b = GridSearchCV(BestSubsetSelection(big_M=1000), grid, cv=3).fit(X, y)
    assert a.best_params_ == b.best_params_ and np.array_equal(a.cv_results_["mean_test_score"], b.cv_results_["mean_test_score"])
    assert np.array_equal(a.best_estimator_.coef_, b.best_estimator_.coef_)
    assert_exclusion(a.best_estimator_.solver_info_)
    assert "bound" not in b.best_estimator_.solver_info_
    # a ridge term with a Tikhonov matrix
    W = np.random.default_rng(1).standard_normal((12, 12))
    Xd, yd = draw(40)
    est = RidgedBestSubsetSelection(sparse_bound=3, eta=0.1, tikhonov_w=W, big_M=1000, solver_options=XB).fit(Xd, yd)
    compare(est, brute_force(Xd, yd, K=3, eta=0.1, W=W, big_M=1000), Xd, yd, eta=0.1, W=W)
    assert_exclusion(est.solver_info_)
    # the plain bound by name: the default search, and the keys say so
    named = BestSubsetSelection(sparse_bound=3, big_M=1000, solver_options={"bound": "q_all"}).fit(Xd, yd)
    assert named.solver_info_["bound"] == "q_all" and np.array_equal(named.coef_, BestSubsetSelection(sparse_bound=3, big_M=1000).fit(Xd, yd).coef_)
