"""The exact l0 profile on the GPU (``sparselm_amd.miqp.l0_profile``, ``slm_solve_l0_profile``, the PROFILE instantiation of
csrc/l0_kernels.hpp) against the per-size brute force of tests/_l0_profile_reference.py and against the estimators one by one.

Tolerances and the well-posedness premise are those of tests/test_l0_gpu.py, per size: the reference's best-to-second gap of
that size is >= 1e-6 and the condition number of its winner's block <= 1e4 -- asserted on the reference's numbers first --
and then identical supports, objectives to 1e-10, coefficients to 1e-9.  No size is skipped.

Designs (checked on the CPU, tests/test_l0_profile_cpu.py for the first): ``make_regression(40, 12, n_informative=5,
noise=30.0)`` and the same at 40 x 24 in 12 groups of 2, centred, seeds 0 and 1 -- every size 1 .. 11 has a gap >= 3e-5 and
the values fall strictly; with ``noise=5.0`` the 40 x 12 design falls under 1e-6 at one size.  Below the ticket prefix the
suppressor-pair designs of tests/test_l0_search_gpu.py, imported."""

import functools

import numpy as np
import pytest
from sklearn.datasets import make_regression
from sklearn.exceptions import ConvergenceWarning

from _l0_profile_reference import envelope_sizes, profile_table, regularized_of
from _l0_reference import brute_force, objective_of, search_rank, solve_support
from test_l0_gpu import COEF_RTOL, GAP_MIN, KAPPA_MAX, OBJ_RTOL
from test_l0_search_gpu import HIER, PREFIX, THREES, suppressor

pytestmark = pytest.mark.gpu


# ---- designs and references, computed once -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def design(seed, grouped=False, n=40, noise=30.0):
    X, y = make_regression(n, 24 if grouped else 12, n_informative=5, noise=noise, random_state=seed)
    X, y = X - X.mean(axis=0), y - y.mean()
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y, (np.repeat(np.arange(12), 2) if grouped else None)


@functools.lru_cache(maxsize=None)
def design_table(seed, grouped=False, eta=0.0, tikhonov=False, big_M=np.inf, K=None):
    X, y, groups = design(seed, grouped)
    return profile_table(X, y, groups=groups, K=K, eta=eta, W=tikhonov_w() if tikhonov else None, big_M=big_M)


@functools.lru_cache(maxsize=None)
def tikhonov_w():
    W = np.eye(12) + 0.3 * np.random.default_rng(1).standard_normal((12, 12))
    W.setflags(write=False)
    return W


def compare_table(prof, table, X, y, eta=0.0, W=None, singular=False, sizes=None):
    """Per size: the premise on the reference, then support, value (the table's and the one recomputed from X at the
    coefficients), coefficients -- or, for designs whose blocks are singular by construction, fitted values."""
    K = len(table["values"]) - 1
    assert prof.values_.shape == (K + 1,) and prof.supports_.shape == table["actives"].shape and prof.coefs_.shape == table["coefs"].shape
    assert prof.values_[0] == 0.0 and not prof.supports_[0].any() and not prof.coefs_[0].any()
    for k in range(1, K + 1) if sizes is None else sizes:
        ref_v = table["values"][k]
        print(f"size {k}: reference value {ref_v:.12e} gap {table['gaps'][k]:.3e} kappa {table['kappas'][k]:.3e}; engine {prof.values_[k]:.12e}")
        if not np.isfinite(ref_v):  # the hierarchy admits no support of this size
            assert np.isinf(prof.values_[k]) and not prof.supports_[k].any() and not prof.coefs_[k].any()
            continue
        assert table["gaps"][k] >= GAP_MIN and (singular or table["kappas"][k] <= KAPPA_MAX)
        np.testing.assert_array_equal(prof.supports_[k], table["actives"][k])
        assert prof.supports_[k].sum() == k
        assert abs(prof.values_[k] - ref_v) <= OBJ_RTOL * abs(ref_v)
        assert abs(objective_of(X, y, prof.coefs_[k], k, eta=eta, W=W) - ref_v) <= OBJ_RTOL * abs(ref_v)
        if singular:
            fit_ref = X @ table["coefs"][k]
            assert np.max(np.abs(X @ prof.coefs_[k] - fit_ref)) <= COEF_RTOL * np.max(np.abs(fit_ref)) and np.isfinite(prof.coefs_[k]).all()
        else:
            err = np.max(np.abs(prof.coefs_[k] - table["coefs"][k])) / np.max(np.abs(table["coefs"][k]))
            assert err <= COEF_RTOL, (k, err)


def assert_finished(prof):
    info = prof.solver_info_
    assert prof.proven_optimal_ and info["proven_optimal"] and info["status"] == "optimal" and info["launches"] == 1


# ---- 1. the table against enumeration: 12 groups, every ticket one support ---------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("seed", [0, 1])
def test_table_equals_enumeration(seed, grouped):
    from sparselm_amd.miqp import l0_profile

    X, y, groups = design(seed, grouped)
    table = design_table(seed, grouped)
    assert (table["gaps"][1:12] >= 3e-5).all() and (np.diff(table["values"]) < 0).all()  # the premise, every size
    prof = l0_profile(X, y, groups=groups, max_groups=12, big_M=1000)
    assert_finished(prof)
    compare_table(prof, table, X, y)
    assert prof.alpha_min_ == 0.0 and (prof.intercepts_ == 0.0).all()
    r_all = X @ np.linalg.lstsq(X, y, rcond=None)[0] - y
    assert abs(prof.solver_info_["q_all"] - float(r_all @ r_all - y @ y) / 80) <= OBJ_RTOL * abs(prof.solver_info_["q_all"])


# ---- 2. against the estimators, one by one -------------------------------------------------------------------------------------
def test_best_subset_at_every_bound_is_the_estimator():
    from sparselm_amd.miqp import l0_profile
    from sparselm_amd.model import BestSubsetSelection

    X, y, _ = design(0)
    table = design_table(0)
    assert (table["gaps"][1:12] >= GAP_MIN).all() and (np.diff(table["values"]) < 0).all()
    prof = l0_profile(X, y, max_groups=12, big_M=1000)
    assert_finished(prof)
    for bound in range(1, 13):
        est = BestSubsetSelection(sparse_bound=bound, big_M=1000).fit(X, y)
        coef, intercept, active = prof.best_subset(bound)
        np.testing.assert_array_equal(active, est.active_groups_)
        assert active.sum() == bound and np.array_equal(coef, est.coef_) and intercept == est.intercept_ == 0.0
        assert prof.values_[bound] == est.solver_info_["objective"]


@pytest.mark.parametrize("eta", [1e-2, 1.0])
def test_ridged_best_subset_at_every_bound_is_the_estimator(eta):
    from sparselm_amd.miqp import l0_profile
    from sparselm_amd.model import RidgedBestSubsetSelection

    X, y, _ = design(0)
    W = tikhonov_w()
    table = design_table(0, eta=eta, tikhonov=True)
    assert (table["gaps"][1:12] >= GAP_MIN).all() and (np.diff(table["values"]) < 0).all() and (table["kappas"] <= KAPPA_MAX).all()
    prof = l0_profile(X, y, max_groups=12, eta=eta, tikhonov_w=W, big_M=1000)
    assert_finished(prof)
    compare_table(prof, table, X, y, eta=eta, W=W)
    for bound in range(1, 13):
        est = RidgedBestSubsetSelection(sparse_bound=bound, eta=eta, tikhonov_w=W, big_M=1000).fit(X, y)
        coef, _, active = prof.best_subset(bound)
        np.testing.assert_array_equal(active, est.active_groups_)
        assert active.sum() == bound and np.array_equal(coef, est.coef_)


@pytest.mark.parametrize("rel_alpha", [1e-4, 1e-2, 0.2])
def test_regularized_is_the_estimator(rel_alpha):
    from sparselm_amd.miqp import l0_profile
    from sparselm_amd.model import L2L0, RegularizedL0

    X, y, _ = design(0)
    alpha = rel_alpha * float(np.var(y))
    W = tikhonov_w()
    for eta in (0.0, 1e-2):
        table = design_table(0, eta=eta, tikhonov=eta > 0)
        # the premise: the regularised optimum is separated from the runner-up over ALL supports
        ref = brute_force(X, y, alpha=alpha, eta=eta, W=W if eta else None)
        assert ref["gap"] >= GAP_MIN and ref["kappa"] <= KAPPA_MAX and ref["active"].sum() == regularized_of(table, alpha)
        prof = l0_profile(X, y, eta=eta, tikhonov_w=W if eta else None, big_M=1000)
        est = (L2L0(alpha=alpha, eta=eta, tikhonov_w=W, big_M=1000) if eta else RegularizedL0(alpha=alpha, big_M=1000)).fit(X, y)
        coef, _, active = prof.regularized(alpha)
        print(f"alpha {alpha:.4e} eta {eta}: size {active.sum()}")
        np.testing.assert_array_equal(active, est.active_groups_)
        np.testing.assert_array_equal(active, ref["active"])
        assert np.array_equal(coef, est.coef_)
        assert abs(prof.values_[active.sum()] + alpha * active.sum() - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])


# ---- 3. below the ticket prefix ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deep_case(name):
    """(X, y, groups, hierarchy, K) of the three cases below the prefix, and their reference table."""
    hierarchy = None
    if name == "singles":
        X, y, groups, _, _ = suppressor(20)
        K = 4
    elif name == "hierarchy":
        # rank 16 (deep, in the free optimum of size 4) needs rank 0 (prefix, not in it); rank 2 needs rank 19 (a prefix group that
        # needs a deep one); rank 18 needs rank 19 (both deep, the later one needed by the earlier)
        X, y, groups, _, _ = suppressor(HIER["ng"], **HIER["design"])
        K = 4
        at = np.argsort(search_rank(X, y))
        hierarchy = [[] for _ in range(HIER["ng"])]
        hierarchy[at[16]] = [int(at[0])]
        hierarchy[at[2]] = [int(at[19])]
        hierarchy[at[18]] = [int(at[19])]
    else:  # groups of three columns
        X, y, groups, _, _ = suppressor(THREES["ng"], **THREES["design"])
        K = 3
    table = profile_table(X, y, groups=groups, K=K, big_M=1000, hierarchy=hierarchy)
    if hierarchy is not None:  # the premise of that case: the hierarchy changed the table
        free = profile_table(X, y, groups=groups, K=K, big_M=1000)
        assert any(not np.array_equal(free["actives"][k], table["actives"][k]) for k in range(1, K + 1))
    return X, y, groups, hierarchy, K, table


@pytest.mark.parametrize("name", ["singles", "hierarchy", "threes"])
def test_table_below_the_ticket_prefix(name):
    from sparselm_amd.miqp import l0_profile

    X, y, groups, hierarchy, K, table = deep_case(name)
    rank = search_rank(X, y, groups=groups)
    deep = [k for k in range(1, K + 1) if (rank[np.flatnonzero(table["actives"][k])] >= PREFIX).any()]
    print(f"supports {table['n_supports']}; sizes whose best support holds a group of rank >= {PREFIX}: {deep}")
    assert deep and table["n_supports"] <= 60000  # the premise: only the depth-first search proper reaches those
    prof = l0_profile(X, y, groups=groups, max_groups=K, hierarchy=hierarchy, big_M=1000)
    assert_finished(prof)
    compare_table(prof, table, X, y)
    if hierarchy is not None:
        for k in range(1, K + 1):
            for i in np.flatnonzero(prof.supports_[k]):
                assert all(prof.supports_[k][q] for q in hierarchy[i])


# ---- 4. alpha_min > 0 is exact where promised -------------------------------------------------------------------------------------
def test_pruned_table_is_exact_from_alpha_min_up():
    from sparselm_amd.miqp import l0_profile

    X, y, _ = design(0)
    n = len(y)
    var = float(np.var(y))
    alpha_min = 1e-3 * var
    top = 1.01 * float(y @ y) / (2 * n)  # above what any support gains: the optimum is empty
    prof = l0_profile(X, y, alpha_min=alpha_min, big_M=1000)
    full = l0_profile(X, y, big_M=1000)
    assert_finished(prof)
    print(f"nodes {prof.solver_info_['nodes']} at alpha_min, {full.solver_info_['nodes']} at 0")
    assert prof.alpha_min_ == alpha_min and prof.solver_info_["nodes"] <= full.solver_info_["nodes"]
    sizes = []
    for alpha in (alpha_min, 1e-2 * var, 0.05 * var, 0.2 * var, top):
        ref = brute_force(X, y, alpha=alpha, big_M=1000)
        assert ref["gap"] >= GAP_MIN and ref["kappa"] <= KAPPA_MAX
        coef, intercept, active = prof.regularized(alpha)
        k = int(active.sum())
        sizes.append(k)
        np.testing.assert_array_equal(active, ref["active"])
        assert abs(prof.values_[k] + alpha * k - ref["objective"]) <= OBJ_RTOL * max(abs(ref["objective"]), np.finfo(float).tiny)
        assert abs(objective_of(X, y, coef, k, alpha=alpha) - ref["objective"]) <= OBJ_RTOL * max(abs(ref["objective"]), np.finfo(float).tiny)
        if k:
            assert np.max(np.abs(coef - ref["coef"])) <= COEF_RTOL * np.max(np.abs(ref["coef"]))
            assert np.array_equal(coef, full.regularized(alpha)[0])  # the same support, the same host code
    print(f"sizes along the alphas: {sizes}")
    assert sizes[-1] == 0 and len(set(sizes)) >= 3
    with pytest.raises(ValueError, match="alpha_min"):
        prof.regularized(0.999 * alpha_min)
    with pytest.raises(ValueError, match="alpha_min"):
        prof.best_subset(3)


def greedy_values(X, y, K):
    """The values of the supports greedy forward selection passes through (single columns), by residual sum of squares."""
    chosen, out = [], [0.0]
    for _ in range(K):
        rss, j = min((solve_support(X, y, np.array(chosen + [j]))[1], j) for j in range(X.shape[1]) if j not in chosen)
        chosen.append(j)
        out.append((rss - float(y @ y)) / (2.0 * len(y)))
    return np.array(out)


def test_alpha_min_above_every_gain_cuts_at_the_root():
    from sparselm_amd.miqp import l0_profile

    X, y, _ = design(0)
    alpha_min = 1.01 * float(y @ y) / (2 * len(y))
    prof = l0_profile(X, y, alpha_min=alpha_min, big_M=1000)
    assert_finished(prof)
    assert prof.solver_info_["nodes"] == 0  # q_all + alpha_min >= 0 = E(0): deterministic
    # the table's only finite entries are the seeds: the supports of the greedy selection
    seeds = greedy_values(X, y, 12)
    assert np.isfinite(prof.values_).all() and np.max(np.abs(prof.values_ - seeds)) <= OBJ_RTOL * np.max(np.abs(seeds))
    coef, intercept, active = prof.regularized(alpha_min)
    assert not active.any() and not coef.any() and intercept == 0.0


# ---- 5. the cases the estimators are tested on ------------------------------------------------------------------------------------
def test_binding_box():
    from sparselm_amd.miqp import l0_profile

    X, y, _ = design(0)
    K = 6
    free = design_table(0)
    big_M = 0.6 * float(np.max(np.abs(free["coefs"][5])))
    table = design_table(0, big_M=big_M, K=K)
    bound = [k for k in range(1, K + 1) if np.isclose(np.max(np.abs(table["coefs"][k])), big_M, rtol=1e-9, atol=0)]
    print(f"big_M {big_M:.4f}; sizes whose winner sits on the box: {bound}")
    assert 5 in bound and any(table["values"][k] > free["values"][k] * (1 - 1e-6) for k in bound)  # it binds
    prof = l0_profile(X, y, max_groups=K, big_M=big_M)
    assert_finished(prof)
    compare_table(prof, table, X, y)
    assert np.max(np.abs(prof.coefs_)) <= big_M


def test_duplicated_column():
    """Column 5 is a copy of column 3: supports tie exactly, so only what is unique is compared -- every size's value -- and
    no row holds both copies with a non-zero coefficient."""
    from sparselm_amd.miqp import l0_profile

    X, y = make_regression(20, 8, n_informative=4, noise=1.0, random_state=1)
    X[:, 5] = X[:, 3]
    table = profile_table(X, y, K=4, big_M=1000)
    prof = l0_profile(X, y, max_groups=4, big_M=1000)
    assert_finished(prof)
    for k in range(1, 5):
        print(f"size {k}: reference {table['values'][k]:.12e}, engine {prof.values_[k]:.12e}")
        assert abs(prof.values_[k] - table["values"][k]) <= OBJ_RTOL * abs(table["values"][k])
        assert abs(objective_of(X, y, prof.coefs_[k], k) - table["values"][k]) <= OBJ_RTOL * abs(table["values"][k])
        assert prof.supports_[k].sum() == k and not (prof.coefs_[k][3] != 0 and prof.coefs_[k][5] != 0)


def test_centred_one_hot_group():
    from sparselm_amd.miqp import l0_profile

    rng = np.random.default_rng(12)
    level = rng.integers(0, 3, 36)
    Z = rng.standard_normal((36, 3))
    X = np.column_stack([np.eye(3)[level], Z])
    y = np.array([4.0, -2.0, 1.0])[level] + 0.5 * Z[:, 1] + 0.1 * rng.standard_normal(36)
    groups = np.array([7, 7, 7, 1, 2, 3])
    Xp, yp = X - X.mean(axis=0), y - y.mean()
    table = profile_table(Xp, yp, groups=groups, K=3, big_M=1000)
    prof = l0_profile(X, y, groups=groups, max_groups=3, big_M=1000, fit_intercept=True)
    assert_finished(prof)
    compare_table(prof, table, Xp, yp, singular=True)
    assert prof.supports_[1][-1] and prof.supports_[2][-1]  # (label 7 sorts last: the levels carry the signal)
    for k in range(4):
        np.testing.assert_allclose(X @ prof.coefs_[k] + prof.intercepts_[k], Xp @ table["coefs"][k] + y.mean(), rtol=0, atol=1e-8)


def test_fewer_rows_than_columns():
    from sparselm_amd.miqp import l0_profile

    X, y = make_regression(10, 12, n_informative=5, noise=30.0, random_state=0)
    K = 5
    table = profile_table(X, y, K=K, big_M=1000)
    prof = l0_profile(X, y, max_groups=K, big_M=1000)
    assert_finished(prof)
    compare_table(prof, table, X, y)


def test_intercept_and_sample_weight():
    from sparselm_amd.miqp import l0_profile
    from sparselm_amd.model import BestSubsetSelection

    X, y, _ = design(0)
    X, y = X + 3.0, y + 10.0
    w = np.random.default_rng(5).uniform(0.5, 2.0, 40)
    K = 4
    prof = l0_profile(X, y, max_groups=K, big_M=1000, fit_intercept=True, sample_weight=w)
    assert_finished(prof)
    wn = w * (40 / w.sum())
    xm, ym = np.average(X, axis=0, weights=wn), np.average(y, weights=wn)
    Xp, yp = (X - xm) * np.sqrt(wn)[:, None], (y - ym) * np.sqrt(wn)
    table = profile_table(Xp, yp, K=K, big_M=1000)
    compare_table(prof, table, Xp, yp)
    for k in range(K + 1):
        assert abs(prof.intercepts_[k] - (ym - xm @ table["coefs"][k])) <= 1e-9 * max(1.0, abs(ym))
    est = BestSubsetSelection(sparse_bound=3, big_M=1000, fit_intercept=True).fit(X, y, sample_weight=w)
    coef, intercept, active = prof.best_subset(3)
    assert np.array_equal(coef, est.coef_) and intercept == est.intercept_ and np.array_equal(active, est.active_groups_)


# ---- 6. the node budget ---------------------------------------------------------------------------------------------------------
def test_exhausted_budget_keeps_the_incumbents():
    from sparselm_amd.miqp import l0_profile

    X, y = make_regression(25, 30, n_informative=10, noise=1.0, random_state=0)
    K = 15
    with pytest.warns(ConvergenceWarning):
        prof = l0_profile(X, y, max_groups=K, big_M=1000, solver_options={"max_nodes": 1000})
    info = prof.solver_info_
    print(info)
    assert not prof.proven_optimal_ and not info["proven_optimal"] and info["status"] == "node_budget" and info["nodes"] >= 1000
    seeds = greedy_values(X, y, K)
    assert np.isfinite(prof.values_).all()  # every size has its seed at the least
    for k in range(K + 1):
        assert prof.supports_[k].sum() == k and np.count_nonzero(prof.coefs_[k]) <= k
        at_coef = objective_of(X, y, prof.coefs_[k], k)
        assert abs(at_coef - prof.values_[k]) <= 1e-9 * max(abs(prof.values_[k]), np.finfo(float).tiny)
        assert prof.values_[k] <= seeds[k] + 1e-9 * abs(seeds[k])


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
def test_65_columns_are_refused_by_the_engine():
    from sparselm_amd.miqp import l0_profile

    X, y = make_regression(80, 65, n_informative=5, random_state=2)
    with pytest.raises(NotImplementedError, match="64"):
        l0_profile(X, y, max_groups=1)


def test_row_sharded_dataset_is_refused():
    from sparselm_amd import _engine
    from sparselm_amd import distributed as D

    X, y, _ = design(0)
    eng = _engine.Engine(0)
    try:
        D.init_row_sharding(eng, rank=0, world_size=1)
        with eng.dataset(X, y) as ds:
            ds.set_global_rows(len(y))
            with pytest.raises(NotImplementedError, match="row-sharded"):
                ds.solve_l0_profile(max_groups=3)
    finally:
        eng.comm_destroy()
        eng.close()


def test_bad_arguments_are_refused_by_both_routes():
    from sparselm_amd import _engine

    if _engine.load_binding() is None:
        pytest.fail("the compiled binding is not built")
    X, y, _ = design(0)
    W = tikhonov_w()
    with _engine.get_engine().dataset(X, y) as ds:
        a = ds.solve_l0_profile(max_groups=5, eta=0.1, T=W.T @ W, big_M=50.0, binding=False)
        b = ds.solve_l0_profile(max_groups=5, eta=0.1, T=W.T @ W, big_M=50.0, binding=True)
        for route in (False, True):
            with pytest.raises(ValueError):
                ds.solve_l0_profile(alpha_min=-1.0, binding=route)
            with pytest.raises(ValueError):
                ds.solve_l0_profile(alpha_min=np.inf, binding=route)
            with pytest.raises(ValueError):
                ds.solve_l0_profile(need=[1 << 12] + [0] * 11, binding=route)
    for x, z in zip(a[:3], b[:3]):
        assert x.tobytes() == z.tobytes()
    assert {k: v for k, v in a[3].items() if k != "nodes"} == {k: v for k, v in b[3].items() if k != "nodes"}


# ---- 8. the regularisation path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True])
def test_alpha_breakpoints(grouped):
    from sparselm_amd.miqp import l0_profile

    X, y, groups = design(0, grouped)
    table = design_table(0, grouped)
    prof = l0_profile(X, y, groups=groups, big_M=1000)
    alphas, sizes = prof.alpha_breakpoints()
    print(f"breakpoints {alphas}, sizes {sizes}")
    assert len(sizes) == len(alphas) + 1 and (np.diff(alphas) < 0).all() and (alphas > 0).all()
    assert sizes.tolist() == envelope_sizes(table["values"]) and sizes[0] == 0 and len(sizes) >= 4
    edges = np.concatenate([[2.0 * alphas[0]], alphas, [0.0]])
    for i, size in enumerate(sizes):
        mid = 0.5 * (edges[i] + edges[i + 1])
        coef, _, active = prof.regularized(mid)
        assert active.sum() == size == regularized_of(table, mid)
        np.testing.assert_array_equal(active, table["actives"][size])
