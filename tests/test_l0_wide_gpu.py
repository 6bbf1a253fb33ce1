"""The WIDE exact l0 search on the GPU (``slm_solve_l0_wide``, ``slm_solve_l0_profile_wide``, the WIDE instantiations of
csrc/l0_kernels.hpp; ``solver_options={"wide": True}``): up to 128 columns and 128 groups, supports of at most 64 independent
columns.

The references are the brute forces of tests/_l0_reference.py and tests/_l0_profile_reference.py; the designs are the
suppressor pairs of tests/test_l0_search_gpu.py (the optimum needs groups that rank LAST in the search order -- here beyond
rank 64, where the second state slot and the high mask word are at work).  Every test asserts its premises on the reference
first (gap >= GAP_MIN, kappa <= KAPPA_MAX, search ranks from ``search_rank``) and compares with ``compare`` of
tests/test_l0_gpu.py at its tolerances; every bounded call must come back proven optimal under the default budget.  Every
reference enumerates under 90 000 supports (asserted); they are computed once and shared."""

import functools
import os
import types
import warnings

import numpy as np
import pytest
from sklearn.datasets import make_regression
from sklearn.exceptions import ConvergenceWarning

from _l0_profile_reference import profile_table
from _l0_reference import brute_force, objective_of, search_rank
from test_l0_gpu import COEF_RTOL, GAP_MIN, KAPPA_MAX, OBJ_RTOL, assert_parents_active, compare, draw
from test_l0_search_gpu import expected_nodes, suppressor

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NARROW = 64  # L0_PMAX: the narrow search's columns and groups, a lane's worth of state, a mask word
MAX_SUPPORTS = 90000
WIDE = {"wide": True}


def namespace(beta, support, info, ng):
    """A dataset call's result in the shape ``compare`` takes."""
    return types.SimpleNamespace(coef_=beta, solver_info_=info, active_groups_=np.array([(support >> i) & 1 for i in range(ng)], dtype=bool))


def assert_same_result(a, b):
    """(beta, support, info) of two calls: the same bits."""
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2]["objective"] == b[2]["objective"]
    assert a[2]["proven_optimal"] and b[2]["proven_optimal"] and a[2]["lower_bound"] == b[2]["lower_bound"]


# ---- 1. the wide kernel on narrow problems: the same bits as the narrow one -------------------------------------------------
@pytest.mark.parametrize("n", [40, 10])
def test_wide_kernel_on_the_twelve_column_designs(n):
    from sparselm_amd import _engine

    X, y = draw(n)
    alpha = 1e-2 * float(np.var(y))
    W = np.random.default_rng(1).standard_normal((12, 12))
    need = [0] * 12
    need[3] = 1 << 0
    with _engine.get_engine().dataset(X, y) as ds:
        for kw in (dict(max_groups=1), dict(max_groups=3), dict(max_groups=5), dict(alpha=alpha), dict(alpha=1e-4 * float(np.var(y))),
                   dict(alpha=alpha, eta=0.1, T=W.T @ W), dict(max_groups=5, big_M=50.0), dict(max_groups=4, need=need)):
            kw.setdefault("big_M", 1000.0)
            narrow, wide = ds.solve_l0(**kw), ds.solve_l0_wide(**kw)
            print(f"{sorted(kw)}: objective {wide[2]['objective']:.12e}, nodes narrow {narrow[2]['nodes']} wide {wide[2]['nodes']}")
            assert_same_result(narrow, wide)
            assert wide[2]["status"] == "optimal" and wide[2]["capacity_cut"] is None and wide[2]["launches"] == 1
        # the two routes into the library
        a, b = ds.solve_l0_wide(alpha=alpha, need=need, binding=False), ds.solve_l0_wide(alpha=alpha, need=need, binding=True)
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1] and {k: v for k, v in a[2].items() if k != "nodes"} == {
            k: v for k, v in b[2].items() if k != "nodes"}
        for route in (False, True):
            with pytest.raises(ValueError):
                ds.solve_l0_wide(alpha=-1.0, binding=route)
            with pytest.raises(ValueError):
                ds.solve_l0_wide(need=[1 << 12] + [0] * 11, binding=route)  # a bit at the group count
            with pytest.raises(ValueError):
                ds.solve_l0_wide(need=[1 << 100] + [0] * 11, binding=route)  # ... and one in the high word
    # ... and it is the optimum
    ref = brute_force(X, y, K=3, big_M=1000)
    with _engine.get_engine().dataset(X, y) as ds:
        compare(namespace(*ds.solve_l0_wide(max_groups=3, big_M=1000.0), 12), ref, X, y)


def test_wide_kernel_on_grouped_columns():
    from sparselm_amd import _engine

    X, y = draw(40)
    gidx = np.array([2, 2, 0, 0, 0, 1, 1, 4, 3, 3, 3, 4])
    need = [1 << 4, 1 << 0, (1 << 0) | (1 << 4), 0, 1 << 3]  # (the group-level hierarchy of test_l0_gpu.py, as masks)
    alpha = 1e-2 * float(np.var(y))
    with _engine.get_engine().dataset(X, y) as ds:
        ds.set_groups(gidx, 5)
        for kw in (dict(max_groups=2), dict(alpha=alpha), dict(alpha=alpha, need=need)):
            assert_same_result(ds.solve_l0(big_M=1000.0, **kw), ds.solve_l0_wide(big_M=1000.0, **kw))


def test_wide_kernel_below_the_prefix():
    from sparselm_amd import _engine

    X, y, _, hidden, _ = suppressor(24)
    ref = brute_force(X, y, K=4, big_M=1000)
    rank = search_rank(X, y)
    assert ref["n_supports"] <= MAX_SUPPORTS and np.count_nonzero(rank[np.flatnonzero(ref["active"])] >= 16) >= 2
    with _engine.get_engine().dataset(X, y) as ds:
        narrow, wide = ds.solve_l0(max_groups=4, big_M=1000.0), ds.solve_l0_wide(max_groups=4, big_M=1000.0)
    assert_same_result(narrow, wide)
    compare(namespace(*wide, 24), ref, X, y)


def test_wide_profile_on_a_narrow_problem():
    from sparselm_amd import _engine

    X, y = make_regression(40, 12, n_informative=5, noise=30.0, random_state=0)
    X, y = X - X.mean(axis=0), y - y.mean()
    with _engine.get_engine().dataset(X, y) as ds:
        narrow = ds.solve_l0_profile(max_groups=12, big_M=1000.0)
        wide = ds.solve_l0_profile_wide(max_groups=12, big_M=1000.0)
        routes = [ds.solve_l0_profile_wide(max_groups=12, big_M=1000.0, binding=route) for route in (False, True)]
    assert narrow[3]["proven_optimal"] and wide[3]["proven_optimal"]
    for k in range(13):  # every size
        assert np.array_equal(narrow[0][k], wide[0][k]) and int(narrow[1][k]) == wide[1][k] and narrow[2][k] == wide[2][k]
        assert bin(wide[1][k]).count("1") == k
    assert np.array_equal(routes[0][0], routes[1][0]) and routes[0][1] == routes[1][1] and np.array_equal(routes[0][2], routes[1][2])


# ---- 2. more than 64 columns, few groups -------------------------------------------------------------------------------------
def test_ninety_six_columns_in_twelve_groups():
    from sparselm_amd.model import BestSubsetSelection

    X, y, groups, hidden, _ = suppressor(12, width=8, pairs=1, tau=0.3, n=150)
    assert X.shape == (150, 96) and len(np.unique(groups)) == 12
    ref = brute_force(X, y, groups=groups, K=3, big_M=1000)
    ranks = np.sort(search_rank(X, y, groups=groups)[np.flatnonzero(ref["active"])])
    print(f"supports {ref['n_supports']}, winner's search ranks {ranks.tolist()}")
    assert ref["n_supports"] <= MAX_SUPPORTS and set(hidden) <= set(np.flatnonzero(ref["active"]))
    assert 8 * ranks[0] < NARROW <= 8 * ranks[-1]  # the winner's columns lie on both sides of column 64 of the search order
    est = BestSubsetSelection(groups=groups, sparse_bound=3, big_M=1000, solver_options=WIDE).fit(X, y)
    compare(est, ref, X, y)
    assert est.solver_info_["capacity_cut"] is None and np.count_nonzero(est.coef_) == 24


# ---- 3. more than 64 groups: the second state slot and the high mask word --------------------------------------------------
SINGLETONS = {(66, 3): 100, (80, 2): 120, (100, 2): 150, (128, 2): 200}  # (ng, K): n


def singletons(ng, n):
    return suppressor(ng, pairs=1, tau=0.3, n=n)


@functools.lru_cache(maxsize=None)
def singletons_ref(ng, n, K, alpha=0.0, max_size=None, need=None):
    X, y, _, _, _ = singletons(ng, n)
    return brute_force(X, y, K=K, alpha=alpha, big_M=1000, max_size=max_size, hierarchy=[list(v) for v in need] if need is not None else None)


def assert_beyond_the_first_word(ref, rank, at_least=2):
    ranks = np.sort(rank[np.flatnonzero(ref["active"])])
    print(f"supports {ref['n_supports']}, winner's search ranks {ranks.tolist()}")
    assert ref["n_supports"] <= MAX_SUPPORTS and np.count_nonzero(ranks >= NARROW) >= at_least


@pytest.mark.parametrize("ng,K", sorted(SINGLETONS))
def test_more_than_64_groups_bounded(ng, K):
    from sparselm_amd.model import BestSubsetSelection

    n = SINGLETONS[ng, K]
    X, y, _, hidden, _ = singletons(ng, n)
    ref = singletons_ref(ng, n, K)
    assert set(hidden) <= set(np.flatnonzero(ref["active"]))
    assert_beyond_the_first_word(ref, search_rank(X, y))
    est = BestSubsetSelection(sparse_bound=K, big_M=1000, solver_options=WIDE).fit(X, y)
    compare(est, ref, X, y)
    assert est.solver_info_["capacity_cut"] is None


@pytest.mark.parametrize("rel_alpha", [0.02, 0.05, 0.2])
def test_more_than_64_groups_penalised(rel_alpha):
    from sparselm_amd.model import RegularizedL0

    X, y, _, hidden, _ = singletons(80, 120)
    alpha = rel_alpha * float(np.var(y))
    ref = singletons_ref(80, 120, None, alpha=alpha, max_size=2)
    assert ref["closed"] and set(np.flatnonzero(ref["active"])) == set(hidden)  # the hidden pair
    assert_beyond_the_first_word(ref, search_rank(X, y))
    est = RegularizedL0(alpha=alpha, big_M=1000, solver_options=WIDE).fit(X, y)
    compare(est, ref, X, y, alpha=alpha)
    assert est.solver_info_["capacity_cut"] is None


def test_every_support_is_visited_once_at_80_groups():
    """K = 2 and alpha = 0: nothing but the cardinality prunes (q_all lies below every value the search can hold, every
    column is independent, no include meets a full factor), so the node count is the one the rule of
    tests/test_l0_search_gpu.py gives."""
    from sparselm_amd.model import BestSubsetSelection

    X, y, _, _, _ = singletons(80, 120)
    ref = singletons_ref(80, 120, 2)
    r_all = X @ np.linalg.lstsq(X, y, rcond=None)[0] - y
    q_all = float(r_all @ r_all - y @ y) / (2 * 120)
    assert q_all < ref["objective"] * (1 + 1e-9) and np.linalg.matrix_rank(X) == 80
    fits = [BestSubsetSelection(sparse_bound=2, big_M=1000, solver_options=WIDE).fit(X, y) for _ in range(2)]
    compare(fits[0], ref, X, y)
    print(f"nodes {fits[0].solver_info_['nodes']}, {fits[1].solver_info_['nodes']}; expected {expected_nodes(80, 2)}")
    assert fits[0].solver_info_["nodes"] == fits[1].solver_info_["nodes"] == expected_nodes(80, 2)


# ---- 4. hierarchy across the word boundary -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["high_needs_low", "low_needs_high"])
def test_hierarchy_across_the_word_boundary(case):
    from sparselm_amd.model import BestSubsetSelection

    ng, n, K = 80, 120, 3
    X, y, _, hidden, _ = singletons(ng, n)
    rank = search_rank(X, y)
    at = np.argsort(rank)  # at[r]: the column of search rank r
    free = singletons_ref(ng, n, K)
    won = set(np.flatnonzero(free["active"]))
    need = [[] for _ in range(ng)]
    if case == "high_needs_low":  # the hidden group of rank 78 needs the decoy of rank 3
        assert at[78] in hidden and at[79] in hidden and at[3] not in won
        need[at[78]] = [at[3]]
    else:  # a group of the free winner in the first word needs a decoy beyond it: an engine that ignored the high word keeps the free winner
        src = next(j for j in won if rank[j] < NARROW)
        dst = next(j for j in at[NARROW:] if j not in won)
        print(f"the free winner's group of rank {rank[src]} needs the decoy of rank {rank[dst]}")
        need[src] = [dst]
    ref = singletons_ref(ng, n, K, need=tuple(tuple(int(v) for v in row) for row in need))
    ranks = np.sort(rank[np.flatnonzero(ref["active"])])
    print(f"free optimum's search ranks {np.sort(rank[list(won)]).tolist()}, with the hierarchy {ranks.tolist()}, supports {ref['n_supports']}, "
          f"gap {ref['gap']:.3e}")
    assert ref["n_supports"] <= MAX_SUPPORTS and free["n_supports"] <= MAX_SUPPORTS
    assert not np.array_equal(ref["active"], free["active"])  # the hierarchy changed the answer
    if case == "high_needs_low":
        assert ranks.tolist() == [3, 78, 79]
    assert np.count_nonzero(ranks >= NARROW) >= 1
    est = BestSubsetSelection(sparse_bound=K, hierarchy=need, big_M=1000, solver_options=WIDE).fit(X, y)
    compare(est, ref, X, y)
    assert_parents_active(est.active_groups_, need, list(range(ng)))


# ---- 5. capacity: a support holds at most 64 independent columns ---------------------------------------------------------------
def ten_groups_of_eight():
    X, y, groups, _, _ = suppressor(10, width=8, pairs=1, tau=0.3, n=160, noise=0.2)
    assert X.shape == (160, 80) and np.linalg.matrix_rank(X) == 80  # any nine groups exceed 64 independent columns
    return X, y, groups


@functools.lru_cache(maxsize=None)
def ten_groups_ref(K=None, rel_alpha=0.0):
    X, y, groups = ten_groups_of_eight()
    return brute_force(X, y, groups=groups, K=K, alpha=rel_alpha * float(np.var(y)), big_M=1000)


def test_capacity_cuts_the_search_and_says_so():
    from sparselm_amd.model import RegularizedL0

    X, y, groups = ten_groups_of_eight()
    alpha = 1e-9 * float(np.var(y))
    full, ref = ten_groups_ref(None, 1e-9), ten_groups_ref(8, 1e-9)
    print(f"full optimum {full['objective']:.12e} ({full['active'].sum()} groups), at most eight groups {ref['objective']:.12e} gap {ref['gap']:.3e}")
    assert full["active"].all() and ref["active"].sum() == 8 and ref["gap"] >= GAP_MIN and ref["kappa"] <= KAPPA_MAX
    est = RegularizedL0(groups=groups, alpha=alpha, big_M=1000, solver_options=WIDE)
    with pytest.warns(ConvergenceWarning, match="64 independent columns"):
        est.fit(X, y)
    info = est.solver_info_
    print(info)
    assert not info["proven_optimal"] and info["status"] == "capacity" and info["capacity_cut"] == 8
    assert info["lower_bound"] <= full["objective"] <= info["objective"]
    assert info["lower_bound"] <= info["q_all"] + 9 * alpha
    # the optimum over supports of at most eight groups, at the tolerances of ``compare``
    np.testing.assert_array_equal(est.active_groups_, ref["active"])
    assert abs(info["objective"] - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])
    assert abs(objective_of(X, y, est.coef_, 8, alpha=alpha) - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])
    assert np.max(np.abs(est.coef_ - ref["coef"])) <= COEF_RTOL * np.max(np.abs(ref["coef"]))


def test_capacity_is_no_obstacle_where_the_bound_closes_the_search():
    from sparselm_amd.model import BestSubsetSelection, RegularizedL0

    X, y, groups = ten_groups_of_eight()
    ref = ten_groups_ref(None, 0.05)
    assert ref["n_supports"] == 1024 and ref["active"].sum() == 2
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        est = RegularizedL0(groups=groups, alpha=0.05 * float(np.var(y)), big_M=1000, solver_options=WIDE).fit(X, y)
        compare(est, ref, X, y, alpha=0.05 * float(np.var(y)))
        assert est.solver_info_["capacity_cut"] is None
        # the cardinality bound stops the search before a ninth group is tried
        est = BestSubsetSelection(groups=groups, sparse_bound=8, big_M=1000, solver_options=WIDE).fit(X, y)
        compare(est, ten_groups_ref(8, 0.0), X, y)
        assert est.solver_info_["capacity_cut"] is None


def test_wide_profile_under_the_capacity():
    from sparselm_amd.miqp import l0_profile
    from sparselm_amd.model import BestSubsetSelection

    X, y, groups = ten_groups_of_eight()
    with pytest.raises(NotImplementedError, match="64"):
        l0_profile(X, y, groups=groups, max_groups=9, big_M=1000, solver_options=WIDE)
    prof = l0_profile(X, y, groups=groups, max_groups=8, big_M=1000, solver_options=WIDE)
    assert prof.proven_optimal_ and prof.solver_info_["status"] == "optimal" and (np.diff(prof.values_) < 0).all()
    for bound in range(1, 9):
        est = BestSubsetSelection(groups=groups, sparse_bound=bound, big_M=1000, solver_options=WIDE).fit(X, y)
        coef, _, active = prof.best_subset(bound)
        np.testing.assert_array_equal(active, est.active_groups_)
        assert active.sum() == bound and np.array_equal(coef, est.coef_) and prof.values_[bound] == est.solver_info_["objective"]
    table = profile_table(X, y, groups=groups, K=3, big_M=1000)
    for k in range(4):
        print(f"size {k}: reference {table['values'][k]:.12e} gap {table['gaps'][k]:.3e}; engine {prof.values_[k]:.12e}")
        assert k == 0 or (table["gaps"][k] >= GAP_MIN and table["kappas"][k] <= KAPPA_MAX)
        np.testing.assert_array_equal(prof.supports_[k], table["actives"][k])
        assert abs(prof.values_[k] - table["values"][k]) <= OBJ_RTOL * abs(table["values"][k])
        assert np.max(np.abs(prof.coefs_[k] - table["coefs"][k])) <= COEF_RTOL * max(np.max(np.abs(table["coefs"][k])), np.finfo(float).tiny)


# ---- 6. the wide profile over singletons ---------------------------------------------------------------------------------------
def test_wide_profile_over_80_singletons():
    from sparselm_amd.miqp import l0_profile

    X, y, _, hidden, _ = singletons(80, 120)
    prof = l0_profile(X, y, max_groups=2, alpha_min=0.0, big_M=1000, solver_options=WIDE)
    assert prof.proven_optimal_ and prof.values_[0] == 0.0 and prof.values_.shape == (3,)
    one = brute_force(X, y, K=1, big_M=1000)
    two = singletons_ref(80, 120, 2)
    assert one["active"].sum() == 1 and two["active"].sum() == 2  # (best subset at the bound k holds k columns here: the table's row k)
    assert_beyond_the_first_word(two, search_rank(X, y))
    for k, ref in ((1, one), (2, two)):
        est = types.SimpleNamespace(coef_=prof.coefs_[k], active_groups_=prof.supports_[k], solver_info_=dict(
            prof.solver_info_, objective=float(prof.values_[k]), lower_bound=float(prof.values_[k])))
        compare(est, ref, X, y)


# ---- 7. the reference's own data: 290 x 66 -----------------------------------------------------------------------------------
def test_reference_data_66_columns():
    from sparselm_amd.model import L2L0

    X = np.load(os.path.join(ROOT, "tests", "golden", "reference_examples", "corr.npy"))
    y = np.load(os.path.join(ROOT, "tests", "golden", "reference_examples", "energy.npy"))
    assert X.shape == (290, 66)
    constant = np.flatnonzero(np.ptp(X, axis=0) == 0.0)  # (the fixture holds none: the check on it is made below, with one added)
    alpha, eta = 3.16e-7, 1.66e-6
    fits = []
    for _ in range(2):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", ConvergenceWarning)
            fits.append(L2L0(fit_intercept=True, alpha=alpha, eta=eta, solver_options={"wide": True, "max_nodes": 2**22}).fit(X, y))
    est = fits[0]
    info = est.solver_info_
    print(info, int(est.active_groups_.sum()))
    assert info["lower_bound"] <= info["objective"] <= info["seed_objective"]
    Xc, yc = X - X.mean(axis=0), y - y.mean()
    at_coef = objective_of(Xc, yc, est.coef_, int(est.active_groups_.sum()), alpha=alpha, eta=eta)
    assert abs(at_coef - info["objective"]) <= OBJ_RTOL * abs(info["objective"])
    assert not est.coef_[constant].any() and np.isfinite(est.coef_).all()
    assert fits[0].coef_.tobytes() == fits[1].coef_.tobytes()
    # a column that is constant in the data: the fixture has none (its centred rank is 66), so one is appended -- centred away
    # under fit_intercept, it can gain nothing and must keep a zero coefficient
    X1 = np.column_stack([X, np.ones(len(y))])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        est1 = L2L0(fit_intercept=True, alpha=alpha, eta=eta, solver_options={"wide": True, "max_nodes": 2**22}).fit(X1, y)
    info1 = est1.solver_info_
    assert est1.coef_[66] == 0.0 and not est1.active_groups_[66] and info1["lower_bound"] <= info1["objective"] <= info1["seed_objective"]
    at_coef = objective_of(np.column_stack([Xc, np.zeros(len(y))]), yc, est1.coef_, int(est1.active_groups_.sum()), alpha=alpha, eta=eta)
    assert abs(at_coef - info1["objective"]) <= OBJ_RTOL * abs(info1["objective"])


def test_65_columns_without_the_option_point_to_it():
    from sparselm_amd.model import BestSubsetSelection

    X, y = make_regression(80, 65, n_informative=5, random_state=2)
    with pytest.raises(NotImplementedError, match="64.*wide"):
        BestSubsetSelection(sparse_bound=1).fit(X, y)
    est = BestSubsetSelection(sparse_bound=1, big_M=1000, solver_options=WIDE).fit(X, y)
    compare(est, brute_force(X, y, K=1, big_M=1000), X, y)
