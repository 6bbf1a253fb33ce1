"""The exact l0 estimators on the GPU (``slm_solve_l0``, csrc/l0_kernels.hpp) against the brute force of
tests/_l0_reference.py, which solves every admissible support straight from X.

Every comparison first asserts ON THE REFERENCE'S NUMBERS that the question is well posed -- the relative gap to the
second-best support is >= 1e-6 and the condition number of the winner's Gram block is <= 1e4 -- and then: identical
supports, objectives to 1e-10 relative, coefficients to 1e-9 relative in the infinity norm (kappa * 2^-52 ~ 2e-12 for the
engine's Gram route, with a margin of about 500).  Every call must come back ``proven_optimal`` under the default budget.
Sizes stay at p <= 14 so that a brute force takes well under a second.

Mirrors /root/reference/tests/test_miqp.py (slack variables :69-103, hierarchy :105-224), whose solver is Gurobi."""

import functools
import warnings

import numpy as np
import pytest
from sklearn.datasets import make_regression
from sklearn.exceptions import ConvergenceWarning

from _l0_reference import brute_force, forward_stepwise, objective_of

pytestmark = pytest.mark.gpu

GAP_MIN, KAPPA_MAX, OBJ_RTOL, COEF_RTOL = 1e-6, 1e4, 1e-10, 1e-9


@functools.lru_cache(maxsize=None)
def draw(n, p=12):
    X, y = make_regression(n, p, n_informative=5, noise=1.0, random_state=0)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def compare(est, ref, X, y, alpha=0.0, eta=0.0, W=None, check_premise=True):
    """The comparison every test shares: premise on the reference, then support, objective, coefficients."""
    print(f"reference: gap {ref['gap']:.3e} kappa {ref['kappa']:.3e} objective {ref['objective']:.12e}; engine: objective "
          f"{est.solver_info_['objective']:.12e} nodes {est.solver_info_['nodes']} status {est.solver_info_['status']}")
    if check_premise:
        assert ref["gap"] >= GAP_MIN and ref["kappa"] <= KAPPA_MAX
    info = est.solver_info_
    assert info["proven_optimal"] and info["status"] == "optimal"
    assert info["lower_bound"] == info["objective"]
    np.testing.assert_array_equal(est.active_groups_, ref["active"])
    scale = max(abs(ref["objective"]), np.finfo(float).tiny)
    assert abs(info["objective"] - ref["objective"]) <= OBJ_RTOL * scale
    # ... and the reported objective is the objective of the reported coefficients
    at_coef = objective_of(X, y, est.coef_, int(est.active_groups_.sum()), alpha=alpha, eta=eta, W=W)
    assert abs(at_coef - ref["objective"]) <= OBJ_RTOL * scale
    top = np.max(np.abs(ref["coef"]))
    if top > 0:
        err = np.max(np.abs(est.coef_ - ref["coef"])) / top
        print(f"coefficients: rel-inf error {err:.3e}")
        assert err <= COEF_RTOL
    else:
        assert not est.coef_.any()


# ---- 1. the four estimators on an overdetermined and an underdetermined draw ------------------------------------------------
@pytest.mark.parametrize("n", [40, 10])
@pytest.mark.parametrize("K", [1, 3, 5])
def test_best_subset(n, K):
    from sparselm_amd.model import BestSubsetSelection

    X, y = draw(n)
    est = BestSubsetSelection(sparse_bound=K, big_M=1000).fit(X, y)
    compare(est, brute_force(X, y, K=K, big_M=1000), X, y)
    assert est.active_groups_.sum() <= K and est.intercept_ == 0.0


@pytest.mark.parametrize("n", [40, 10])
@pytest.mark.parametrize("rel_alpha", [1e-4, 1e-2, 0.2])
def test_regularized_l0(n, rel_alpha):
    from sparselm_amd.model import RegularizedL0

    X, y = draw(n)
    alpha = rel_alpha * float(np.var(y))
    est = RegularizedL0(alpha=alpha, big_M=1000).fit(X, y)
    compare(est, brute_force(X, y, alpha=alpha, big_M=1000), X, y, alpha=alpha)


@pytest.mark.parametrize("n", [40, 10])
@pytest.mark.parametrize("eta", [1e-2, 1.0])
def test_ridged_best_subset_and_l2l0(n, eta):
    from sparselm_amd.model import L2L0, RidgedBestSubsetSelection

    X, y = draw(n)
    est = RidgedBestSubsetSelection(sparse_bound=3, eta=eta, big_M=1000).fit(X, y)
    compare(est, brute_force(X, y, K=3, eta=eta, big_M=1000), X, y, eta=eta)
    alpha = 1e-2 * float(np.var(y))
    est = L2L0(alpha=alpha, eta=eta, big_M=1000).fit(X, y)
    compare(est, brute_force(X, y, alpha=alpha, eta=eta, big_M=1000), X, y, alpha=alpha, eta=eta)


def test_l2l0_with_a_tikhonov_matrix():
    from sparselm_amd.model import L2L0

    X, y = draw(40)
    W = np.random.default_rng(1).standard_normal((12, 12))
    alpha = 1e-2 * float(np.var(y))
    est = L2L0(alpha=alpha, eta=0.1, tikhonov_w=W, big_M=1000).fit(X, y)
    compare(est, brute_force(X, y, alpha=alpha, eta=0.1, W=W, big_M=1000), X, y, alpha=alpha, eta=0.1, W=W)


# ---- 2. a design on which greedy forward selection is wrong ---------------------------------------------------------------
def ar1_draw(seed=7, n=40, p=12, rho=0.9):
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, p))
    X = np.empty((n, p))
    X[:, 0] = Z[:, 0]
    for j in range(1, p):
        X[:, j] = rho * X[:, j - 1] + np.sqrt(1 - rho**2) * Z[:, j]
    beta = np.zeros(p)
    beta[[2, 5, 8]] = [1.0, -1.0, 1.0]
    return X, X @ beta + 0.5 * rng.standard_normal(n)


def test_optimum_where_forward_stepwise_is_wrong():
    from sparselm_amd.model import BestSubsetSelection

    X, y = ar1_draw()
    ref = brute_force(X, y, K=3)
    greedy, greedy_rss = forward_stepwise(X, y, 3)
    assert greedy != list(np.flatnonzero(ref["active"]))  # the premise: stepwise selection misses the optimum here
    est = BestSubsetSelection(sparse_bound=3, big_M=1000).fit(X, y)
    compare(est, ref, X, y)
    assert est.solver_info_["objective"] < est.solver_info_["seed_objective"]


# ---- 3. groups ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_groups", [4, 6])
def test_groups_enter_whole(n_groups):
    from sparselm_amd.model import BestSubsetSelection, RegularizedL0

    X, y = draw(40)
    rng = np.random.default_rng(n_groups)
    sizes = {4: [5, 1, 4, 2], 6: [1, 3, 2, 1, 4, 1]}[n_groups]
    labels = rng.permutation(np.arange(10, 10 + 7 * n_groups, 7))  # shuffled, unevenly spaced labels
    groups = rng.permutation(np.repeat(labels, sizes))
    K = n_groups // 2
    alpha = 1e-2 * float(np.var(y))
    for est, ref in (
        (BestSubsetSelection(groups=groups, sparse_bound=K, big_M=1000), brute_force(X, y, groups=groups, K=K, big_M=1000)),
        (RegularizedL0(groups=groups, alpha=alpha, big_M=1000), brute_force(X, y, groups=groups, alpha=alpha, big_M=1000)),
    ):
        est.fit(X, y)
        compare(est, ref, X, y, alpha=alpha if isinstance(est, RegularizedL0) else 0.0)
        for lab, active in zip(np.unique(groups), est.active_groups_):
            assert (est.coef_[groups == lab] != 0).all() if active else (est.coef_[groups == lab] == 0).all()


# ---- 4. hierarchy ----------------------------------------------------------------------------------------------------------
def test_fully_chained_hierarchy_gives_all_zeros():
    # /root/reference/tests/test_miqp.py:116-127: a ring of dependencies and a bound below p leave nothing
    from sparselm_amd.model import BestSubsetSelection

    X, y = draw(40)
    p = X.shape[1]
    chained = [[p - 1]] + [[i] for i in range(p - 1)]
    est = BestSubsetSelection(sparse_bound=p // 2, hierarchy=chained, big_M=1000).fit(X, y)
    assert est.solver_info_["proven_optimal"]
    assert (est.coef_ == 0).all() and not est.active_groups_.any() and est.solver_info_["objective"] == 0.0


def assert_parents_active(active, hierarchy, labels):
    index = {lab: i for i, lab in enumerate(labels)}
    for i, parents in enumerate(hierarchy):
        if active[i]:
            assert all(active[index[q]] for q in parents)


@pytest.mark.parametrize("kind", ["bound", "alpha"])
def test_star_hierarchy(kind):
    # /root/reference/tests/test_miqp.py:129-149: everything depends on one column, halves on two more
    from sparselm_amd.model import BestSubsetSelection, RegularizedL0

    X, y = draw(40)
    p = X.shape[1]
    free = brute_force(X, y, K=5)
    idx = np.flatnonzero(free["active"])
    # (parents chosen among the columns the free optimum does NOT use, so that the hierarchy changes the answer)
    out = [j for j in range(p) if j not in idx]
    hub, left, right = out[0], out[1], out[2]
    hierarchy = []
    for i in range(p):
        hierarchy.append([] if i == hub else [hub])
        if 0 < i < p // 2 and i not in (left, hub):
            hierarchy[i].append(left)
        if p // 2 <= i and i not in (right, hub):
            hierarchy[i].append(right)
    if kind == "bound":
        est = BestSubsetSelection(sparse_bound=5, hierarchy=hierarchy, big_M=1000).fit(X, y)
        ref = brute_force(X, y, K=5, hierarchy=hierarchy, big_M=1000)
        compare(est, ref, X, y)
    else:
        alpha = 1e-2 * float(np.var(y))
        est = RegularizedL0(alpha=alpha, hierarchy=hierarchy, big_M=1000).fit(X, y)
        ref = brute_force(X, y, alpha=alpha, hierarchy=hierarchy, big_M=1000)
        compare(est, ref, X, y, alpha=alpha)
    assert not np.array_equal(ref["active"], free["active"])  # the hierarchy changed the answer
    assert_parents_active(est.active_groups_, hierarchy, list(range(p)))


def test_group_level_hierarchy():
    from sparselm_amd.model import RegularizedL0

    X, y = draw(40)
    groups = np.array([30, 30, 10, 10, 10, 20, 20, 50, 40, 40, 40, 50])
    labels = [10, 20, 30, 40, 50]
    hierarchy = [[50], [10], [10, 50], [], [40]]  # entry i: the labels that label i needs
    alpha = 1e-2 * float(np.var(y))
    est = RegularizedL0(groups=groups, alpha=alpha, hierarchy=hierarchy, big_M=1000).fit(X, y)
    ref = brute_force(X, y, groups=groups, alpha=alpha, hierarchy=hierarchy, big_M=1000)
    compare(est, ref, X, y, alpha=alpha)
    assert_parents_active(est.active_groups_, hierarchy, labels)


# ---- 5. the box --------------------------------------------------------------------------------------------------------------
def test_big_m_binds():
    from sparselm_amd.model import BestSubsetSelection, RegularizedL0

    X, y = draw(40)
    assert np.max(np.abs(brute_force(X, y, K=5)["coef"])) > 50  # the premise: the unboxed winner leaves the box
    est = BestSubsetSelection(sparse_bound=5, big_M=50).fit(X, y)
    compare(est, brute_force(X, y, K=5, big_M=50), X, y)
    assert np.max(np.abs(est.coef_)) <= 50
    alpha = 1e-2 * float(np.var(y))
    est = RegularizedL0(alpha=alpha, big_M=50).fit(X, y)
    compare(est, brute_force(X, y, alpha=alpha, big_M=50), X, y, alpha=alpha)
    assert np.max(np.abs(est.coef_)) <= 50


# ---- 6. rank deficiency ------------------------------------------------------------------------------------------------------
def test_duplicated_column():
    """Column 5 is a copy of column 3: two supports tie exactly, so the premise on the gap does not apply and only the
    objective is compared; the engine's pivot rule keeps at most one of the two."""
    from sparselm_amd.model import BestSubsetSelection, RegularizedL0

    X, y = make_regression(20, 8, n_informative=4, noise=1.0, random_state=1)
    X[:, 5] = X[:, 3]
    alpha = 1e-3 * float(np.var(y))
    for est, ref in (
        (BestSubsetSelection(sparse_bound=4, big_M=1000), brute_force(X, y, K=4, big_M=1000)),
        (RegularizedL0(alpha=alpha, big_M=1000), brute_force(X, y, alpha=alpha, big_M=1000)),
    ):
        est.fit(X, y)
        info = est.solver_info_
        print(f"reference objective {ref['objective']:.12e}, engine {info['objective']:.12e}")
        assert info["proven_optimal"] and np.isfinite(est.coef_).all() and np.isfinite(info["objective"])
        assert abs(info["objective"] - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])
        assert not (est.coef_[3] != 0 and est.coef_[5] != 0)


# ---- 6b. dependent columns inside groups, and dependent parents ------------------------------------------------------------
def compare_singular(est, ref, X, y, alpha=0.0):
    """For designs whose winning block is singular by construction: the premise on kappa cannot hold and the coefficients
    are not unique (the brute force's lstsq returns the minimum-norm ones, the engine leaves a dependent column at 0), so
    the support, the objective and the FITTED VALUES are compared -- those are unique -- at the tolerances of ``compare``."""
    info = est.solver_info_
    print(f"reference: gap {ref['gap']:.3e} objective {ref['objective']:.12e} active {np.flatnonzero(ref['active'])}; engine: objective "
          f"{info['objective']:.12e} active {np.flatnonzero(est.active_groups_)} nodes {info['nodes']} status {info['status']}")
    assert ref["gap"] >= GAP_MIN
    assert info["proven_optimal"] and info["lower_bound"] == info["objective"]
    np.testing.assert_array_equal(est.active_groups_, ref["active"])
    assert abs(info["objective"] - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])
    at_coef = objective_of(X, y, est.coef_, int(est.active_groups_.sum()), alpha=alpha)
    assert abs(at_coef - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])
    fit_ref = X @ ref["coef"]
    err = np.max(np.abs(X @ est.coef_ - fit_ref)) / np.max(np.abs(fit_ref))
    print(f"fitted values: rel-inf error {err:.3e}")
    assert err <= COEF_RTOL and np.isfinite(est.coef_).all()


def test_group_with_a_collinear_column():
    """Groups {a, 2a}, {c}, {d, e} and y ~ a: the first group must be found although its second column depends on its
    first (it stays at 0; an INACTIVE group is all zero, an active one need not be all non-zero)."""
    from sparselm_amd.model import BestSubsetSelection, RegularizedL0

    rng = np.random.default_rng(11)
    a, c, d, e = rng.standard_normal((4, 30))
    X = np.column_stack([a, 2 * a, c, d, e])
    y = 3 * a + 0.3 * c + 0.1 * rng.standard_normal(30)
    groups = np.array([0, 0, 1, 2, 2])
    est = BestSubsetSelection(groups=groups, sparse_bound=1, big_M=1000).fit(X, y)
    compare_singular(est, brute_force(X, y, groups=groups, K=1, big_M=1000), X, y)
    assert est.active_groups_.tolist() == [True, False, False] and not est.coef_[2:].any()
    alpha = 1e-3 * float(np.var(y))
    est = RegularizedL0(groups=groups, alpha=alpha, big_M=1000).fit(X, y)
    compare_singular(est, brute_force(X, y, groups=groups, alpha=alpha, big_M=1000), X, y, alpha=alpha)
    assert est.active_groups_[0]


def test_centred_one_hot_group():
    """A one-hot group under ``fit_intercept=True``: the centred indicator columns sum to zero, so the last one depends
    on the others -- the group must still be active when the levels carry the signal."""
    from sparselm_amd.model import BestSubsetSelection

    rng = np.random.default_rng(12)
    level = rng.integers(0, 3, 36)
    Z = rng.standard_normal((36, 3))
    X = np.column_stack([np.eye(3)[level], Z])
    y = np.array([4.0, -2.0, 1.0])[level] + 0.5 * Z[:, 1] + 0.1 * rng.standard_normal(36)
    groups = np.array([7, 7, 7, 1, 2, 3])
    est = BestSubsetSelection(groups=groups, sparse_bound=2, big_M=1000, fit_intercept=True).fit(X, y)
    Xp, yp = X - X.mean(axis=0), y - y.mean()
    ref = brute_force(Xp, yp, groups=groups, K=2, big_M=1000)
    compare_singular(est, ref, Xp, yp)
    assert est.active_groups_[-1]  # (label 7 sorts last)
    np.testing.assert_allclose(est.predict(X), Xp @ ref["coef"] + y.mean(), rtol=0, atol=1e-8)


def test_fewer_rows_than_columns_with_rank_deficient_groups():
    """n = 10 < p = 12 in four groups of three; the first two groups span one 4-dimensional subspace together (the second
    is only partly new beside the first), the last two another.  The pair that spans the subspace of the signal wins."""
    from sparselm_amd.model import BestSubsetSelection, RegularizedL0

    rng = np.random.default_rng(13)
    U, V = rng.standard_normal((10, 4)), rng.standard_normal((10, 4))
    X = np.column_stack([U @ rng.standard_normal((4, 6)), V @ rng.standard_normal((4, 6))])
    y = U @ np.array([3.0, -2.0, 2.5, 1.5]) + 0.05 * rng.standard_normal(10)
    groups = np.repeat([0, 1, 2, 3], 3)
    assert np.linalg.matrix_rank(X[:, :6]) == 4 and np.linalg.matrix_rank(X) == 8
    est = BestSubsetSelection(groups=groups, sparse_bound=2, big_M=1000).fit(X, y)
    compare_singular(est, brute_force(X, y, groups=groups, K=2, big_M=1000), X, y)
    assert est.active_groups_.tolist() == [True, True, False, False] and not est.coef_[6:].any()
    alpha = 1e-3 * float(np.var(y))
    est = RegularizedL0(groups=groups, alpha=alpha, big_M=1000).fit(X, y)
    compare_singular(est, brute_force(X, y, groups=groups, alpha=alpha, big_M=1000), X, y, alpha=alpha)
    assert est.active_groups_.tolist() == [True, True, False, False]


def test_dependent_parent_under_hierarchy():
    """Column 5 = column 3 + column 4, and columns 0, 1, 2 need 5, 3, 4: the optimum holds all six, and whichever of 3, 4, 5
    comes last in the search order brings no column of its own -- it must be included all the same, because a group needs it."""
    from sparselm_amd.model import RegularizedL0

    rng = np.random.default_rng(14)
    X = rng.standard_normal((30, 8))
    X[:, 5] = X[:, 3] + X[:, 4]
    y = X[:, :5] @ np.array([4.0, -3.0, 3.5, 2.0, -2.5]) + 0.1 * rng.standard_normal(30)
    hierarchy = [[5], [3], [4], [], [], [], [], []]
    alpha = 1e-3 * float(np.var(y))
    est = RegularizedL0(alpha=alpha, hierarchy=hierarchy, big_M=1000).fit(X, y)
    ref = brute_force(X, y, alpha=alpha, hierarchy=hierarchy, big_M=1000)
    compare_singular(est, ref, X, y, alpha=alpha)
    assert est.active_groups_.tolist() == [True] * 6 + [False] * 2
    assert_parents_active(est.active_groups_, hierarchy, list(range(8)))


# ---- 7. intercept and sample weights -----------------------------------------------------------------------------------------
def test_intercept_and_sample_weight():
    from sparselm_amd.model import BestSubsetSelection

    X, y = draw(40)
    X = X + 3.0
    y = y + 10.0
    w = np.random.default_rng(5).uniform(0.5, 2.0, 40)
    est = BestSubsetSelection(sparse_bound=3, big_M=1000, fit_intercept=True).fit(X, y, sample_weight=w)
    # the reference's preprocessing (sklearn's _preprocess_data + _rescale_data): weights summing to n, weighted centring,
    # rows times sqrt(w)
    wn = w * (40 / w.sum())
    xm, ym = np.average(X, axis=0, weights=wn), np.average(y, weights=wn)
    Xp, yp = (X - xm) * np.sqrt(wn)[:, None], (y - ym) * np.sqrt(wn)
    ref = brute_force(Xp, yp, K=3, big_M=1000)
    compare(est, ref, Xp, yp)
    assert abs(est.intercept_ - (ym - xm @ ref["coef"])) <= 1e-9 * max(1.0, abs(ym))
    np.testing.assert_allclose(est.predict(X[:3]), X[:3] @ est.coef_ + est.intercept_)


# ---- 8. widths ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 63, 64])
def test_widths(p):
    from sparselm_amd.model import BestSubsetSelection, RegularizedL0

    X, y = make_regression(80, p, n_informative=min(p, 5), noise=1.0, random_state=2)
    # alpha above ||y||^2 / (2n): no support can gain what it costs, the optimum is the empty one
    est = RegularizedL0(alpha=1.01 * float(y @ y) / (2 * 80), big_M=1000).fit(X, y)
    assert est.solver_info_["proven_optimal"] and not est.coef_.any() and est.solver_info_["objective"] == 0.0
    # one column: the reference is a p-way scan
    est = BestSubsetSelection(sparse_bound=1, big_M=1000).fit(X, y)
    compare(est, brute_force(X, y, K=1, big_M=1000), X, y, check_premise=p > 1)


def test_65_columns_are_refused_by_the_engine():
    from sparselm_amd.model import BestSubsetSelection

    X, y = make_regression(80, 65, n_informative=5, random_state=2)
    with pytest.raises(NotImplementedError, match="64"):
        BestSubsetSelection(sparse_bound=1).fit(X, y)


# ---- 9. the node budget ------------------------------------------------------------------------------------------------------
def test_exhausted_budget_keeps_the_incumbent():
    from sparselm_amd.model import BestSubsetSelection

    X, y = make_regression(25, 30, n_informative=10, noise=1.0, random_state=0)
    est = BestSubsetSelection(sparse_bound=15, big_M=1000, solver_options={"max_nodes": 1000})
    with pytest.warns(ConvergenceWarning):
        est.fit(X, y)
    info = est.solver_info_
    print(info)
    assert not info["proven_optimal"] and info["status"] == "node_budget"
    assert info["lower_bound"] <= info["objective"] <= info["seed_objective"]
    assert info["nodes"] >= 1000 and est.active_groups_.sum() <= 15
    at_coef = objective_of(X, y, est.coef_, int(est.active_groups_.sum()))
    assert abs(at_coef - info["objective"]) <= 1e-9 * abs(info["objective"])


# ---- 10. determinism ---------------------------------------------------------------------------------------------------------
def test_two_fits_give_identical_coefficients():
    """``coef_`` is bit-identical between two fits of one problem: the winner is picked from the wavefronts' bests in a
    fixed order and its coefficients are recomputed in one place.  ``nodes`` may differ, because pruning depends on when
    a wavefront sees another one's incumbent."""
    from sparselm_amd.model import L2L0

    X, y = make_regression(25, 20, n_informative=10, noise=1.0, random_state=0)
    fits = [L2L0(alpha=3.0, eta=1.0, big_M=1000).fit(X, y) for _ in range(2)]
    assert fits[0].solver_info_["proven_optimal"] and fits[1].solver_info_["proven_optimal"]
    assert fits[0].coef_.tobytes() == fits[1].coef_.tobytes()
    assert fits[0].solver_info_["objective"] == fits[1].solver_info_["objective"]
    np.testing.assert_array_equal(fits[0].active_groups_, fits[1].active_groups_)


# ---- 11. the two routes into the library -------------------------------------------------------------------------------------
def test_ctypes_and_compiled_binding_agree():
    from sparselm_amd import _engine

    if _engine.load_binding() is None:
        pytest.fail("the compiled binding is not built")
    X, y = draw(40)
    eng = _engine.get_engine()
    W = np.random.default_rng(1).standard_normal((12, 12))
    need = [0] * 12
    need[3] = 1 << 0
    with eng.dataset(X, y) as ds:
        a = ds.solve_l0(alpha=10.0, max_groups=6, eta=0.1, T=W.T @ W, big_M=50.0, need=need, binding=False)
        b = ds.solve_l0(alpha=10.0, max_groups=6, eta=0.1, T=W.T @ W, big_M=50.0, need=need, binding=True)
        with pytest.raises(ValueError):
            ds.solve_l0(alpha=-1.0, binding=False)
        with pytest.raises(ValueError):
            ds.solve_l0(alpha=-1.0, binding=True)
        with pytest.raises(ValueError):
            ds.solve_l0(need=[1 << 12] + [0] * 11, binding=False)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    for key in ("objective", "lower_bound", "proven_optimal", "status", "loss", "seed_objective", "q_all", "launches"):
        assert a[2][key] == b[2][key], key
    assert a[2]["launches"] == 1 and abs(a[2]["loss"] - np.sum((X @ a[0] - y) ** 2) / 80) <= 1e-10 * a[2]["loss"]


# ---- 12. model selection ---------------------------------------------------------------------------------------------------
def test_grid_search_over_the_bound():
    from sparselm_amd.model import BestSubsetSelection
    from sparselm_amd.model_selection import GridSearchCV

    X, y = draw(40)
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        search = GridSearchCV(BestSubsetSelection(big_M=1000), {"sparse_bound": [1, 2, 3]}, cv=4).fit(X, y)
    assert search.best_params_["sparse_bound"] in (1, 2, 3)
    assert np.count_nonzero(search.best_estimator_.coef_) <= search.best_params_["sparse_bound"]
