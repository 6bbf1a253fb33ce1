"""``L1L0`` on the GPU (``slm_solve_l0_l1``: the l1 mode of the exact search, csrc/l0_kernels.hpp) against the brute force of
tests/_l1l0_reference.py, which solves a lasso per admissible support straight from X and asserts every solution's KKT
residual.

As in test_l0_gpu.py every comparison first asserts ON THE REFERENCE'S NUMBERS that the question is well posed -- relative
gap to the second-best support >= 1e-6, condition number of the winner's active block <= 1e4 -- and then: identical
``active_groups_``, objectives to 1e-10 relative, coefficients to 1e-9 relative in the infinity norm (the project's constants:
both sides end in an exact solve on the sign pattern).  ``proven_optimal`` must hold with ``lower_bound == objective``."""

import functools
import warnings

import numpy as np
import pytest
from sklearn.datasets import make_regression
from sklearn.exceptions import ConvergenceWarning

from _l1l0_reference import brute_force_l1, objective_of_l1, solve_support_l1

pytestmark = pytest.mark.gpu

GAP_MIN, KAPPA_MAX, OBJ_RTOL, COEF_RTOL = 1e-6, 1e4, 1e-10, 1e-9


@functools.lru_cache(maxsize=None)
def draw(n, p=10):
    X, y = make_regression(n, p, n_informative=5, noise=1.0, random_state=0)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def scales(X, y):
    """(var y, ||X^T y / n||_inf): what alpha and eta are stated relative to"""
    return float(np.var(y)), float(np.max(np.abs(X.T @ y / X.shape[0])))


def compare(est, ref, X, y, alpha, eta, coefficients=True):
    """Premise on the reference, then support, objective, coefficients (or fitted values where those are what is unique)."""
    info = est.solver_info_
    print(f"reference: gap {ref['gap']:.3e} kappa {ref['kappa']:.3e} kkt {ref['kkt']:.1e} objective {ref['objective']:.12e} active "
          f"{np.flatnonzero(ref['active'])}; engine: objective {info['objective']:.12e} active {np.flatnonzero(est.active_groups_)} nodes "
          f"{info['nodes']} descents {info['descents']} bound {info['q_all']:.6e} status {info['status']}")
    assert ref["gap"] >= GAP_MIN and (ref["kappa"] <= KAPPA_MAX or not coefficients)
    assert info["proven_optimal"] and info["status"] == "optimal"
    assert info["lower_bound"] == info["objective"]
    np.testing.assert_array_equal(est.active_groups_, ref["active"])
    scale = max(abs(ref["objective"]), np.finfo(float).tiny)
    assert abs(info["objective"] - ref["objective"]) <= OBJ_RTOL * scale
    at_coef = objective_of_l1(X, y, est.coef_, int(est.active_groups_.sum()), alpha=alpha, eta=eta)
    assert abs(at_coef - ref["objective"]) <= OBJ_RTOL * scale
    got, want = (est.coef_, ref["coef"]) if coefficients else (X @ est.coef_, X @ ref["coef"])
    top = np.max(np.abs(want))
    if top > 0:
        err = np.max(np.abs(got - want)) / top
        print(f"{'coefficients' if coefficients else 'fitted values'}: rel-inf error {err:.3e}")
        assert err <= COEF_RTOL
    else:
        assert not est.coef_.any()


# ---- 1. an overdetermined and an underdetermined draw, three alphas by three etas ------------------------------------------
@pytest.mark.parametrize("n", [40, 10])
@pytest.mark.parametrize("rel_alpha", [1e-4, 1e-2, 0.2])
@pytest.mark.parametrize("rel_eta", [1e-3, 0.05, 0.5])
def test_l1l0(n, rel_alpha, rel_eta):
    from sparselm_amd.miqp import L1L0

    X, y = draw(n)
    var, cinf = scales(X, y)
    alpha, eta = rel_alpha * var, rel_eta * cinf
    est = L1L0(alpha=alpha, eta=eta, big_M=1000).fit(X, y)
    compare(est, brute_force_l1(X, y, alpha=alpha, eta=eta, big_M=1000), X, y, alpha, eta)
    assert est.intercept_ == 0.0


def test_eta_changes_the_support():
    """n = 10, alpha = 1e-4 var y, eta = 0.05 ||c||_inf: the optimum {0, 2, 3, 6, 7} is not RegularizedL0's {0, 3, 6, 7} -- an
    engine that ignored eta would return the latter."""
    from sparselm_amd.miqp import L1L0, RegularizedL0

    X, y = draw(10)
    var, cinf = scales(X, y)
    with_l1 = L1L0(alpha=1e-4 * var, eta=0.05 * cinf, big_M=1000).fit(X, y)
    without = RegularizedL0(alpha=1e-4 * var, big_M=1000).fit(X, y)
    assert np.flatnonzero(with_l1.active_groups_).tolist() == [0, 2, 3, 6, 7]
    assert np.flatnonzero(without.active_groups_).tolist() == [0, 3, 6, 7]


# ---- 2. a dependent column that carries the coefficient ------------------------------------------------------------------
def dependent_case():
    rng = np.random.default_rng(3)
    X = rng.standard_normal((30, 8))
    X[:, 7] = X[:, 0] + X[:, 1]
    y = 3 * (X[:, 0] + X[:, 1]) + 2 * X[:, 4] + 0.1 * rng.standard_normal(30)
    groups = np.array([0, 0, 1, 2, 3, 4, 5, 0])  # {0, 1, 7}, {2}, {3}, {4}, {5}, {6}
    return X, y, groups


def test_dependent_column_inside_a_group():
    """Column 7 = column 0 + column 1, all three in one group: with an l1 term the optimum puts ONE coefficient on column 7
    (objective -11.5095) where the pivot rule's answer, two coefficients on columns 0 and 1, costs -10.5649.  Objective and
    fitted values are compared, not coefficients."""
    from sparselm_amd.miqp import L1L0

    X, y, groups = dependent_case()
    var, cinf = scales(X, y)
    alpha, eta = 1e-2 * var, 0.05 * cinf
    ref = brute_force_l1(X, y, groups=groups, alpha=alpha, eta=eta, big_M=1000)
    assert np.flatnonzero(ref["active"]).tolist() == [0, 3] and np.flatnonzero(ref["coef"]).tolist() == [4, 7]
    assert abs(ref["objective"] + 11.5095) < 1e-4
    est = L1L0(groups=groups, alpha=alpha, eta=eta, big_M=1000).fit(X, y)
    compare(est, ref, X, y, alpha, eta, coefficients=False)


# ---- 3. the two ends: eta = 0 and alpha = 0 ---------------------------------------------------------------------------------
def test_eta_zero_is_regularized_l0_bit_for_bit():
    from sparselm_amd.miqp import L1L0, RegularizedL0

    X, y = draw(40)
    alpha = 1e-2 * float(np.var(y))
    a = L1L0(alpha=alpha, eta=0.0, big_M=50).fit(X, y)
    b = RegularizedL0(alpha=alpha, big_M=50).fit(X, y)
    assert a.coef_.tobytes() == b.coef_.tobytes() and a.solver_info_["objective"] == b.solver_info_["objective"]
    np.testing.assert_array_equal(a.active_groups_, b.active_groups_)
    assert a.solver_info_["proven_optimal"] and a.coef_.any()


def test_alpha_zero_is_a_plain_lasso():
    """Without a price per group every support that holds the lasso's non-zero columns ties: objective and coefficients only."""
    from sparselm_amd.miqp import L1L0

    X, y = draw(40)
    eta = 0.05 * scales(X, y)[1]
    b, value, kkt = solve_support_l1(X, y, np.arange(10), eta)
    assert kkt <= 1e-10 * scales(X, y)[1]
    est = L1L0(alpha=0.0, eta=eta, big_M=1000).fit(X, y)
    info = est.solver_info_
    print(f"lasso value {value:.12e}, engine {info['objective']:.12e}, nodes {info['nodes']} descents {info['descents']}")
    assert info["proven_optimal"] and info["lower_bound"] == info["objective"]
    assert abs(info["objective"] - value) <= OBJ_RTOL * abs(value)
    assert np.max(np.abs(est.coef_ - b)) <= COEF_RTOL * np.max(np.abs(b))
    assert est.active_groups_[np.flatnonzero(b)].all()


# ---- 4. the box ---------------------------------------------------------------------------------------------------------------
def test_big_m_binds():
    from sparselm_amd.miqp import L1L0

    X, y = draw(40)
    var, cinf = scales(X, y)
    alpha, eta = 1e-2 * var, 0.05 * cinf
    assert np.max(np.abs(brute_force_l1(X, y, alpha=alpha, eta=eta, big_M=1000)["coef"])) > 50  # the premise: the box will bind
    ref = brute_force_l1(X, y, alpha=alpha, eta=eta, big_M=50)
    est = L1L0(alpha=alpha, eta=eta, big_M=50).fit(X, y)
    compare(est, ref, X, y, alpha, eta)
    assert np.max(np.abs(est.coef_)) == 50.0 and np.max(np.abs(ref["coef"])) == 50.0


# ---- 5. hierarchy and groups ---------------------------------------------------------------------------------------------------
def test_star_hierarchy():
    """Everything depends on one column the free optimum does not use, halves on two more (reference tests/test_miqp.py:129-149)."""
    from sparselm_amd.miqp import L1L0

    X, y = draw(40)
    p = X.shape[1]
    var, cinf = scales(X, y)
    alpha, eta = 1e-2 * var, 0.05 * cinf
    free = brute_force_l1(X, y, alpha=alpha, eta=eta, big_M=1000)
    out = [j for j in range(p) if not free["active"][j]]
    hub, left, right = out[0], out[1], out[2]
    hierarchy = []
    for i in range(p):
        hierarchy.append([] if i == hub else [hub])
        if 0 < i < p // 2 and i not in (left, hub):
            hierarchy[i].append(left)
        if p // 2 <= i and i not in (right, hub):
            hierarchy[i].append(right)
    ref = brute_force_l1(X, y, alpha=alpha, eta=eta, big_M=1000, hierarchy=hierarchy)
    est = L1L0(alpha=alpha, eta=eta, hierarchy=hierarchy, big_M=1000).fit(X, y)
    compare(est, ref, X, y, alpha, eta)
    assert not np.array_equal(ref["active"], free["active"])  # the hierarchy changed the answer
    for i, parents in enumerate(hierarchy):
        if est.active_groups_[i]:
            assert all(est.active_groups_[q] for q in parents)


def test_groups_of_two_and_three_columns():
    from sparselm_amd.miqp import L1L0

    X, y = draw(40)
    var, cinf = scales(X, y)
    alpha, eta = 1e-2 * var, 0.05 * cinf
    groups = np.array([31, 17, 31, 24, 17, 24, 10, 17, 10, 31])  # sizes 3, 3, 2, 2 under shuffled, unevenly spaced labels
    ref = brute_force_l1(X, y, groups=groups, alpha=alpha, eta=eta, big_M=1000)
    est = L1L0(groups=groups, alpha=alpha, eta=eta, big_M=1000).fit(X, y)
    compare(est, ref, X, y, alpha, eta)
    for lab, active in zip(np.unique(groups), est.active_groups_):
        if not active:
            assert (est.coef_[groups == lab] == 0).all()


# ---- 6. widths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 63, 64])
def test_widths(p):
    """One column carries the signal; alpha is three quarters of what that column gains, so that the reference's own numbers
    close the enumeration at supports of one column (``closed``: q_all + 2 alpha is above the optimum)."""
    from sparselm_amd.miqp import L1L0

    X, y = make_regression(80, p, n_informative=1, noise=1.0, random_state=2)
    cinf = scales(X, y)[1]
    eta = 0.05 * cinf
    single = min(solve_support_l1(X, y, np.array([j]), eta)[1] for j in range(p))
    alpha = 0.75 * abs(single)
    ref = brute_force_l1(X, y, alpha=alpha, eta=eta, big_M=1000, max_size=1)
    assert ref["closed"] and ref["active"].sum() == 1
    est = L1L0(alpha=alpha, eta=eta, big_M=1000).fit(X, y)
    compare(est, ref, X, y, alpha, eta)


def test_65_columns_are_refused_by_the_engine():
    from sparselm_amd.miqp import L1L0

    X, y = make_regression(80, 65, n_informative=5, random_state=2)
    with pytest.raises(NotImplementedError, match="64"):
        L1L0(alpha=1.0, eta=1.0).fit(X, y)


# ---- 7. the node budget ------------------------------------------------------------------------------------------------------
def test_exhausted_budget_keeps_the_incumbent():
    from sparselm_amd.miqp import L1L0

    X, y = make_regression(25, 30, n_informative=10, noise=1.0, random_state=0)
    var, cinf = scales(X, y)
    alpha, eta = 1e-4 * var, 1e-3 * cinf
    est = L1L0(alpha=alpha, eta=eta, big_M=1000, solver_options={"max_nodes": 1000})
    with pytest.warns(ConvergenceWarning):
        est.fit(X, y)
    info = est.solver_info_
    print(info)
    assert not info["proven_optimal"] and info["status"] == "node_budget"
    assert info["lower_bound"] <= info["objective"] and info["nodes"] >= 1000
    at_coef = objective_of_l1(X, y, est.coef_, int(est.active_groups_.sum()), alpha=alpha, eta=eta)
    assert abs(at_coef - info["objective"]) <= 1e-9 * abs(info["objective"])


# ---- 8. determinism -----------------------------------------------------------------------------------------------------------
def test_two_fits_give_identical_coefficients():
    from sparselm_amd.miqp import L1L0

    X, y = make_regression(25, 20, n_informative=10, noise=1.0, random_state=0)
    cinf = scales(X, y)[1]
    fits = [L1L0(alpha=3.0, eta=0.05 * cinf, big_M=1000).fit(X, y) for _ in range(2)]
    assert fits[0].solver_info_["proven_optimal"] and fits[1].solver_info_["proven_optimal"]
    assert fits[0].coef_.tobytes() == fits[1].coef_.tobytes()
    assert fits[0].solver_info_["objective"] == fits[1].solver_info_["objective"]
    np.testing.assert_array_equal(fits[0].active_groups_, fits[1].active_groups_)


# ---- 9. the two routes into the library -------------------------------------------------------------------------------------
def test_ctypes_and_compiled_binding_agree():
    from sparselm_amd import _engine

    if _engine.load_binding() is None:
        pytest.fail("the compiled binding is not built")
    X, y = draw(40)
    var, cinf = scales(X, y)
    eng = _engine.get_engine()
    need = [0] * 10
    need[3] = 1 << 0
    kw = dict(alpha=1e-2 * var, eta_l1=0.05 * cinf, big_M=50.0, need=need)
    with eng.dataset(X, y) as ds:
        a = ds.solve_l0_l1(binding=False, **kw)
        b = ds.solve_l0_l1(binding=True, **kw)
        for route in (False, True):
            with pytest.raises(ValueError):
                ds.solve_l0_l1(alpha=-1.0, eta_l1=1.0, binding=route)
            with pytest.raises(ValueError):
                ds.solve_l0_l1(alpha=1.0, eta_l1=-1.0, binding=route)
            with pytest.raises(ValueError):
                ds.solve_l0_l1(alpha=1.0, eta_l1=float("nan"), binding=route)
        with pytest.raises(ValueError):
            ds.solve_l0_l1(eta_l1=1.0, need=[1 << 10] + [0] * 9, binding=False)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    for key in ("objective", "lower_bound", "proven_optimal", "status", "loss", "seed_objective", "q_all", "launches"):
        assert a[2][key] == b[2][key], key
    assert a[2]["launches"] == 1 and a[2]["descents"] > 0 and b[2]["descents"] > 0
    assert abs(a[2]["loss"] - np.sum((X @ a[0] - y) ** 2) / 80) <= 1e-10 * a[2]["loss"]


# ---- 10. model selection -----------------------------------------------------------------------------------------------------
def test_grid_search_over_eta():
    from sparselm_amd.miqp import L1L0
    from sparselm_amd.model_selection import GridSearchCV

    X, y = draw(40)
    var, cinf = scales(X, y)
    etas = [1e-3 * cinf, 0.05 * cinf, 0.5 * cinf]
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        search = GridSearchCV(L1L0(alpha=1e-2 * var, big_M=1000), {"eta": etas}, cv=4).fit(X, y)
    assert search.best_params_["eta"] in etas
    assert search.best_estimator_.solver_info_["proven_optimal"]
