"""The L1L0 profile on the GPU (``sparselm_amd.miqp.l1l0_profile``; ``slm_solve_l0_l1_profile`` and ``_wide``: the L1 + PROFILE
instantiations of csrc/l0_kernels.hpp, narrow and wide) against the per-size brute force of tests/_l1l0_profile_reference.py --
a lasso per admissible support straight from X, every solution's KKT residual asserted -- and against ``L1L0`` itself.

Tolerances are those of tests/test_l1l0_gpu.py (gap >= 1e-6, kappa <= 1e4, objectives to 1e-10, coefficients to 1e-9), per
size, and every premise is asserted on the reference's numbers first.  What is particular to an l1 term: the table
SATURATES -- from the size that holds every column the lasso on all columns uses, larger sizes tie in value and their
supports are not unique.  A row whose gap is >= GAP_MIN is compared in full (support, value, the objective recomputed from X,
coefficients); a saturated row on what is unique (value, size of the support, the objective recomputed from X).  Every test
names the rows that MUST be compared in full, so that it cannot hide behind skipped rows."""

import functools
import os
import warnings

import numpy as np
import pytest
from sklearn.datasets import make_regression
from sklearn.exceptions import ConvergenceWarning

from _l0_reference import search_rank
from _l1l0_profile_reference import profile_table_l1
from _l1l0_reference import brute_force_l1, objective_of_l1
from test_l0_profile_gpu import design
from test_l0_search_gpu import suppressor
from test_l1l0_gpu import COEF_RTOL, GAP_MIN, KAPPA_MAX, OBJ_RTOL, dependent_case

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
WIDE = {"wide": True}


def c_inf(X, y):
    return float(np.max(np.abs(X.T @ y / X.shape[0])))


# ---- designs and references, computed once -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def narrow_table(seed, rel, big_M=1000.0, K=12):
    X, y, _ = design(seed)
    return profile_table_l1(X, y, K=K, eta=rel * c_inf(X, y), big_M=big_M)


@functools.lru_cache(maxsize=None)
def wide_singles():
    X, y, groups, _, _ = suppressor(80, pairs=1, tau=0.3, n=120)
    assert groups is None and X.shape == (120, 80)
    return X, y, 0.05 * c_inf(X, y), search_rank(X, y)


@functools.lru_cache(maxsize=None)
def wide_singles_table(with_hierarchy):
    X, y, eta, rank = wide_singles()
    return profile_table_l1(X, y, K=2, eta=eta, big_M=1000, hierarchy=wide_hierarchy() if with_hierarchy else None)


def wide_hierarchy():
    """the group of search rank 78 needs the group of search rank 3"""
    X, y, eta, rank = wide_singles()
    at = np.argsort(rank)
    hierarchy = [[] for _ in range(80)]
    hierarchy[at[78]] = [int(at[3])]
    return hierarchy


@functools.lru_cache(maxsize=None)
def wide_groups():
    X, y, groups, _, _ = suppressor(10, width=8, pairs=1, tau=0.3, n=160, noise=0.2)
    assert X.shape == (160, 80) and np.linalg.matrix_rank(X) == 80
    eta = 0.02 * c_inf(X, y)
    return X, y, groups, eta, profile_table_l1(X, y, groups=groups, K=3, eta=eta, big_M=1000)


def compare_table(prof, table, X, y, eta, full, fitted=False):
    """Per size: a row whose reference gap is >= GAP_MIN in full, any other row on what is unique.  ``full``: the rows that
    have to be among the former.  ``fitted``: fitted values in place of coefficients (blocks singular by construction)."""
    K = len(table["values"]) - 1
    assert prof.values_.shape == (K + 1,) and prof.supports_.shape == table["actives"].shape and prof.coefs_.shape == table["coefs"].shape
    assert prof.values_[0] == 0.0 and not prof.supports_[0].any() and not prof.coefs_[0].any() and prof.eta_ == eta
    in_full = []
    for k in range(1, K + 1):
        ref_v = table["values"][k]
        print(f"size {k}: reference value {ref_v:.12e} gap {table['gaps'][k]:.3e} kappa {table['kappas'][k]:.3e}; engine {prof.values_[k]:.12e} "
              f"support {np.flatnonzero(prof.supports_[k])}")
        assert np.isfinite(ref_v)
        assert abs(prof.values_[k] - ref_v) <= OBJ_RTOL * abs(ref_v)
        assert prof.supports_[k].sum() == k
        assert abs(objective_of_l1(X, y, prof.coefs_[k], k, eta=eta) - ref_v) <= OBJ_RTOL * abs(ref_v)
        if not table["gaps"][k] >= GAP_MIN:
            continue  # (a tie: the support is not unique)
        in_full.append(k)
        assert fitted or table["kappas"][k] <= KAPPA_MAX
        np.testing.assert_array_equal(prof.supports_[k], table["actives"][k])
        got, want = (X @ prof.coefs_[k], X @ table["coefs"][k]) if fitted else (prof.coefs_[k], table["coefs"][k])
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        assert err <= COEF_RTOL, (k, err)
    print(f"rows compared in full: {in_full}")
    assert set(full) <= set(in_full), (full, in_full)


def assert_finished(prof):
    info = prof.solver_info_
    print(info)
    assert prof.proven_optimal_ and info["proven_optimal"] and info["status"] == "optimal" and info["launches"] == 1 and info["descents"] > 0


# ---- 1. the table against enumeration, narrow ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, rel, full, lasso_nz", [(1, 0.05, range(1, 8), 7), (1, 0.3, range(1, 4), 3), (0, 0.3, range(1, 5), 4)])
def test_table_equals_enumeration(seed, rel, full, lasso_nz):
    from sparselm_amd.miqp import l1l0_profile

    X, y, _ = design(seed)
    eta = rel * c_inf(X, y)
    table = narrow_table(seed, rel)
    # the premise: the rows named are separated (>= 6e-5), the lasso on all columns uses lasso_nz columns, the rest is saturated
    assert (table["gaps"][list(full)] >= 6e-5).all() and table["n_supports"] == 4096
    assert np.count_nonzero(table["coefs"][12]) == lasso_nz == max(full)
    assert (np.abs(table["values"][lasso_nz:] - table["values"][12]) <= 1e-12 * abs(table["values"][12])).all()
    prof = l1l0_profile(X, y, eta=eta, max_groups=12, big_M=1000)
    assert_finished(prof)
    compare_table(prof, table, X, y, eta, full)
    assert prof.alpha_min_ == 0.0 and (prof.intercepts_ == 0.0).all()
    # the bound the search cut with: a lower bound on the lasso on all columns, at or above the quadratic value of all columns
    r_all = X @ np.linalg.lstsq(X, y, rcond=None)[0] - y
    q_all = float(r_all @ r_all - y @ y) / 80
    assert q_all * (1 + 1e-9) <= prof.solver_info_["q_all"] <= table["values"][12] * (1 - 1e-12)
    # best subset under an l1 term: the cardinality-bounded lasso, ties to the smaller size
    for bound in (2, lasso_nz, 12):
        coef, _, active = prof.best_subset(bound)
        k, want = int(active.sum()), table["values"][min(bound, lasso_nz)]
        assert k <= bound and np.array_equal(coef, prof.coefs_[k]) and abs(prof.values_[k] - want) <= OBJ_RTOL * abs(want)
        assert k == bound or bound > lasso_nz  # (below the saturation the values fall strictly: the bound is used up)


# ---- 2. eta changes a row ------------------------------------------------------------------------------------------------------
def test_eta_changes_a_row():
    """Seed 1 at 0.3 ||c||_inf: the best pair is {8, 11} where ``l0_profile``'s is {3, 8} -- an engine that ignored eta fails."""
    from sparselm_amd.miqp import l0_profile, l1l0_profile

    from _l0_profile_reference import profile_table

    X, y, _ = design(1)
    eta = 0.3 * c_inf(X, y)
    table = narrow_table(1, 0.3)
    assert np.flatnonzero(table["actives"][2]).tolist() == [8, 11] and table["gaps"][2] >= 3e-2
    assert np.flatnonzero(profile_table(X, y, K=2, big_M=1000)["actives"][2]).tolist() == [3, 8]
    with_l1 = l1l0_profile(X, y, eta=eta, max_groups=2, big_M=1000)
    without = l0_profile(X, y, max_groups=2, big_M=1000)
    assert np.flatnonzero(with_l1.supports_[2]).tolist() == [8, 11]
    assert np.flatnonzero(without.supports_[2]).tolist() == [3, 8]


# ---- 3. regularized(alpha) is the estimator ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def full_profile(seed, rel):
    from sparselm_amd.miqp import l1l0_profile

    X, y, _ = design(seed)
    return l1l0_profile(X, y, eta=rel * c_inf(X, y), big_M=1000)


@pytest.mark.parametrize("rel_alpha, size", [(1e-4, 6), (1e-2, 3), (0.2, 1)])
def test_regularized_is_the_estimator(rel_alpha, size):
    from sparselm_amd.miqp import L1L0

    X, y, _ = design(1)
    alpha, eta = rel_alpha * float(np.var(y)), 0.05 * c_inf(X, y)
    ref = brute_force_l1(X, y, alpha=alpha, eta=eta, big_M=1000)
    print(f"reference: size {ref['active'].sum()} gap {ref['gap']:.3e} kappa {ref['kappa']:.3e}")
    assert ref["gap"] >= 1e-4 and ref["kappa"] <= KAPPA_MAX and ref["active"].sum() == size
    prof = full_profile(1, 0.05)
    est = L1L0(alpha=alpha, eta=eta, big_M=1000).fit(X, y)
    coef, intercept, active = prof.regularized(alpha)
    np.testing.assert_array_equal(active, ref["active"])
    np.testing.assert_array_equal(active, est.active_groups_)
    assert coef.tobytes() == est.coef_.tobytes() and intercept == est.intercept_ == 0.0
    objective = prof.values_[size] + alpha * size
    assert objective == est.solver_info_["objective"]
    assert abs(objective - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])
    assert abs(objective_of_l1(X, y, coef, size, alpha=alpha, eta=eta) - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])


def test_eta_zero_is_l0_profile_bit_for_bit():
    from sparselm_amd.miqp import l0_profile, l1l0_profile

    X, y, _ = design(1)
    a = l1l0_profile(X, y, eta=0.0, big_M=50)
    b = l0_profile(X, y, big_M=50)
    assert a.values_.tobytes() == b.values_.tobytes() and a.coefs_.tobytes() == b.coefs_.tobytes()
    np.testing.assert_array_equal(a.supports_, b.supports_)
    assert a.proven_optimal_ and a.coefs_[12].all() and a.solver_info_["q_all"] == b.solver_info_["q_all"] and a.eta_ == 0.0


# ---- 4. a pruned table ---------------------------------------------------------------------------------------------------------
def test_pruned_table_is_exact_from_alpha_min_up():
    from sparselm_amd.miqp import l1l0_profile

    X, y, _ = design(1)
    var, eta = float(np.var(y)), 0.05 * c_inf(X, y)
    alpha_min = 1e-3 * var
    prof = l1l0_profile(X, y, eta=eta, alpha_min=alpha_min, big_M=1000)
    full = full_profile(1, 0.05)
    assert_finished(prof)
    print(f"nodes {prof.solver_info_['nodes']} at alpha_min, {full.solver_info_['nodes']} at 0")
    assert prof.alpha_min_ == alpha_min and prof.solver_info_["nodes"] <= full.solver_info_["nodes"]
    sizes = []
    for alpha in (alpha_min, 1e-2 * var, 0.2 * var):
        ref = brute_force_l1(X, y, alpha=alpha, eta=eta, big_M=1000)
        assert ref["gap"] >= GAP_MIN and ref["kappa"] <= KAPPA_MAX
        coef, _, active = prof.regularized(alpha)
        k = int(active.sum())
        sizes.append(k)
        np.testing.assert_array_equal(active, ref["active"])
        assert abs(prof.values_[k] + alpha * k - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])
        assert coef.tobytes() == full.regularized(alpha)[0].tobytes()  # the same support, the same host code
        assert np.max(np.abs(coef - ref["coef"])) <= COEF_RTOL * np.max(np.abs(ref["coef"]))
    print(f"sizes along the alphas: {sizes}")
    assert len(set(sizes)) == 3
    with pytest.raises(ValueError, match="alpha_min"):
        prof.regularized(0.999 * alpha_min)
    with pytest.raises(ValueError, match="alpha_min"):
        prof.best_subset(3)


# ---- 5. grouped columns and a dependent column ---------------------------------------------------------------------------------
def test_dependent_column_inside_a_group():
    """Column 7 = column 0 + column 1, all three in group 0: a row that holds that group puts ONE coefficient on column 7, which
    the pivot rule alone would have left at zero.  Values and fitted values are compared, not coefficients."""
    from sparselm_amd.miqp import l1l0_profile

    X, y, groups = dependent_case()
    eta = 0.05 * c_inf(X, y)
    table = profile_table_l1(X, y, groups=groups, K=6, eta=eta, big_M=1000)
    carried = [k for k in range(1, 7) if table["gaps"][k] >= GAP_MIN and table["actives"][k][0] and table["coefs"][k][7] != 0.0
               and not table["coefs"][k][[0, 1]].any()]
    print(f"rows whose winner holds group 0 with its coefficient on column 7 alone: {carried}")
    assert 1 in carried and 2 in carried  # the premise
    prof = l1l0_profile(X, y, eta=eta, groups=groups, big_M=1000)
    assert_finished(prof)
    compare_table(prof, table, X, y, eta, carried, fitted=True)
    for k in carried:
        assert prof.coefs_[k][7] != 0.0 and not prof.coefs_[k][[0, 1]].any()


# ---- 6. a binding box, an intercept with sample weights, an exhausted budget -------------------------------------------------------
def test_binding_box():
    from sparselm_amd.miqp import l1l0_profile

    X, y, _ = design(0)
    K = 6
    eta = 0.05 * c_inf(X, y)
    free = narrow_table(0, 0.05, K=K)
    big_M = 0.6 * float(np.max(np.abs(free["coefs"][5])))
    table = narrow_table(0, 0.05, big_M=big_M, K=K)
    bound = [k for k in range(1, K + 1) if np.isclose(np.max(np.abs(table["coefs"][k])), big_M, rtol=1e-9, atol=0)]
    print(f"big_M {big_M:.4f}; sizes whose winner sits on the box: {bound}")
    assert 5 in bound and any(table["values"][k] > free["values"][k] * (1 - 1e-6) for k in bound)  # it binds
    assert (table["gaps"][bound] >= GAP_MIN).all()
    prof = l1l0_profile(X, y, eta=eta, max_groups=K, big_M=big_M)
    assert_finished(prof)
    compare_table(prof, table, X, y, eta, bound)
    assert np.max(np.abs(prof.coefs_)) <= big_M


def test_intercept_and_sample_weight():
    from sparselm_amd.miqp import L1L0, l1l0_profile

    X, y, _ = design(0)
    X, y = X + 3.0, y + 10.0
    w = np.random.default_rng(5).uniform(0.5, 2.0, 40)
    K = 4
    wn = w * (40 / w.sum())
    xm, ym = np.average(X, axis=0, weights=wn), np.average(y, weights=wn)
    Xp, yp = (X - xm) * np.sqrt(wn)[:, None], (y - ym) * np.sqrt(wn)
    eta = 0.05 * c_inf(Xp, yp)
    table = profile_table_l1(Xp, yp, K=K, eta=eta, big_M=1000)
    assert (table["gaps"][1:] >= GAP_MIN).all()
    prof = l1l0_profile(X, y, eta=eta, max_groups=K, big_M=1000, fit_intercept=True, sample_weight=w)
    assert_finished(prof)
    compare_table(prof, table, Xp, yp, eta, range(1, K + 1))
    for k in range(K + 1):
        assert abs(prof.intercepts_[k] - (ym - xm @ table["coefs"][k])) <= 1e-9 * max(1.0, abs(ym))
    alpha = 1.5 * float(table["values"][2] - table["values"][3])  # (above what the third column gains: a size below 3)
    est = L1L0(alpha=alpha, eta=eta, big_M=1000, fit_intercept=True).fit(X, y, sample_weight=w)
    coef, intercept, active = prof.regularized(alpha)
    assert 1 <= active.sum() <= 2
    assert coef.tobytes() == est.coef_.tobytes() and intercept == est.intercept_ and np.array_equal(active, est.active_groups_)


def test_exhausted_budget_keeps_the_incumbents():
    from sparselm_amd.miqp import l1l0_profile

    X, y = make_regression(25, 30, n_informative=10, noise=1.0, random_state=0)
    K = 15
    eta = 0.05 * c_inf(X, y)
    with pytest.warns(ConvergenceWarning):
        prof = l1l0_profile(X, y, eta=eta, max_groups=K, big_M=1000, solver_options={"max_nodes": 1000})
    info = prof.solver_info_
    print(info)
    assert not prof.proven_optimal_ and not info["proven_optimal"] and info["status"] == "node_budget" and info["nodes"] >= 1000
    assert np.isfinite(prof.values_).all()  # every size has its seed at the least
    for k in range(K + 1):
        assert prof.supports_[k].sum() == k and np.count_nonzero(prof.coefs_[k]) <= k
        at_coef = objective_of_l1(X, y, prof.coefs_[k], k, eta=eta)
        # (n < p: the Gram's value and the one from X differ by the rounding of a singular Gram -- the bound of the l0 profile's test)
        assert abs(at_coef - prof.values_[k]) <= 1e-9 * max(abs(prof.values_[k]), np.finfo(float).tiny)
    assert (np.diff(prof.values_[:4]) < 0).all()


# ---- 7. the wide kernel on a narrow problem --------------------------------------------------------------------------------------
def test_wide_kernel_gives_the_narrow_bytes_by_both_routes():
    from sparselm_amd import _engine

    if _engine.load_binding() is None:
        pytest.fail("the compiled binding is not built")
    X, y, _ = design(1)
    eta = 0.05 * c_inf(X, y)
    need = [0] * 12
    need[5] = 1 << 2  # (a hierarchy too: group 5 needs group 2)
    results = []
    with _engine.get_engine().dataset(X, y) as ds:
        for wide in (False, True):
            for route in (False, True):
                solve = ds.solve_l0_l1_profile_wide if wide else ds.solve_l0_l1_profile
                results.append(solve(alpha_min=0.0, max_groups=12, eta_l1=eta, big_M=1000.0, need=need, binding=route))
        for route in (False, True):
            with pytest.raises(ValueError):
                ds.solve_l0_l1_profile(eta_l1=-1.0, binding=route)
            with pytest.raises(ValueError):
                ds.solve_l0_l1_profile_wide(eta_l1=np.inf, binding=route)
            with pytest.raises(ValueError):
                ds.solve_l0_l1_profile(alpha_min=-1.0, eta_l1=eta, binding=route)
            with pytest.raises(ValueError):
                ds.solve_l0_l1_profile(eta_l1=eta, need=[1 << 12] + [0] * 11, binding=route)
    betas, masks, values, info = results[0]
    assert info["proven_optimal"] and info["descents"] > 0 and np.isfinite(values).all()
    assert all((int(m) >> 5) & 1 == 0 or (int(m) >> 2) & 1 for m in masks)
    for other in results[1:]:
        assert other[0].tobytes() == betas.tobytes() and other[2].tobytes() == values.tobytes()
        assert [int(m) for m in other[1]] == [int(m) for m in masks]
        assert other[3]["proven_optimal"] and other[3]["q_all"] == info["q_all"]


# ---- 8., 9. more than 64 singleton groups ------------------------------------------------------------------------------------------
def test_more_than_64_singletons():
    from sparselm_amd.miqp import l1l0_profile

    X, y, eta, rank = wide_singles()
    table = wide_singles_table(False)
    ranks = [np.sort(rank[np.flatnonzero(table["actives"][k])]).tolist() for k in (1, 2)]
    print(f"supports {table['n_supports']}, gaps {table['gaps'][1:]}, search ranks of the winners {ranks}")
    # the premise: row 2 lies wholly beyond the first mask word and the first state slot
    assert table["n_supports"] == 3241 and ranks == [[0], [78, 79]] and table["gaps"][1] >= 1e-2 and table["gaps"][2] >= 0.5
    prof = l1l0_profile(X, y, eta=eta, max_groups=2, big_M=1000, solver_options=WIDE)
    assert_finished(prof)
    compare_table(prof, table, X, y, eta, (1, 2))


def test_hierarchy_across_the_word_boundary():
    from sparselm_amd.miqp import l1l0_profile

    X, y, eta, rank = wide_singles()
    hierarchy = wide_hierarchy()
    table = wide_singles_table(True)
    ranks = [np.sort(rank[np.flatnonzero(table["actives"][k])]).tolist() for k in (1, 2)]
    print(f"supports {table['n_supports']}, gaps {table['gaps'][1:]}, search ranks of the winners {ranks}")
    # the premise: the hierarchy takes {78, 79} away; an engine that dropped the high word of a need mask keeps it
    assert ranks == [[0], [2, 8]] and table["gaps"][2] >= 1e-2
    prof = l1l0_profile(X, y, eta=eta, max_groups=2, big_M=1000, hierarchy=hierarchy, solver_options=WIDE)
    assert_finished(prof)
    compare_table(prof, table, X, y, eta, (1, 2))


# ---- 10. wide groups -------------------------------------------------------------------------------------------------------------
def test_wide_groups():
    from sparselm_amd.miqp import l1l0_profile

    X, y, groups, eta, table = wide_groups()
    supports = [np.flatnonzero(table["actives"][k]).tolist() for k in (1, 2, 3)]
    nonzero = [int(np.count_nonzero(table["coefs"][k])) for k in (1, 2, 3)]
    print(f"supports {supports}, non-zero coefficients {nonzero}, gaps {table['gaps'][1:]}")
    assert supports == [[3], [0, 8], [0, 6, 8]] and nonzero == [8, 16, 24] and (table["gaps"][1:] >= 1e-3).all()  # the premise
    with pytest.raises(NotImplementedError, match="64"):  # nine groups of eight columns: a support would not fit
        l1l0_profile(X, y, eta=eta, groups=groups, max_groups=9, big_M=1000, solver_options=WIDE)
    prof = l1l0_profile(X, y, eta=eta, groups=groups, max_groups=3, big_M=1000, solver_options=WIDE)
    assert_finished(prof)
    compare_table(prof, table, X, y, eta, (1, 2, 3))
    eight = l1l0_profile(X, y, eta=eta, groups=groups, max_groups=8, big_M=1000, solver_options=WIDE)
    assert_finished(eight)
    for k in (1, 2, 3):  # (the same rows, whatever the bound)
        assert eight.values_[k] == prof.values_[k] and np.array_equal(eight.supports_[k], prof.supports_[k])
    assert (np.diff(eight.values_) <= 0).all() and all(eight.supports_[k].sum() == k for k in range(9))


# ---- 11. the reference's own data: 290 x 66 --------------------------------------------------------------------------------------
def test_reference_data_66_columns():
    from sparselm_amd.miqp import l1l0_profile

    X = np.load(os.path.join(ROOT, "tests", "golden", "reference_examples", "corr.npy"))
    y = np.load(os.path.join(ROOT, "tests", "golden", "reference_examples", "energy.npy"))
    assert X.shape == (290, 66)
    alpha_min, eta = 3.16e-7, 1.66e-6
    profs = []
    for _ in range(2):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", ConvergenceWarning)
            # (max_groups: one size per lane in wide mode, 64 at the most)
            profs.append(l1l0_profile(X, y, eta=eta, alpha_min=alpha_min, max_groups=64, fit_intercept=True,
                                      solver_options={"wide": True, "max_nodes": 2**22}))
    prof = profs[0]
    info = prof.solver_info_
    filled = np.flatnonzero(np.isfinite(prof.values_))
    print(info, f"filled rows {len(filled)} of {len(prof.values_)}")
    Xc, yc = X - X.mean(axis=0), y - y.mean()
    assert len(filled) >= 2 and filled[0] == 0
    for k in filled[1:]:
        assert prof.supports_[k].sum() == k and np.isfinite(prof.coefs_[k]).all()
        at_coef = objective_of_l1(Xc, yc, prof.coefs_[k], k, eta=eta)
        assert abs(at_coef - prof.values_[k]) <= OBJ_RTOL * abs(prof.values_[k]), (k, at_coef, prof.values_[k])
    assert info["q_all"] <= np.min(prof.values_[filled] + alpha_min * filled)
    assert profs[0].values_.tobytes() == profs[1].values_.tobytes() and profs[0].coefs_.tobytes() == profs[1].coefs_.tobytes()
    assert np.array_equal(profs[0].supports_, profs[1].supports_)
    assert profs[0].intercepts_.tobytes() == profs[1].intercepts_.tobytes()


def test_65_columns_without_the_option_point_to_it():
    from sparselm_amd.miqp import l1l0_profile

    X, y = make_regression(80, 65, n_informative=5, random_state=2)
    with pytest.raises(NotImplementedError, match="64.*wide"):
        l1l0_profile(X, y, eta=0.1, max_groups=1)
    prof = l1l0_profile(X, y, eta=0.05 * c_inf(X, y), max_groups=1, big_M=1000, solver_options=WIDE)
    # one column alone is a closed form: f({j}) = -1/2 (|c_j| - eta)_+^2 / G_jj
    c, g = X.T @ y / 80, np.einsum("ij,ij->j", X, X) / 80
    single = -0.5 * np.maximum(np.abs(c) - 0.05 * c_inf(X, y), 0.0) ** 2 / g
    j = int(np.argmin(single))
    assert np.sort(single)[1] - single[j] >= GAP_MIN * abs(single[j])
    assert prof.proven_optimal_ and prof.supports_[1].sum() == 1 and prof.supports_[1][j]
    assert abs(prof.values_[1] - single[j]) <= OBJ_RTOL * abs(single[j])
