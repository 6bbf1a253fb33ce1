"""Linear constraints on the GPU: the one-launch splitting of ``slm_solve_constrained`` on the reference's
cluster-expansion data, its agreement with the host sweeps, the hand-over to them outside the kernel's scope, the group
classes, the warm re-weighting rounds, a design the general engine takes, and the ABI's argument checks."""

import ctypes as C
import os
import warnings

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint

from _constrained_oracle import condat_vu, kkt_constrained, stack

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _ce_problem():
    """The reference's plot_chull.py data (290 x 66) with non-negativity on the first coefficients, 100 hull-like
    inequalities (a structure's prediction at least eps below the mean of two others) and one equality."""
    X = np.load(os.path.join(HERE, "golden", "reference_examples", "corr.npy"))
    y = np.load(os.path.join(HERE, "golden", "reference_examples", "energy.npy"))
    n, p = X.shape
    rng = np.random.default_rng(7)
    rows = rng.choice(100, 100, replace=False)
    others = rng.integers(150, n, (100, 2))
    H = X[rows] - 0.5 * (X[others[:, 0]] + X[others[:, 1]])
    lb = np.full(p, -np.inf)
    lb[:5] = 0.0
    E = np.zeros((1, p))
    E[0, 6], E[0, 7] = 1.0, -1.0
    cons = [Bounds(lb, np.inf), LinearConstraint(H, -np.inf, -1e-3), LinearConstraint(E, 0.0, 0.0)]
    alpha = 1e-2 * np.max(np.abs(X.T @ y)) / n
    return X, y, cons, alpha


def _stacked_multipliers(est, cons, p):
    out = []
    for c, lam in zip(cons, est.constraint_multipliers_):
        lb = np.broadcast_to(np.asarray(c.lb, float), lam.shape)
        ub = np.broadcast_to(np.asarray(c.ub, float), lam.shape)
        out.append(lam[np.isfinite(lb) | np.isfinite(ub)])
    return np.concatenate(out)


def _certify(est, X, y, cons, penalty, rtol=1e-6):
    A, lo, hi = stack(cons, X.shape[1])
    ok, measures = kkt_constrained(X, y, penalty, A, lo, hi, est.coef_, _stacked_multipliers(est, cons, X.shape[1]), rtol=rtol)
    assert ok, measures
    return A, lo, hi


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def test_on_chip_lasso_on_the_ce_fixture():
    from sparselm_amd.model import Lasso

    X, y, cons, alpha = _ce_problem()
    p = X.shape[1]
    est = Lasso(alpha=alpha, constraints=cons).fit(X, y)
    assert est.solver_info_["route"] == "on_chip"
    assert est.solver_info_["launches"] == 1
    assert est.solver_info_["max_violation"] <= 1e-8
    penalty = (alpha * np.ones(p), None, None, None, p)
    A, lo, hi = _certify(est, X, y, cons, penalty)
    ref, _, _ = condat_vu(X, y, penalty, A, lo, hi)
    assert _rel(est.coef_, ref) < 1e-6


def test_on_chip_adaptive_lasso_on_the_ce_fixture():
    from sparselm_amd.model import AdaptiveLasso

    X, y, cons, alpha = _ce_problem()
    p = X.shape[1]
    est = AdaptiveLasso(alpha=alpha, max_iter=3, constraints=cons).fit(X, y)
    assert est.solver_info_["route"] == "on_chip"
    assert all(s.get("launches") == 1 for s in est.solver_info_["solves"])
    A, lo, hi = stack(cons, p)
    # the oracle's rounds: the reference's loop (_adaptive_lasso.py:206-232) over constrained solves
    w = alpha * np.ones(p)
    prev = w.copy()
    for _ in range(3):
        b, lam, _ = condat_vu(X, y, (w, None, None, None, p), A, lo, hi)
        last_w = w
        w = alpha * (alpha / (np.abs(b) + est.eps))
        if np.linalg.norm(w - prev) <= est.tol:
            break
        prev = w.copy()
    ok, measures = kkt_constrained(X, y, (last_w, None, None, None, p), A, lo, hi, est.coef_, _stacked_multipliers(est, cons, p))
    assert ok, measures
    assert _rel(est.coef_, b) < 1e-6


def test_on_chip_and_host_routes_agree():
    from sparselm_amd.model import Lasso, OrdinaryLeastSquares

    X, y, cons, alpha = _ce_problem()
    chip = Lasso(alpha=alpha, constraints=cons).fit(X, y)
    host = Lasso(alpha=alpha, constraints=cons, solver_options={"on_chip": False}).fit(X, y)
    assert chip.solver_info_["route"] == "on_chip" and host.solver_info_["route"] == "host"
    assert _rel(chip.coef_, host.coef_) < 1e-6
    ols_chip = OrdinaryLeastSquares(constraints=cons).fit(X, y)
    ols_host = OrdinaryLeastSquares(constraints=cons, solver_options={"on_chip": False}).fit(X, y)
    assert ols_chip.solver_info_["route"] == "on_chip"
    assert _rel(ols_chip.coef_, ols_host.coef_) < 1e-6


def _feasible_problem(n, p, m):
    """Dense-ish Lasso data with m rows A b <= hi that half the least-squares fit satisfies -- a quarter of them with no
    slack -- and row 0 an equality."""
    rng = np.random.default_rng(1000 * n + 10 * p + m)
    X = rng.standard_normal((n, p))
    beta = np.where(rng.random(p) < 0.3, rng.standard_normal(p), 0.0)
    y = X @ beta + 0.1 * rng.standard_normal(n)
    A = rng.standard_normal((m, p)) / np.sqrt(p)
    b_feas = 0.5 * np.linalg.lstsq(X, y, rcond=None)[0]
    slack = np.where(rng.random(m) < 0.25, 0.0, rng.uniform(0.05, 1.0, m))
    slack[0] = 0.0  # (the equality goes through the feasible point)
    hi = A @ b_feas + slack
    lo = np.full(m, -np.inf)
    lo[0] = hi[0]
    alpha = 0.02 * np.max(np.abs(X.T @ y)) / n
    return X, y, [LinearConstraint(A, lo, hi)], alpha


# p = 64 fills a lane's first position, 65 is the first with a second, 128 the widest; m = 64 / 65 is the step to a second
# constraint row per lane, 512 the most
@pytest.mark.parametrize("n,p,m", [(40, 5, 1), (160, 64, 64), (160, 65, 65), (300, 128, 512), (160, 65, 1), (40, 5, 65)])
def test_on_chip_lasso_where_the_kernel_changes_path(n, p, m):
    from sparselm_amd.model import Lasso

    X, y, cons, alpha = _feasible_problem(n, p, m)
    chip = Lasso(alpha=alpha, constraints=cons).fit(X, y)
    assert chip.solver_info_["route"] == "on_chip"
    assert chip.solver_info_["launches"] == 1
    _certify(chip, X, y, cons, (alpha * np.ones(p), None, None, None, p))
    host = Lasso(alpha=alpha, constraints=cons, solver_options={"on_chip": False}).fit(X, y)
    assert host.solver_info_["route"] == "host"
    print(f"({n}, {p}, {m}): chip vs host {_rel(chip.coef_, host.coef_):.3e}")
    assert _rel(chip.coef_, host.coef_) < 1e-6


def _abi_call(ds, A, lo, hi, a=None):
    from sparselm_amd import _engine

    lib = _engine.load_library()
    A = np.ascontiguousarray(A, dtype=np.float64)
    m, p = A.shape
    a = np.full(p, 0.1) if a is None else a
    lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
    beta, lam = np.zeros(p), np.zeros(m)
    opts = _engine._SolveOpts(1e-10, 0, 0, 0.0, 0)
    info = np.zeros(1, dtype=_engine._INFO_DTYPE)
    return lib.slm_solve_constrained(ds._h, a.ctypes.data, A.ctypes.data, int(m), lo.ctypes.data, hi.ctypes.data,
                                     C.byref(opts), 0.0, 0, None, 0, beta.ctypes.data, lam.ctypes.data,
                                     info.ctypes.data_as(C.POINTER(_engine._PointInfo)))


@pytest.mark.parametrize("case", ["p129", "m513", "n_ld"])
def test_outside_the_kernel_scope_hands_over_to_the_host_route(case):
    from sparselm_amd import _engine
    from sparselm_amd.model import Lasso

    rng = np.random.default_rng(3)
    n, p, m = {"p129": (200, 129, 10), "m513": (100, 20, 513), "n_ld": (5000, 20, 10)}[case]
    X = rng.standard_normal((n, p))
    y = X @ rng.standard_normal(p) + 0.1 * rng.standard_normal(n)
    A = rng.standard_normal((m, p))
    lo, hi = np.full(m, -np.inf), np.abs(A @ np.linalg.lstsq(X, y, rcond=None)[0]) * 0.5 + 1.0
    lo[0] = hi[0] = 0.0  # one equality
    with _engine.get_engine(0).dataset(X, y) as ds:
        assert _abi_call(ds, A, lo, hi) == _engine.SLM_ERR_UNSUPPORTED
    alpha = 0.05 * np.max(np.abs(X.T @ y)) / n
    cons = [LinearConstraint(A, lo, hi)]
    est = Lasso(alpha=alpha, constraints=cons).fit(X, y)
    assert est.solver_info_["route"] == "host"
    _certify(est, X, y, cons, (alpha * np.ones(p), None, None, None, p))


@pytest.mark.parametrize("cls", ["GroupLasso", "SparseGroupLasso", "RidgedGroupLasso"])
def test_group_classes_certify_through_the_host_route(cls):
    from sparselm_amd import model

    rng = np.random.default_rng(11)
    n, p = 60, 24
    X = rng.standard_normal((n, p))
    y = X @ rng.standard_normal(p) + 0.1 * rng.standard_normal(n)
    groups = np.repeat(np.arange(6), 4)
    lb = np.full(p, -np.inf)
    lb[:6] = 0.0
    cons = [Bounds(lb, np.inf), LinearConstraint(np.ones((1, p)), -np.inf, 0.5), LinearConstraint(np.eye(p)[[8]] - np.eye(p)[[9]], 0.0, 0.0)]
    kw = {"delta": (0.5,)} if cls == "RidgedGroupLasso" else {}
    est = getattr(model, cls)(groups=groups, alpha=0.05, constraints=cons, **kw).fit(X, y)
    assert est.solver_info_["route"] == "host"
    a, b, d, gidx, G = est._penalty(X)
    _certify(est, X, y, cons, (a, b, d, gidx, G))


def test_warm_adaptive_rounds_match_cold_solves():
    from sparselm_amd.model import AdaptiveLasso
    from sparselm_amd.model._constrained import ConstrainedProblem

    X, y, cons, alpha = _ce_problem()
    p = X.shape[1]
    est = AdaptiveLasso(alpha=alpha, max_iter=3, tol=0.0, constraints=cons).fit(X, y)
    A, lo, hi = stack(cons, p)
    w = alpha * np.ones(p)
    for _ in range(3):
        prob = ConstrainedProblem(X, y, None, p, A, lo, hi, {})
        try:
            b, _, info = prob.solve(w, None, None)
        finally:
            prob.close()
        assert info["route"] == "on_chip"
        w = alpha * (alpha / (np.abs(b) + est.eps))
    assert est.n_iter_ == 3
    assert _rel(est.coef_, b) < 1e-6


def test_general_engine_design_certifies():
    from sparselm_amd.model import Lasso

    rng = np.random.default_rng(5)
    n, p, m = 20000, 400, 50
    X = rng.standard_normal((n, p))
    beta = np.zeros(p)
    beta[:40] = rng.standard_normal(40)
    y = X @ beta + 0.5 * rng.standard_normal(n)
    A = rng.standard_normal((m, p))
    b_ls = np.linalg.lstsq(X, y, rcond=None)[0]
    hi = A @ b_ls - 0.2 * np.abs(A @ b_ls) - 0.05  # every row cuts the unconstrained fit off: some of them bind
    cons = [LinearConstraint(A, -np.inf, hi)]
    alpha = 0.02 * np.max(np.abs(X.T @ y)) / n
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # (the sweeps converge: no ConvergenceWarning)
        est = Lasso(alpha=alpha, constraints=cons).fit(X, y)
    assert est.solver_info_["route"] == "host"
    assert np.sum(np.abs(est.constraint_multipliers_[0]) > 0) > 0
    _certify(est, X, y, cons, (alpha * np.ones(p), None, None, None, p))


def test_bad_arguments_are_refused_before_any_launch():
    from sparselm_amd import _engine

    rng = np.random.default_rng(2)
    X = rng.standard_normal((50, 8))
    y = rng.standard_normal(50)
    A = rng.standard_normal((3, 8))
    with _engine.get_engine(0).dataset(X, y) as ds:
        bad = A.copy()
        bad[1, 2] = np.nan
        assert _abi_call(ds, bad, np.zeros(3) - 1, np.ones(3)) == _engine.SLM_ERR_BAD_ARG
        assert _abi_call(ds, A, np.array([0.0, 2.0, 0.0]), np.array([1.0, 1.0, 1.0])) == _engine.SLM_ERR_BAD_ARG
        # and a good call on the same dataset afterwards runs
        assert _abi_call(ds, A, np.full(3, -np.inf), np.full(3, 0.5)) == _engine.SLM_OK
