"""Linear constraints on the estimator surface, without a GPU: every solve goes through the CPU oracle
(``_backend.use_backend(OracleBackend())``), so these tests pin the splitting of model/_constrained.py, the public
surface (``constraints=``, ``add_constraints``, validation, ``constraint_multipliers_``) and the maps for the overlap
classes, against an independent Condat-Vu oracle and a KKT certificate."""

import warnings

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint
from sklearn.base import clone

from _constrained_oracle import condat_vu, kkt_constrained, stack
from _oracle_backend import OracleBackend

from sparselm_amd import _backend
from sparselm_amd import model as M
from sparselm_amd.model import (
    AdaptiveGroupLasso,
    AdaptiveLasso,
    AdaptiveSparseGroupLasso,
    GroupLasso,
    Lasso,
    OrdinaryLeastSquares,
    OverlapGroupLasso,
    RidgedGroupLasso,
    SparseGroupLasso,
)
from sparselm_amd.model._lasso import overlap_extension
from sparselm_amd.model_selection import GridSearchCV

ALL = [getattr(M, name) for name in M.__all__]


@pytest.fixture(autouse=True)
def oracle_backend():
    with _backend.use_backend(OracleBackend()):
        yield


@pytest.fixture(scope="module", params=[20, 30])
def random_model(request):
    """The conftest's random models (25 samples, 20 and 30 features, 10 informative, a bias) drawn from a generator of
    this module's own: the package-wide one stays where the other modules' draws expect it."""
    from sklearn.datasets import make_regression

    rng = np.random.default_rng(1000 + request.param)
    X, y, beta = make_regression(n_samples=25, n_features=request.param, n_informative=10, coef=True,
                                 random_state=int(rng.integers(0, 2**32 - 1)), bias=10 * rng.random())
    return X, y, beta


def _constraints(X, y):
    """Bounds (coef[:3] >= 0), one inequality that cuts the least-squares fit off, one equality."""
    p = X.shape[1]
    lb = np.full(p, -np.inf)
    lb[:3] = 0.0
    w = np.random.default_rng(1).standard_normal(p)
    b_ls = np.linalg.lstsq(X, y, rcond=None)[0]
    E = np.zeros((1, p))
    E[0, 3], E[0, 4] = 1.0, -1.0
    return [Bounds(lb, np.inf), LinearConstraint(w[None, :], -np.inf, 0.5 * float(w @ b_ls)), LinearConstraint(E, 0.0, 0.0)]


def _stacked_multipliers(est, cons):
    out = []
    for c, lam in zip(cons, est.constraint_multipliers_):
        lb = np.broadcast_to(np.asarray(c.lb, float), lam.shape)
        ub = np.broadcast_to(np.asarray(c.ub, float), lam.shape)
        out.append(lam[np.isfinite(lb) | np.isfinite(ub)])
    return np.concatenate(out)


def _rel(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


# ---- surface ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ALL, ids=lambda c: c.__name__)
def test_constraints_is_a_parameter_of_every_estimator(cls):
    cons = [Bounds(0.0, np.inf)]
    est = cls(constraints=cons)
    assert est.get_params()["constraints"] is cons
    assert clone(est).get_params()["constraints"] is not None
    other = [LinearConstraint(np.ones((1, 3)), 0.0, 1.0)]
    assert est.set_params(constraints=other).constraints is other
    assert cls().constraints is None


def test_add_constraints_builds_a_new_list():
    mine = [Bounds(0.0, np.inf)]
    est = Lasso(constraints=mine)
    extra = LinearConstraint(np.ones((1, 3)), -np.inf, 1.0)
    assert est.add_constraints(extra) is est
    assert len(mine) == 1 and len(est.constraints) == 2 and est.constraints is not mine
    fresh = Lasso().add_constraints([extra])
    assert fresh.constraints == [extra]


def test_validation_errors():
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((20, 4)), rng.standard_normal(20)

    class CvxpyLike:  # what a cvxpy constraint looks like to the estimator: not a scipy object
        pass

    with pytest.raises(TypeError, match="scipy.optimize"):
        Lasso(alpha=0.1, constraints=[CvxpyLike()]).fit(X, y)
    with pytest.raises(TypeError, match="scipy.optimize"):
        Lasso(alpha=0.1, constraints="beta >= 0").fit(X, y)
    with pytest.raises(ValueError, match="columns"):
        Lasso(alpha=0.1, constraints=LinearConstraint(np.ones((1, 5)), 0.0, 1.0)).fit(X, y)
    with pytest.raises(ValueError, match="lb > ub"):
        Lasso(alpha=0.1, constraints=LinearConstraint(np.ones((2, 4)), [0.0, 2.0], [1.0, 1.0])).fit(X, y)
    bad = np.ones((1, 4))
    bad[0, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        Lasso(alpha=0.1, constraints=LinearConstraint(bad, 0.0, 1.0)).fit(X, y)
    with pytest.raises(ValueError, match="infeasible"):
        Lasso(alpha=0.1, constraints=[Bounds(0.0, np.inf), LinearConstraint(np.ones((1, 4)), -np.inf, -1.0)]).fit(X, y)


def test_sparse_matrix_and_dropped_rows():
    import scipy.sparse as sp

    rng = np.random.default_rng(4)
    X, y = rng.standard_normal((30, 6)), rng.standard_normal(30)
    A = sp.csr_matrix(np.array([[1.0, 1.0, 0, 0, 0, 0], [0, 0, 1.0, 0, 0, 0]]))
    est = Lasso(alpha=0.01, constraints=LinearConstraint(A, [-np.inf, -np.inf], [0.1, np.inf])).fit(X, y)
    assert est.coef_[0] + est.coef_[1] <= 0.1 + 1e-9
    lam = est.constraint_multipliers_[0]
    assert lam.shape == (2,) and lam[1] == 0.0


def test_standardized_sparse_group_lasso_refuses_constraints():
    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((20, 4)), rng.standard_normal(20)
    for cls in (SparseGroupLasso, AdaptiveSparseGroupLasso):
        with pytest.raises(ValueError, match="standardize=True"):
            cls(groups=[0, 0, 1, 1], standardize=True, constraints=Bounds(0.0, np.inf)).fit(X, y)


# ---- solutions against the oracle --------------------------------------------------------------------------------
def _make(name, groups):
    return {
        "OrdinaryLeastSquares": lambda: OrdinaryLeastSquares(),
        "Lasso": lambda: Lasso(alpha=1.0),
        "GroupLasso": lambda: GroupLasso(groups=groups, alpha=2.0),
        "SparseGroupLasso": lambda: SparseGroupLasso(groups=groups, alpha=2.0, l1_ratio=0.5),
        "RidgedGroupLasso": lambda: RidgedGroupLasso(groups=groups, alpha=2.0, delta=(0.5,)),
    }[name]()


@pytest.mark.parametrize("name", ["OrdinaryLeastSquares", "Lasso", "GroupLasso", "SparseGroupLasso", "RidgedGroupLasso"])
def test_plain_estimators_match_the_oracle(random_model, name):
    X, y, _ = random_model
    p = X.shape[1]
    groups = np.arange(p) // 5
    cons = _constraints(X, y)
    est = _make(name, groups).set_params(constraints=cons).fit(X, y)
    assert est.solver_info_["route"] == "host"
    assert est.solver_info_["max_violation"] <= 1e-8 * max(1.0, np.max(np.abs(est.coef_)))
    a, b, d, gidx, G = est._penalty(X)
    penalty = (a, b, d, gidx, G)
    A, lo, hi = stack(cons, p)
    ok, measures = kkt_constrained(X, y, penalty, A, lo, hi, est.coef_, _stacked_multipliers(est, cons))
    assert ok, measures
    if name == "OrdinaryLeastSquares" and p > X.shape[0]:
        return  # (more features than samples: the minimiser is not unique, the certificate is the test)
    ref, _, _ = condat_vu(X, y, penalty, A, lo, hi)
    assert _rel(est.coef_, ref) < 1e-6


def test_overlap_group_lasso_matches_the_oracle(random_model):
    X, y, _ = random_model
    p = X.shape[1]
    group_list = [[j // 4] + ([j // 4 + 1] if j % 4 == 3 else []) for j in range(p)]
    cons = _constraints(X, y)
    est = OverlapGroupLasso(group_list=group_list, alpha=2.0, constraints=cons).fit(X, y)
    bidx, ext = overlap_extension(group_list, p)
    G = int(ext.max()) + 1
    A, lo, hi = stack(cons, p)
    ref_ext, _, _ = condat_vu(X[:, bidx], y, (None, 2.0 * np.ones(G), None, ext, G), A[:, bidx], lo, hi)
    ref = np.bincount(bidx, weights=ref_ext, minlength=p)
    assert _rel(est.coef_, ref) < 1e-6


def test_standardized_group_lasso_is_feasible_and_optimal(random_model):
    """standardize=True: the constraints are mapped onto the per-group change of variables (Design.map_constraints)."""
    X, y, _ = random_model
    p = X.shape[1]
    groups = np.arange(p) // 5
    cons = _constraints(X, y)
    est = GroupLasso(groups=groups, alpha=2.0, standardize=True, constraints=cons).fit(X, y)
    assert est.solver_info_["max_violation"] <= 1e-8 * max(1.0, np.max(np.abs(est.coef_)))
    # the objective of the reference's standardised penalty is not above that of the plain oracle's point
    def objective(b):
        pen = sum(np.linalg.norm(X[:, groups == g] @ b[groups == g]) for g in np.unique(groups))
        return 0.5 / len(y) * np.sum((X @ b - y) ** 2) + 2.0 * pen
    plain = GroupLasso(groups=groups, alpha=2.0, constraints=cons).fit(X, y)
    assert objective(est.coef_) <= objective(plain.coef_) + 1e-9 * abs(objective(plain.coef_))


def _adaptive_oracle(X, y, cons, alpha, rounds, eps, tol, group=None):
    p = X.shape[1]
    A, lo, hi = stack(cons, p)
    if group is None:
        w = alpha * np.ones(p)
    else:
        G = int(group.max()) + 1
        w = alpha * np.ones(G)
    prev = w.copy()
    for _ in range(rounds):
        pen = (w, None, None, None, p) if group is None else (None, w, None, group, G)
        b, _, _ = condat_vu(X, y, pen, A, lo, hi)
        if group is None:
            w = alpha * (alpha / (np.abs(b) + eps))
        else:
            gn = np.sqrt(np.bincount(group, weights=b * b, minlength=G))
            w = alpha * (alpha / (gn + eps))
        if np.linalg.norm(w - prev) <= tol:
            break
        prev = w.copy()
    return b


@pytest.mark.parametrize("grouped", [False, True])
def test_adaptive_estimators_match_the_oracle(random_model, grouped):
    X, y, _ = random_model
    p = X.shape[1]
    cons = _constraints(X, y)
    groups = np.arange(p) // 5
    # (re-weighting multiplies a round's error into the next round's weights -- alpha / (||b_g|| + eps) reaches 4e6 on
    #  a group at zero -- so the rounds are solved to the oracle's own tolerance)
    opts = {"tol": 1e-12}
    if grouped:
        est = AdaptiveGroupLasso(groups=groups, alpha=2.0, max_iter=3, constraints=cons, solver_options=opts).fit(X, y)
    else:
        est = AdaptiveLasso(alpha=1.0, max_iter=3, constraints=cons, solver_options=opts).fit(X, y)
    ref = _adaptive_oracle(X, y, cons, est.alpha, 3, est.eps, est.tol, group=groups if grouped else None)
    assert _rel(est.coef_, ref) < 1e-6
    assert len(est.solver_info_["solves"]) == est.n_iter_


def test_inactive_constraints_reproduce_the_unconstrained_fit(random_model):
    X, y, _ = random_model
    p = X.shape[1]
    free = Lasso(alpha=1.0, solver_options={"tol": 1e-12}).fit(X, y)
    big = 10.0 * np.max(np.abs(free.coef_)) + 1.0
    cons = [Bounds(-big, big), LinearConstraint(np.ones((1, p)), -p * big, p * big)]
    est = Lasso(alpha=1.0, constraints=cons, solver_options={"tol": 1e-12}).fit(X, y)
    assert _rel(est.coef_, free.coef_) < 1e-8
    assert all(np.all(lam == 0.0) for lam in est.constraint_multipliers_)


def test_intercept_and_sample_weight_keep_the_reference_formula(random_model):
    X, y, _ = random_model
    n, p = X.shape
    w = np.random.default_rng(2).uniform(0.5, 2.0, n)
    cons = _constraints(X, y)
    est = Lasso(alpha=1.0, fit_intercept=True, constraints=cons).fit(X, y, sample_weight=w)
    x_off = np.average(X, axis=0, weights=w)
    y_off = np.average(y, weights=w)
    assert abs(est.intercept_ - (y_off - x_off @ est.coef_)) <= 1e-10 * max(1.0, abs(est.intercept_))
    wn = w * (n / w.sum())
    Xc = (X - x_off) * np.sqrt(wn)[:, None]
    yc = (y - y_off) * np.sqrt(wn)
    A, lo, hi = stack(cons, p)
    ref, _, _ = condat_vu(Xc, yc, (np.ones(p), None, None, None, p), A, lo, hi)
    assert _rel(est.coef_, ref) < 1e-6


def test_grid_search_takes_the_generic_route_and_refits_feasibly(random_model):
    X, y, _ = random_model
    cons = _constraints(X, y)
    with _backend.use_backend(_backend.HipBackend()):  # (the gate itself, as the product evaluates it)
        assert GridSearchCV(Lasso(), {"alpha": [0.5, 1.0]})._fast_path_ok({})
        assert not GridSearchCV(Lasso(constraints=cons), {"alpha": [0.5, 1.0]})._fast_path_ok({})
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        search = GridSearchCV(Lasso(constraints=cons), {"alpha": [0.5, 1.0, 2.0]}, cv=3).fit(X, y)
    best = search.best_estimator_
    A, lo, hi = stack(cons, X.shape[1])
    v = A @ best.coef_
    assert np.all(v >= lo - 1e-8 * max(1.0, np.max(np.abs(v)))) and np.all(v <= hi + 1e-8 * max(1.0, np.max(np.abs(v))))


def test_warm_start_starts_from_coef(random_model):
    X, y, _ = random_model
    cons = _constraints(X, y)
    est = Lasso(alpha=1.0, warm_start=True, constraints=cons).fit(X, y)
    first = est.coef_.copy()
    est.fit(X, y)
    assert _rel(est.coef_, first) < 1e-6
