"""The certificate audit (tests/_certificate.py) on its own: a converged oracle.fista solution reported the way the tail kernel
reports a point passes; the same report with a near-threshold coefficient or an active group wrongly left at zero fails."""

from types import SimpleNamespace

import numpy as np

import oracle
from _certificate import audit_path, lambda_max

TOL = 1e-8


def _report(X, y, B, points, groups=None):
    """Records as the tail writes them: u = prox_s(beta - s g(beta)) with s = 1 / L_true, kkt = ||G_s(beta)||, mu = the
    smallest eigenvalue of X^T X / n."""
    n, p = X.shape
    gidx, G = oracle.group_index(groups, p)
    ev = np.linalg.eigvalsh(X.T @ X / n)
    L, mu = float(ev[-1]), float(ev[0])
    U, kkt = np.empty_like(B), np.empty(len(B))
    for k, (beta, (sa, sb, sd)) in enumerate(zip(B, points)):
        g = X.T @ (X @ beta - y) / n
        U[k] = oracle.prox(beta - g / L, 1.0 / L, sa * np.ones(p), sb * np.ones(G), sd * np.ones(G), gidx, G)
        kkt[k] = np.linalg.norm(beta - U[k]) * L
    loss = np.array([0.5 * np.mean((X @ u - y) ** 2) for u in U])
    return SimpleNamespace(betas=U, kkt=kkt, mu=np.full(len(B), mu), L_points=np.full(len(B), L),
                           beta_norm=np.linalg.norm(U, axis=1), loss=loss, status=np.zeros(len(B), dtype=np.int64))


def _lasso():
    rng = np.random.default_rng(3)
    n, p = 400, 60
    X = rng.standard_normal((n, p))
    beta = np.zeros(p)
    beta[:8] = rng.uniform(0.5, 3.0, 8) * rng.choice([-1.0, 1.0], 8)
    y = X @ beta + 0.5 * rng.standard_normal(n)
    amax = float(np.max(np.abs(X.T @ y)) / n)
    points = [(a, 0.0, 0.0) for a in (0.5 * amax, 0.05 * amax)]
    gidx, G = oracle.group_index(None, p)
    B = np.stack([oracle.fista(X, y, sa, 0.0, 0.0, gidx, G, tol=1e-14)[0] for sa, _, _ in points])
    return X, y, B, points


def test_a_converged_solution_passes():
    X, y, B, points = _lasso()
    res = _report(X, y, B, points)
    rep = audit_path(res, points, X=X, y=y, tol=TOL)
    assert not rep["failures"], rep["failures"]
    assert np.all(rep["sound"] <= 1.0) and np.all(rep["consistent"] <= 1.0)
    assert abs(rep["L_true"] - lambda_max(X)) == 0.0


def test_a_near_threshold_column_forced_to_zero_fails():
    X, y, B, points = _lasso()
    res = _report(X, y, B, points)
    k = 1
    on = np.flatnonzero(res.betas[k])
    j = on[np.argmin(np.abs(res.betas[k][on]))]  # the smallest coefficient: the column closest to its threshold
    assert abs(res.betas[k][j]) < 0.2 * np.max(np.abs(res.betas[k]))
    res.betas[k][j] = 0.0  # (the record -- kkt, beta_norm up to a rounding -- as it was: certified out on a wrong gradient)
    res.beta_norm[k] = np.linalg.norm(res.betas[k])
    rep = audit_path(res, points, X=X, y=y, tol=TOL)
    assert [f[:2] for f in rep["failures"]] == [(k, "soundness")], rep["failures"]
    assert rep["sound"][k] > 1e3


def test_a_group_wrongly_left_at_zero_fails():
    rng = np.random.default_rng(5)
    n, p, gs = 500, 48, 4
    G = p // gs
    groups = np.repeat(np.arange(G), gs)
    X = rng.standard_normal((n, p))
    beta = np.zeros(p)
    beta[groups == 2] = rng.uniform(1.0, 2.0, gs)
    beta[groups == 7] = -rng.uniform(0.2, 0.6, gs)
    y = X @ beta + 0.5 * rng.standard_normal(n)
    g0 = X.T @ y / n
    bmax = float(np.max(np.sqrt(np.bincount(groups, weights=g0 * g0, minlength=G))))
    points = [(0.3 * 0.1 * bmax, 0.7 * 0.1 * bmax, 0.0)]
    gidx, Gn = oracle.group_index(groups, p)
    B = np.stack([oracle.fista(X, y, sa, sb, sd, gidx, Gn, tol=1e-14)[0] for sa, sb, sd in points])
    res = _report(X, y, B, points, groups)
    assert not audit_path(res, points, X=X, y=y, groups=groups, tol=TOL)["failures"]
    norms = np.sqrt(np.bincount(groups, weights=res.betas[0] ** 2, minlength=G))
    active = np.flatnonzero(norms)
    assert len(active) >= 2
    gz = active[np.argmin(norms[active])]
    res.betas[0][groups == gz] = 0.0
    res.beta_norm[0] = np.linalg.norm(res.betas[0])
    rep = audit_path(res, points, X=X, y=y, groups=groups, tol=TOL)
    assert [f[:2] for f in rep["failures"]] == [(0, "soundness")], rep["failures"]


def test_row_weights_enter_the_gradient_and_the_curvature():
    """A fold mask: the audit of a solution of the masked problem passes with the mask and fails without it."""
    X, y, _, points = _lasso()
    n, p = X.shape
    mask = (np.arange(n) % 4 != 0).astype(float)
    ne = int(mask.sum())
    keep = mask > 0
    gidx, G = oracle.group_index(None, p)
    B = np.stack([oracle.fista(X[keep], y[keep], sa, 0.0, 0.0, gidx, G, tol=1e-14)[0] for sa, _, _ in points])
    res = _report(X[keep], y[keep], B, points)
    assert abs(lambda_max(X, mask, ne) - lambda_max(X[keep])) <= 1e-12 * lambda_max(X[keep])
    assert not audit_path(res, points, X=X, y=y, row_weight=mask, n_eff=ne, tol=TOL)["failures"]
    assert audit_path(res, points, X=X, y=y, tol=TOL)["failures"]


def test_a_caller_gradient_and_power_steps_give_the_same_verdicts():
    """audit_path(gradient=...) -- how device-generated data are audited, through Dataset.gradient -- with lambda_max from
    power steps: the estimate lies within [lambda_max, 1.05 lambda_max], and the verdicts are those of the host arrays."""
    X, y, B, points = _lasso()
    n, p = X.shape

    def grad(beta):
        return X.T @ (X @ beta - y) / n

    lam = lambda_max(X)
    est = lambda_max(None, gradient=grad, p=p)
    assert lam <= est <= 1.05 * lam * (1 + 1e-12)
    res = _report(X, y, B, points)
    assert not audit_path(res, points, gradient=grad, tol=TOL)["failures"]
    res.betas[1][np.flatnonzero(res.betas[1])[-1]] = 0.0
    res.beta_norm[1] = np.linalg.norm(res.betas[1])
    host = audit_path(res, points, X=X, y=y, tol=TOL, L_true=est)["failures"]
    dev = audit_path(res, points, gradient=grad, tol=TOL)["failures"]
    assert [f[:2] for f in dev] == [f[:2] for f in host] == [(1, "soundness")]
