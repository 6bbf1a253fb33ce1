"""Audit of a path's certificates: every point the engine reports is checked against X itself.

The tail kernel (csrc/tail_kernels.hpp, ``fista_tail_kernel`` / ``fista_tail_stream_kernel``; the rule itself:
csrc/tail_logic.hpp) reports ``u = prox_s(z - s g(z))`` for a base point z, with
``info.kkt = ||G_s(z)||`` (G_s the proximal-gradient mapping) and ``info.L = 1 / s`` -- the inverse step that produced u, in
both schemes (spectral: ``ak``; FISTA: ``L``).  From ``(z - u) / s - g(z) in dh(u)``:

    dist(0, dF(u)) <= ||G_s(z)|| + ||g(u) - g(z)|| <= (1 + L_true s) ||G_s(z)||,      L_true = lambda_max(X^T W X / n).

That holds whatever gradient the engine used, as long as it produced the same proximal mapping as the true one -- which is
all a certified partial pass (csrc/light_kernels.hpp) claims.  A column certified out on a wrong gradient shows up as a
violation of its optimality condition at u that the inequality does not allow, however small it is next to ``max|beta|``.

``dist(0, dF(u))`` is ``oracle.kkt_residual`` with the gradient at u recomputed in float64 -- numpy from the host arrays
(row weights honoured), or a caller's ``gradient(beta)`` (e.g. ``Dataset.gradient`` for device-generated data).

Rounding floor.  The engine's gradient and the one recomputed here are two float64 evaluations of X^T W (X u - y) / n in
different summation orders, and the tail's own stopping rule stops asking for digits below the rounding level of its step:
``kRoundFloor * (||g|| + L ||beta||)`` with ``kRoundFloor`` = 16 ulp (tail_kernels.hpp).  The audit allows the same amount,
``KROUND * (||g(u)|| + L_true ||u||)``, on top of the bound: below it the two gradients themselves disagree.

The second check is self-consistency: ``info.kkt`` meets the acceptance rule the tail applies,

    kkt <= max(tol * max(||u||, floor) * mu, kRoundFloor * (||g(z)|| + Lhat ||u||)),

with ``info.mu`` and ``info.beta_norm`` as reported.  Quantities the record does not carry are bounded from it: the floor
``1e-10 sqrt(2 loss / max(L, Lhat))`` by ``1e-10 sqrt(2 loss / mu)`` (mu <= Lhat and mu <= L in both schemes), ``Lhat`` by
``max(L_true, info.L)``, and ``||g(z)||`` -- the gradient at the last candidate, which need not be u's base -- by four times
``||g(u)|| + L_true ||u||``.
"""

from __future__ import annotations

import numpy as np

import oracle

KROUND = 16.0 * 2.220446049250313e-16  # kRoundFloor of csrc/tail_kernels.hpp
SLM_OK = 0


def lambda_max(X, row_weight=None, n_eff=None, gradient=None, p=None):
    """lambda_max(X^T W X / n): from the Gram on the host, or -- with ``gradient`` only -- by power steps on
    g(v) - g(0) = X^T W X v / n, then 5 % on top.  A power estimate approaches lambda_max from below, and the audit's bound
    grows with L_true: an estimate short of it would make the bound stricter than the engine's rule (a false alarm), one
    above it looser by the same factor at most.  The 5 % covers what 60 steps may still be short by on a spectrum with a
    small top gap and loosens the bound by no more than that -- nothing next to the factors a wrongly certified column
    shows (test_certificate_cpu checks the estimate against eigvalsh)."""
    if X is not None:
        Xw = X if row_weight is None else X * np.sqrt(row_weight)[:, None]
        n = X.shape[0] if n_eff is None else n_eff
        A = Xw.T @ Xw / n
        return float(np.linalg.eigvalsh(A)[-1])
    g0 = gradient(np.zeros(p))
    v = np.random.default_rng(0).standard_normal(p)
    lam = 0.0
    for _ in range(60):
        v /= np.linalg.norm(v)
        w = gradient(v) - g0
        lam = float(np.linalg.norm(w))
        v = w
    return 1.05 * lam


def true_gradients(X, y, B, row_weight=None, n_eff=None):
    """X^T W (X beta - y) / n for every row beta of B, in float64."""
    n = X.shape[0] if n_eff is None else n_eff
    R = X @ B.T - y[:, None]
    if row_weight is not None:
        R = R * row_weight[:, None]
    return (X.T @ R / n).T


def audit_path(res, points, X=None, y=None, a=None, b=None, d=None, groups=None, tol=1e-8, row_weight=None, n_eff=None,
               gradient=None, L_true=None):
    """Check every point of ``res`` (a PathResult, or anything with ``betas`` and the per-point records ``kkt``, ``mu``,
    ``L_points``, ``beta_norm``, ``loss``, ``status``).  ``points``: the (sa, sb, sd) of each point; ``a`` (p,), ``b`` / ``d``
    (G,): the penalty weights (None: ones).  Returns a report: per point the soundness ratio dist / bound and the consistency
    ratio kkt / rule (both <= 1 when certified), and ``failures``, a list of (point, what, value, limit)."""
    B = np.asarray(res.betas, dtype=np.float64)
    K, p = B.shape
    pts = np.asarray(points, dtype=np.float64).reshape(K, 3)
    gidx, G = oracle.group_index(groups, p)
    a = np.ones(p) if a is None else np.broadcast_to(np.asarray(a, dtype=np.float64), (p,))
    b = np.ones(G) if b is None else np.broadcast_to(np.asarray(b, dtype=np.float64), (G,))
    d = np.ones(G) if d is None else np.broadcast_to(np.asarray(d, dtype=np.float64), (G,))
    if L_true is None:
        L_true = lambda_max(X, row_weight, n_eff, gradient, p)
    if gradient is None:
        grads = true_gradients(X, np.asarray(y, dtype=np.float64), B, row_weight, n_eff)
    else:
        grads = np.stack([gradient(B[k]) for k in range(K)])
    kkt, mu, Linv = np.asarray(res.kkt), np.asarray(res.mu), np.asarray(res.L_points)
    bn, loss, status = np.asarray(res.beta_norm), np.asarray(res.loss), np.asarray(res.status)
    rep = dict(L_true=L_true, sound=np.zeros(K), consistent=np.zeros(K), dist=np.zeros(K), failures=[])
    for k in range(K):
        if status[k] != SLM_OK:
            rep["failures"].append((k, "status", int(status[k]), SLM_OK))
            continue
        u, g = B[k], grads[k]
        dist = oracle.kkt_residual(g, u, pts[k, 0] * a, pts[k, 1] * b, pts[k, 2] * d, gidx, G)
        unorm, gnorm = float(np.linalg.norm(u)), float(np.linalg.norm(g))
        s = 1.0 / Linv[k]
        bound = (1.0 + L_true * s) * kkt[k] * (1.0 + 1e-9) + KROUND * (gnorm + L_true * unorm)
        rule = max(tol * max(bn[k], 1e-10 * np.sqrt(2.0 * max(loss[k], 0.0) / mu[k])) * mu[k],
                   KROUND * 4.0 * (gnorm + L_true * unorm + max(L_true, Linv[k]) * bn[k]))
        rep["dist"][k] = dist
        rep["sound"][k] = dist / bound
        rep["consistent"][k] = kkt[k] / rule
        if not dist <= bound:
            rep["failures"].append((k, "soundness", dist, bound))
        if not kkt[k] <= rule * (1.0 + 1e-9):
            rep["failures"].append((k, "self-consistency", float(kkt[k]), rule))
        if not abs(bn[k] - unorm) <= 1e-9 * max(unorm, 1e-300):
            rep["failures"].append((k, "beta_norm", float(bn[k]), unorm))
    return rep


def assert_certified(res, points, **kw):
    """audit_path, and fail with the first few violations."""
    rep = audit_path(res, points, **kw)
    assert not rep["failures"], rep["failures"][:5]
    return rep
