"""CPU oracle for linearly constrained fits: ``1/(2n)||X b - y||^2 + penalty(b)`` subject to ``lo <= A b <= hi``.

Independent of the splitting in ``sparselm_amd/model/_constrained.py``: the Condat-Vu primal-dual iteration, with the
constraint as the indicator of a box on ``A b`` whose conjugate's prox comes from Moreau's identity,

    b+      = prox_{tau g}(b - tau (grad f(b) + A^T lam))
    lam+    = z - sigma clip(z / sigma, lo, hi),      z = lam + sigma A (2 b+ - b)

(L. Condat, J. Optim. Theory Appl. 158, 2013; B. C. Vu, Adv. Comput. Math. 38, 2013), steps with
``1/tau - sigma ||A||^2 >= L_f / 2``.  The multipliers follow the sign convention of the estimators:
``0 in grad f + d penalty + A^T lam``, ``lam > 0`` where ``hi`` binds, ``< 0`` where ``lo`` binds.
"""

from __future__ import annotations

import numpy as np

from oracle.penalty import prox


def _penalty_parts(penalty, p):
    a, b, d, gidx, G = penalty
    gidx = np.arange(p) if gidx is None else np.asarray(gidx)
    a = np.zeros(p) if a is None else np.broadcast_to(np.asarray(a, float), (p,))
    b = np.zeros(G) if b is None else np.broadcast_to(np.asarray(b, float), (G,))
    d = np.zeros(G) if d is None else np.broadcast_to(np.asarray(d, float), (G,))
    return a, b, d, gidx, G


def condat_vu(X, y, penalty, A, lo, hi, tol=1e-12, max_iter=400000, beta0=None):
    """Minimiser and multipliers: ``(b, lam, iterations)``."""
    X, y = np.asarray(X, float), np.asarray(y, float)
    n, p = X.shape
    A = np.asarray(A, float).reshape(-1, p)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    a, bw, d, gidx, G = _penalty_parts(penalty, p)
    H = X.T @ X / n
    c = X.T @ y / n
    Lf = max(np.linalg.eigvalsh(H)[-1], 1e-12)
    nA2 = max(np.linalg.norm(A, 2) ** 2, 1e-300)
    sigma = Lf / nA2
    tau = 0.99 / (0.5 * Lf + sigma * nA2)
    b = np.zeros(p) if beta0 is None else np.array(beta0, float)
    lam = np.zeros(A.shape[0])
    for it in range(1, max_iter + 1):
        g = H @ b - c + A.T @ lam
        b_new = prox(b - tau * g, tau, a, bw, d, gidx, G)
        z = lam + sigma * (A @ (2.0 * b_new - b))
        lam_new = z - sigma * np.clip(z / sigma, lo, hi)
        db = np.linalg.norm(b_new - b)
        dl = np.linalg.norm(lam_new - lam)
        b, lam = b_new, lam_new
        if db <= tol * max(np.linalg.norm(b), 1e-300) and dl * tau <= tol * max(np.linalg.norm(b), 1e-300):
            break
    return b, lam, it


def kkt_constrained(X, y, penalty, A, lo, hi, b, lam, rtol=1e-6):
    """Certificate of a constrained minimiser: feasibility, multiplier signs with complementarity, and the stationarity
    residual ``||b - prox(b - (grad f(b) + A^T lam))||``.  Returns ``(ok, measures)``; every measure is relative."""
    X, y = np.asarray(X, float), np.asarray(y, float)
    n, p = X.shape
    A = np.asarray(A, float).reshape(-1, p)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    b, lam = np.asarray(b, float), np.asarray(lam, float)
    a, bw, d, gidx, G = _penalty_parts(penalty, p)
    v = A @ b
    scale_v = max(np.max(np.abs(v)) if v.size else 0.0, np.linalg.norm(A, 2) * np.max(np.abs(b)), 1e-300)
    infeas = max(0.0, np.max(lo - v, initial=0.0), np.max(v - hi, initial=0.0)) / scale_v
    lam_scale = max(np.max(np.abs(lam), initial=0.0), np.linalg.norm(X.T @ y) / n, 1e-300)
    # a multiplier away from zero sits on its bound: lam > 0 at hi, lam < 0 at lo
    big = np.abs(lam) > rtol * lam_scale
    gap_hi = np.where(lam > 0, np.abs(hi - v), 0.0)
    gap_lo = np.where(lam < 0, np.abs(v - lo), 0.0)
    wrong = big & (((lam > 0) & ~np.isfinite(hi)) | ((lam < 0) & ~np.isfinite(lo)))
    compl = float(np.max(np.where(big, np.maximum(np.nan_to_num(gap_hi, posinf=1e300), np.nan_to_num(gap_lo, posinf=1e300)), 0.0),
                         initial=0.0)) / scale_v
    grad = X.T @ (X @ b - y) / n + A.T @ lam
    stat = np.linalg.norm(b - prox(b - grad, 1.0, a, bw, d, gidx, G))
    stat_rel = stat / max(np.linalg.norm(X.T @ y) / n, np.linalg.norm(b), 1e-300)
    measures = {"infeasibility": infeas, "complementarity": compl, "wrong_sign": int(np.sum(wrong)), "stationarity": stat_rel}
    ok = infeas <= rtol and compl <= rtol and not wrong.any() and stat_rel <= rtol
    return ok, measures


def stack(constraints, p):
    """scipy constraints -> (A, lo, hi) with the rows the estimators keep (both sides infinite: dropped)."""
    from scipy.optimize import Bounds, LinearConstraint

    if isinstance(constraints, (LinearConstraint, Bounds)):
        constraints = [constraints]
    As, los, his = [], [], []
    for c in constraints:
        A = np.eye(p) if isinstance(c, Bounds) else np.atleast_2d(np.asarray(c.A.toarray() if hasattr(c.A, "toarray") else c.A, float))
        lb = np.broadcast_to(np.asarray(c.lb, float), (A.shape[0],))
        ub = np.broadcast_to(np.asarray(c.ub, float), (A.shape[0],))
        keep = np.isfinite(lb) | np.isfinite(ub)
        As.append(A[keep])
        los.append(lb[keep])
        his.append(ub[keep])
    return np.vstack(As), np.concatenate(los), np.concatenate(his)
