"""Brute-force reference for ``L1L0``: every admissible support, solved straight from X -- never through a Gram.

The problem (sparselm_amd/model/_l1l0.py; the reference's objective divided by 2n):

    minimise over supports S (sets of groups) and beta, supp beta in cols(S), |beta_j| <= big_M:
        1/(2n) ||X beta - y||^2 - 1/(2n) ||y||^2 + eta ||beta||_1 + alpha |S|
    subject to  i in S => hierarchy[i] in S

Per support: scikit-learn's ``Lasso(alpha=eta, fit_intercept=False, tol=1e-14)`` on the columns of the support, whose
objective is exactly ``1/(2n)||y - X b||^2 + eta ||b||_1``, and then an exact solve on its sign pattern by a QR
factorisation of the non-zero columns (``R^T R x = A^T y - n eta s``), taken when the signs hold.  Where that leaves the box,
a projected coordinate descent on the residual, followed by the same exact solve with the bound coordinates fixed.  ``eta = 0``
goes to ``_l0_reference.solve_support``.

Every per-support solution carries its KKT residual, computed from X: with ``g = A^T (A b - y) / n``,
``|g_j + eta sign b_j|`` on a free non-zero coordinate, ``(|g_j| - eta)_+`` on a zero one, and the one-sided violation on a
bound one.  ``brute_force_l1`` asserts it is <= 1e-10 ||X^T y / n||_inf on every support, so that what the engine is compared
with is a minimiser to that accuracy whichever route produced it.

Like ``_l0_reference.brute_force`` it returns ``gap``, ``kappa`` (of the winner's non-zero columns) and ``closed``; the
``closed`` rule of ``max_size`` stays valid because a support's lasso value is never below its unpenalised, unboxed
quadratic value.
"""

from __future__ import annotations

import itertools
import warnings

import numpy as np
from sklearn.linear_model import Lasso

from _l0_reference import group_columns, solve_support

KKT_RTOL = 1e-10


def kkt_residual(A, y, b, eta, big_M=np.inf):
    """The largest violation of the optimality conditions of min 1/(2n)||y - A b||^2 + eta ||b||_1 over |b_j| <= big_M."""
    n = A.shape[0]
    if A.shape[1] == 0:
        return 0.0
    g = A.T @ (A @ b - y) / n
    res = np.zeros(len(b))
    for j, (bj, gj) in enumerate(zip(b, g)):
        if bj == 0.0:
            res[j] = max(abs(gj) - eta, 0.0) if big_M > 0 else 0.0
        elif bj >= big_M:
            res[j] = max(gj + eta, 0.0)
        elif bj <= -big_M:
            res[j] = max(eta - gj, 0.0)
        else:
            res[j] = abs(gj + eta * np.sign(bj))
    return float(np.max(res))


def _exact_on_pattern(A, y, b, eta, big_M):
    """The free non-zero coordinates solved exactly on their signs, the bound ones fixed; b itself when signs or box fail."""
    n = A.shape[0]
    free = np.flatnonzero((b != 0.0) & (np.abs(b) < big_M))
    if len(free) == 0:
        return b
    fixed = np.flatnonzero(np.abs(b) >= big_M) if np.isfinite(big_M) else np.zeros(0, dtype=int)
    rhs_y = y - A[:, fixed] @ b[fixed] if len(fixed) else y
    Q, R = np.linalg.qr(A[:, free])
    if np.min(np.abs(np.diag(R))) <= 1e-12 * np.max(np.abs(np.diag(R))):
        return b
    s = np.sign(b[free])
    x = np.linalg.solve(R, Q.T @ rhs_y - n * eta * np.linalg.solve(R.T, s))
    if np.all(np.sign(x) == s) and np.all(np.abs(x) <= big_M):
        out = b.copy()
        out[free] = x
        return out
    return b


def _boxed_descent(A, y, b, eta, big_M, sweeps=20000):
    """Projected cyclic coordinate descent on the residual (from X, no Gram), from b clipped into the box, until a sweep moves
    nothing by more than 1e-11 relative: enough to settle which coordinates are bound, zero and free -- the exact solve on
    that pattern follows, and the KKT residual judges the result whatever happened here."""
    n = A.shape[0]
    b = np.clip(b, -big_M, big_M)
    r = y - A @ b
    h = np.einsum("ij,ij->j", A, A) / n
    for _ in range(sweeps):
        top = 0.0
        for j in range(len(b)):
            if h[j] == 0.0:
                continue
            u = b[j] + (A[:, j] @ r) / (n * h[j])
            nb = float(np.clip(np.sign(u) * max(abs(u) - eta / h[j], 0.0), -big_M, big_M))
            if nb != b[j]:
                r -= A[:, j] * (nb - b[j])
                top = max(top, abs(nb - b[j]))
                b[j] = nb
        if top <= 1e-11 * max(np.max(np.abs(b)), 1e-300):
            break
    return b


def solve_support_l1(X, y, cols, eta, big_M=np.inf):
    """(b, value, kkt): the minimiser of 1/(2n)||y - X[:, cols] b||^2 - 1/(2n)||y||^2 + eta ||b||_1 inside the box, its value
    and its KKT residual."""
    n = X.shape[0]
    if len(cols) == 0:
        return np.zeros(0), 0.0, 0.0
    A = X[:, cols]
    if eta == 0.0:
        b = solve_support(X, y, cols, big_M)[0]
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            b = Lasso(alpha=eta, fit_intercept=False, tol=1e-14, max_iter=1000000).fit(A, y).coef_.astype(float)
        if big_M <= 0:
            b = np.zeros(len(cols))
        elif np.max(np.abs(b)) > big_M:
            b = _boxed_descent(A, y, b, eta, big_M)
        b = _exact_on_pattern(A, y, b, eta, big_M)
    r = A @ b - y
    value = float((r @ r - y @ y) / (2.0 * n) + eta * np.sum(np.abs(b)))
    return b, value, kkt_residual(A, y, b, eta, big_M)


def objective_of_l1(X, y, coef, n_active, alpha=0.0, eta=0.0):
    """The objective above for given coefficients (straight from X)."""
    n = np.asarray(X).shape[0]
    r = X @ coef - y
    return float((r @ r - y @ y) / (2.0 * n) + eta * np.sum(np.abs(coef)) + alpha * n_active)


def brute_force_l1(X, y, groups=None, alpha=0.0, eta=0.0, big_M=np.inf, hierarchy=None, max_size=None):
    """The optimum over all admissible supports.  Returns a dict: ``active`` (bool per sorted label), ``coef``, ``objective``,
    ``gap`` (relative, to the second-best support), ``kappa`` (condition number of the Gram block of the winner's non-zero
    columns), ``n_supports``, ``closed``, ``kkt`` (the largest per-support KKT residual, asserted <= 1e-10 ||X^T y / n||_inf).

    ``max_size=S`` enumerates supports of at most S groups; ``closed`` says whether ``q_all_ref + alpha (S + 1) > objective``
    with ``q_all_ref`` the unboxed least-squares value on ALL columns: a support's lasso value is never below its quadratic
    value, which is monotone, so no larger support can win; ``gap`` is then capped by the distance to that bound."""
    X = np.asarray(X, dtype=float)
    y = np.asarray(y, dtype=float)
    n, p = X.shape
    uniq, gcols = group_columns(groups, p)
    G = len(uniq)
    S_max = G if max_size is None else int(min(max_size, G))
    index = {u.item(): i for i, u in enumerate(uniq)}
    need = [set() for _ in range(G)]
    if hierarchy is not None:
        assert len(hierarchy) == G
        need = [{index[np.asarray(lab).item()] for lab in subs} for subs in hierarchy]
    c_inf = float(np.max(np.abs(X.T @ y / n)))
    yy = float(y @ y)
    best = (np.inf, None, None)
    second = np.inf
    count = 0
    worst_kkt = 0.0
    for size in range(S_max + 1):
        for S in itertools.combinations(range(G), size):
            chosen = set(S)
            if any(not need[i] <= chosen for i in S):
                continue
            count += 1
            cols = np.concatenate([gcols[i] for i in S]).astype(int) if S else np.zeros(0, dtype=int)
            b, value, kkt = solve_support_l1(X, y, cols, eta, big_M)
            assert kkt <= KKT_RTOL * c_inf, f"support {S}: KKT residual {kkt:.3e} > {KKT_RTOL:g} * {c_inf:.3e}"
            worst_kkt = max(worst_kkt, kkt)
            obj = value + alpha * size
            if obj < best[0]:
                second = best[0]
                best = (obj, S, (cols, b))
            elif obj < second:
                second = obj
    obj, S, (cols, b) = best
    coef = np.zeros(p)
    coef[cols] = b
    active = np.zeros(G, dtype=bool)
    active[list(S)] = True
    scale = abs(obj) if obj != 0.0 else yy / (2.0 * n)
    closed = True
    if S_max < G:
        r_all = X @ np.linalg.lstsq(X, y, rcond=None)[0] - y
        floor = (float(r_all @ r_all) - yy) / (2.0 * n) + alpha * (S_max + 1)
        closed = bool(floor > obj)
        second = min(second, floor)
    kappa = 1.0
    nz = np.flatnonzero(coef)
    if len(nz):
        sv = np.linalg.svd(X[:, nz], compute_uv=False)
        kappa = float((sv[0] / sv[-1]) ** 2) if sv[-1] > 0 else np.inf
    return {"active": active, "coef": coef, "objective": float(obj), "gap": float((second - obj) / scale) if np.isfinite(second) else np.inf,
            "kappa": kappa, "n_supports": count, "closed": closed, "kkt": worst_kkt}
