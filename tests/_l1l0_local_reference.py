"""The l0 local search WITH AN L1 TERM restated in numpy, from its specification (not from the kernel): what the GPU tests
compare against.

For one cell ``(alpha, lam, eta)``, with ``H = G + 2 eta I`` (``G = X^T W X / n``, ``c = X^T W y / n``):

    minimise over beta, |beta_j| <= big_M:   F(beta) = 1/2 beta^T H beta - c^T beta + lam ||beta||_1 + alpha ||beta||_0

State: ``beta``, ``r = c - H beta``, ``d = diag H``.  For coordinate j given the others

    u = r_j + d_j beta_j,   s = sign(u) max(|u| - lam, 0),   b = clip(s / d_j, +-big_M),   gain = u b - 1/2 d_j b^2 - lam |b|

(``gain``: what F without the alpha term falls by when beta_j goes from 0 to b).  Everything else is the rule of
``_l0_local_reference``:

1. Descent: j = 0 .. p-1 cyclically, ``beta_j <- b`` if ``gain > alpha`` (strictly) else 0; a column with
   ``d_j <= PIVOT max d`` stays 0.  A sweep ends the descent when no coordinate entered or left the support and
   ``max |delta_j| sqrt(d_j) <= CD_TOL sqrt(yy)``; ``CD_SWEEPS`` sweeps end it unconverged.
2. Swap scan: for i in the support, ascending, with i removed: ``g_i = gain(i)`` and the best ``g_j`` over j outside the support,
   ties to the lowest j.  If ``g_j > g_i + 1e-10 max(|g_i|, alpha)``: i leaves, j enters at ``b_j``, back to 1.  No swap: done.

``F = -1/2 sum beta_j (c_j + r_j) + lam sum |beta_j| + alpha nnz``.

``local_search`` reports ``margin``: the smallest relative margin of any decision -- each ``gain > alpha`` and each ``|u|`` against
``lam`` of a coordinate the descent visits, each accepted or refused swap, and for an accepted swap the lead of the entering column
over the runner-up.  ``is_l1_swap_inescapable`` is a certificate from ``beta`` alone.  ``brute_force`` is the optimum over all
supports, a lasso on each.
"""

import itertools

import numpy as np
from _l0_local_reference import CD_SWEEPS, CD_TOL, PIVOT, SWAP_CAP, SWAP_TOL, _rel, gram

__all__ = ["local_search", "objective", "polish", "is_l1_swap_inescapable", "brute_force", "solve_cells"]


def _coord(u, d, big_M, lam):
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sign(u) * np.maximum(np.abs(u) - lam, 0.0)
        b = np.clip(s / d, -big_M, big_M)
    return b, u * b - 0.5 * d * b * b - lam * np.abs(b)


def local_search(H, c, alpha, lam, big_M, yy, start=None, swaps=True):
    """The rule on one problem.  Returns a dict: ``beta``, ``F``, ``sweeps``, ``swaps``, ``status`` (0; 1: a descent ran out of
    sweeps; 2: the swap cap), ``margin``, ``changes``, ``lowered`` (every accepted swap lowered F at the descent's next fixed point)."""
    H = np.asarray(H, dtype=float)
    c = np.asarray(c, dtype=float)
    p = len(c)
    d = np.diag(H).copy()
    live = d > PIVOT * (d.max() if p else 0.0)
    idx = np.arange(p)
    beta = np.zeros(p) if start is None else np.where(live, np.asarray(start, dtype=float), 0.0)
    r = c.copy()
    for j in np.flatnonzero(beta):
        r -= H[j] * beta[j]
    tol = CD_TOL * np.sqrt(yy)
    out = {"sweeps": 0, "swaps": 0, "status": 0, "margin": np.inf, "changes": 0, "lowered": True}
    dsafe = np.where(live, d, 1.0)

    def value():
        return float(-0.5 * beta @ (c + r) + lam * np.abs(beta).sum() + alpha * np.count_nonzero(beta))

    before_swap = None
    while True:
        for sweep in range(CD_SWEEPS + 1):
            if sweep == CD_SWEEPS:
                out["status"] |= 1
                break
            moved, maxd, cursor = False, 0.0, 0
            while True:
                u = r + dsafe * beta
                b, gain = _coord(u, dsafe, big_M, lam)
                nb = np.where(gain > alpha, b, 0.0)
                change = live & (nb != beta) & (idx >= cursor)
                j = int(np.argmax(change)) if change.any() else p
                seen = live & (idx >= cursor) & (idx <= j)  # the coordinates the sequential rule visits before r changes
                if seen.any():
                    out["margin"] = min(out["margin"], float(np.min(_rel(gain[seen], alpha))), float(np.min(_rel(np.abs(u[seen]), lam))))
                if j == p:
                    break
                delta = nb[j] - beta[j]
                moved = moved or ((nb[j] != 0.0) != (beta[j] != 0.0))
                maxd = max(maxd, abs(delta) * np.sqrt(d[j]))
                beta[j] = nb[j]
                r -= H[j] * delta
                out["changes"] += 1
                cursor = j + 1
            out["sweeps"] += 1
            if not moved and maxd <= tol:
                break
        if before_swap is not None:
            out["lowered"] = out["lowered"] and value() < before_swap
        if not swaps or out["status"]:
            break
        swapped = False
        for i in np.flatnonzero(beta):
            bi = beta[i]
            _, gi = _coord(r[i] + d[i] * bi, d[i], big_M, lam)
            outside = live & (beta == 0.0)
            if not outside.any():
                continue
            bj, gj = _coord(r + H[i] * bi, dsafe, big_M, lam)
            gj = np.where(outside, gj, -1.0)
            j = int(np.argmax(gj))  # (the first of the largest: ties to the lowest j)
            bar = gi + SWAP_TOL * max(abs(gi), alpha)
            out["margin"] = min(out["margin"], float(_rel(gj[j], bar)))
            if not gj[j] > bar:
                continue
            rest = np.delete(gj, j)
            if rest.size and rest.max() >= 0.0:
                out["margin"] = min(out["margin"], float(_rel(gj[j], rest.max())))
            before_swap = value()
            beta[i] = 0.0
            r += H[i] * bi
            beta[j] = bj[j]
            r -= H[j] * bj[j]
            out["swaps"] += 1
            swapped = True
            break
        if not swapped:
            break
        if out["swaps"] == SWAP_CAP:
            out["status"] |= 2
            break
    out["beta"] = beta
    out["F"] = value()
    return out


def objective(H, c, alpha, lam, beta):
    return float(0.5 * beta @ H @ beta - c @ beta + lam * np.abs(beta).sum() + alpha * np.count_nonzero(beta))


def _lasso_on(Hs, cs, lam, big_M, b, sweeps=20000):
    """The minimiser of 1/2 b^T Hs b - cs^T b + lam ||b||_1 inside the box: soft-threshold descent to the last digit, then the exact
    solve on the sign pattern of the free coordinates, taken when every sign and the box hold."""
    m = len(cs)
    b = np.clip(np.asarray(b, dtype=float), -big_M, big_M)
    for _ in range(sweeps):
        worst = 0.0
        for k in range(m):
            u = cs[k] - Hs[k] @ b + Hs[k, k] * b[k]
            nb = float(np.clip(np.sign(u) * max(abs(u) - lam, 0.0) / Hs[k, k], -big_M, big_M))
            worst = max(worst, abs(nb - b[k]))
            b[k] = nb
        if worst <= 1e-15 * max(np.abs(b).max(), 1e-300):  # (a descent's last digit flickers: the exact solve below settles it)
            break
    free = np.flatnonzero((b != 0.0) & (np.abs(b) < big_M))
    bound = np.flatnonzero(np.abs(b) >= big_M)
    if free.size:
        rhs = cs[free] - lam * np.sign(b[free]) - Hs[np.ix_(free, bound)] @ b[bound]
        try:
            x = np.linalg.solve(Hs[np.ix_(free, free)], rhs)
        except np.linalg.LinAlgError:
            return b
        if np.all(np.sign(x) == np.sign(b[free])) and np.all(np.abs(x) <= big_M):
            trial = b.copy()
            trial[free] = x
            value = lambda v: 0.5 * v @ Hs @ v - cs @ v + lam * np.abs(v).sum()  # noqa: E731
            if value(trial) <= value(b):
                b = trial
    return b


def polish(H, c, lam, big_M, beta):
    """The lasso minimiser on the support of ``beta`` inside the box; a coefficient it brings to zero is zero."""
    S = np.flatnonzero(beta)
    out = np.zeros_like(np.asarray(beta, dtype=float))
    if S.size:
        out[S] = _lasso_on(H[np.ix_(S, S)], c[S], lam, big_M, beta[S])
    return out


def is_l1_swap_inescapable(H, c, alpha, lam, big_M, beta, tol, swaps=True):
    """From ``beta`` alone: every active coordinate sits at its one-coordinate value with ``gain > alpha``, every inactive live one
    has ``gain <= alpha``, and (``swaps``) no column outside the support beats a column inside it with that one removed -- each
    within ``tol``, relative to the decision's own scale.  Returns ``(ok, why)``."""
    H = np.asarray(H, dtype=float)
    beta = np.asarray(beta, dtype=float)
    d = np.diag(H)
    live = d > PIVOT * d.max()
    if np.any(beta[~live] != 0.0) or np.any(np.abs(beta) > big_M):
        return False, "a dead column is active or a coefficient is outside the box"
    r = c - H @ beta
    for j in np.flatnonzero(live):
        b, gain = _coord(r[j] + d[j] * beta[j], d[j], big_M, lam)
        slack = tol * max(abs(gain), alpha)
        if beta[j] != 0.0:
            if not gain > alpha - slack:
                return False, f"active column {j} has gain {gain} <= alpha {alpha}"
            if abs(b - beta[j]) > tol * max(abs(b), abs(beta[j])):
                return False, f"active column {j} is not at its one-coordinate value: {beta[j]} against {b}"
        elif gain > alpha + slack:
            return False, f"inactive column {j} has gain {gain} > alpha {alpha}"
    if not swaps:
        return True, ""
    outside = np.flatnonzero(live & (beta == 0.0))
    for i in np.flatnonzero(beta):
        rp = r + H[:, i] * beta[i]
        _, gi = _coord(rp[i], d[i], big_M, lam)
        for j in outside:
            _, gj = _coord(rp[j], d[j], big_M, lam)
            if gj > gi + SWAP_TOL * max(abs(gi), alpha) + tol * max(abs(gi), alpha):
                return False, f"column {j} (gain {gj}) beats column {i} (gain {gi})"
    return True, ""


def brute_force(H, c, alpha, lam, big_M):
    """``(F, beta)`` of the optimum: the lasso minimiser on every support, valued with alpha on ITS non-zeros.  (The optimum is the
    lasso minimiser on its own support, so the least of these is the optimum.)  Every support's descent runs at once for a
    while; then each support's point is replaced by the exact solve on its sign pattern, which IS the lasso minimiser of that
    support when it keeps every sign, stays inside the box and the zeros of the support satisfy |gradient| <= lam (the problem is
    convex: these conditions suffice); a support where they fail runs its own descent to the last digit."""
    H = np.asarray(H, dtype=float)
    p = len(c)
    masks = np.array(list(itertools.product([0.0, 1.0], repeat=p)))
    d = np.diag(H)
    B = np.zeros_like(masks)
    for sweep in range(150):
        for j in range(p):
            u = c[j] - B @ H[:, j] + d[j] * B[:, j]
            B[:, j] = masks[:, j] * np.clip(np.sign(u) * np.maximum(np.abs(u) - lam, 0.0) / d[j], -big_M, big_M)
    best_F, best = 0.0, np.zeros(p)
    for s in range(len(masks)):
        S = np.flatnonzero(masks[s])
        A = np.flatnonzero(B[s])
        b = np.zeros(p)
        exact = False
        if A.size and np.all(np.abs(B[s, A]) < big_M):
            x = np.linalg.solve(H[np.ix_(A, A)], c[A] - lam * np.sign(B[s, A]))
            b[A] = x
            g = c[S] - H[S] @ b
            exact = bool(np.all(np.sign(x) == np.sign(B[s, A])) and np.all(np.abs(x) < big_M) and np.all(np.abs(g[b[S] == 0.0]) <= lam))
        elif not A.size:
            exact = bool(np.all(np.abs(c[S]) <= lam))
        if not exact:
            b = np.zeros(p)
            b[S] = _lasso_on(H[np.ix_(S, S)], c[S], lam, big_M, B[s, S])
        F = objective(H, c, alpha, lam, b)
        if F < best_F:
            best_F, best = F, b
    return best_F, best


def solve_cells(X, y, alphas, l1s, ridges=None, big_M=100.0, starts=None, swaps=True, sample_weight=None, fit_intercept=False):
    """Every cell ``(alphas[e], l1s[e], ridges[e])`` from the zero start (``starts`` None) or from ``starts[e]`` (S x p): the winner
    by (F, then the lowest start index), polished.  One dict per cell: ``beta``, ``objective``, ``descent_objective``, ``start``,
    ``swaps``, ``sweeps``, ``status``, ``margin`` (over every start's run), ``F`` (per start), ``lead``, ``H``, ``c``."""
    G, c, yy, _, _ = gram(X, y, sample_weight, fit_intercept)
    p = len(c)
    ridges = np.zeros(len(alphas)) if ridges is None else ridges
    cells = []
    for e, (alpha, lam, eta) in enumerate(zip(alphas, l1s, ridges)):
        H = G + 2.0 * eta * np.eye(p)
        runs = [local_search(H, c, alpha, lam, big_M, yy, None if starts is None else s, swaps) for s in ([None] if starts is None else starts[e])]
        F = np.array([run["F"] for run in runs])
        win = int(np.argmin(F))  # (the first of the lowest)
        beta = polish(H, c, lam, big_M, runs[win]["beta"])
        if objective(H, c, alpha, lam, beta) > objective(H, c, alpha, lam, runs[win]["beta"]):
            beta = runs[win]["beta"].copy()  # (the polish never raises F)
        lead = np.inf if len(F) == 1 else float(np.min(_rel(np.delete(F, win), F[win])))
        cells.append({"beta": beta, "objective": objective(H, c, alpha, lam, beta), "descent_objective": float(F[win]), "start": win,
                      "swaps": runs[win]["swaps"], "sweeps": runs[win]["sweeps"], "status": runs[win]["status"],
                      "margin": min(run["margin"] for run in runs), "F": F, "lead": lead, "H": H, "c": c, "yy": yy,
                      "lowered": all(run["lowered"] for run in runs), "run_betas": [run["beta"] for run in runs]})
    return cells
