"""The l0 local search restated in numpy, from its specification (not from the kernel): what the GPU tests compare against.

For one cell, with ``H = G + 2 eta I`` (``G = X^T W X / n``, ``c = X^T W y / n``):

    minimise over beta, |beta_j| <= big_M:   F(beta) = 1/2 beta^T H beta - c^T beta + alpha ||beta||_0

State: ``beta``, ``r = c - H beta``, ``d = diag H``.  For coordinate j given the others ``u = r_j + d_j beta_j``,
``b = clip(u / d_j, +-big_M)``, ``gain = u b - 1/2 d_j b^2``.

1. Descent: j = 0 .. p-1 cyclically, ``beta_j <- b`` if ``gain > alpha`` (strictly) else 0; a column with
   ``d_j <= PIVOT max d`` stays 0.  A sweep ends the descent when no coordinate entered or left the support and
   ``max |delta_j| sqrt(d_j) <= CD_TOL sqrt(yy)``; ``CD_SWEEPS`` sweeps end it unconverged.
2. Swap scan: for i in the support, ascending, with i removed (``r' = r + H[:, i] beta_i``): ``g_i = gain(i)`` and the best
   ``g_j`` over j outside the support, ties to the lowest j.  If ``g_j > g_i + 1e-10 max(|g_i|, alpha)``: i leaves, j enters
   at ``b_j``, back to 1.  No swap: done.  ``SWAP_CAP`` swaps end it unconverged.

The scan for the NEXT CHANGE is vectorised: until a coordinate changes ``r`` is unchanged, so every coordinate is evaluated at
once and the first one at or after the cursor whose value would change is the sequential rule's next change.

``local_search`` also reports ``margin``: the smallest relative margin by which any decision was taken -- every threshold
``gain > alpha`` of a visited coordinate, every accepted or refused swap, and for an accepted swap the lead of the entering
column over the runner-up.  Where it is far above the rounding of a double, no other order of the same arithmetic decides
differently.  ``is_swap_inescapable`` is an independent certificate: from ``beta`` alone it recomputes every one-coordinate
decision and every (i, j) swap.
"""

import numpy as np

PIVOT = 1e-12
CD_TOL = 1e-12
CD_SWEEPS = 10000
SWAP_CAP = 10000
SWAP_TOL = 1e-10


def _coord(u, d, big_M):
    with np.errstate(divide="ignore", invalid="ignore"):
        b = np.clip(u / d, -big_M, big_M)
    return b, u * b - 0.5 * d * b * b


def _rel(a, b):
    """|a - b| relative to the larger magnitude (inf where both are zero: nothing is at stake)."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    scale = np.maximum(np.abs(a), np.abs(b))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0.0, np.abs(a - b) / scale, np.inf)


def local_search(H, c, alpha, big_M, yy, start=None, swaps=True):
    """The rule on one problem.  Returns a dict: ``beta``, ``F``, ``sweeps``, ``swaps``, ``status`` (0; 1: a descent ran out of
    sweeps; 2: the swap cap), ``margin``, ``changes`` (coordinate changes applied)."""
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
    out = {"sweeps": 0, "swaps": 0, "status": 0, "margin": np.inf, "changes": 0}
    dsafe = np.where(live, d, 1.0)
    while True:
        for sweep in range(CD_SWEEPS + 1):
            if sweep == CD_SWEEPS:
                out["status"] |= 1
                break
            moved, maxd, cursor = False, 0.0, 0
            while True:
                b, gain = _coord(r + dsafe * beta, dsafe, big_M)
                nb = np.where(gain > alpha, b, 0.0)
                change = live & (nb != beta) & (idx >= cursor)
                j = int(np.argmax(change)) if change.any() else p
                seen = live & (idx >= cursor) & (idx <= j)  # the coordinates the sequential rule visits before r changes
                if seen.any():
                    out["margin"] = min(out["margin"], float(np.min(_rel(gain[seen], alpha))))
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
        if not swaps or out["status"]:
            break
        swapped = False
        for i in np.flatnonzero(beta):
            bi = beta[i]
            _, gi = _coord(r[i] + d[i] * bi, d[i], big_M)
            outside = live & (beta == 0.0)
            if not outside.any():
                continue
            bj, gj = _coord(r + H[i] * bi, dsafe, big_M)
            gj = np.where(outside, gj, -1.0)
            j = int(np.argmax(gj))  # (the first of the largest: ties to the lowest j)
            bar = gi + SWAP_TOL * max(abs(gi), alpha)
            out["margin"] = min(out["margin"], float(_rel(gj[j], bar)))
            if not gj[j] > bar:
                continue
            rest = np.delete(gj, j)
            if rest.size and rest.max() >= 0.0:
                out["margin"] = min(out["margin"], float(_rel(gj[j], rest.max())))
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
    out["F"] = float(-0.5 * beta @ (c + r) + alpha * np.count_nonzero(beta))
    return out


def objective(H, c, alpha, beta):
    return float(0.5 * beta @ H @ beta - c @ beta + alpha * np.count_nonzero(beta))


def polish(H, c, big_M, beta):
    """The exact minimiser of the quadratic on the support of ``beta`` inside the box."""
    S = np.flatnonzero(beta)
    out = np.zeros_like(beta)
    if S.size == 0:
        return out
    Hs, cs = H[np.ix_(S, S)], c[S]
    b = np.linalg.solve(Hs, cs) if np.linalg.matrix_rank(Hs) == S.size else beta[S].copy()
    if np.any(np.abs(b) > big_M) or not np.allclose(Hs @ b, cs, rtol=0, atol=1e-9 * np.abs(cs).max()):
        b = np.clip(beta[S], -big_M, big_M)  # projected coordinate descent to the last digit
        for _ in range(200000):
            worst = 0.0
            for k in range(S.size):
                nb = np.clip(b[k] + (cs[k] - Hs[k] @ b) / Hs[k, k], -big_M, big_M)
                worst = max(worst, abs(nb - b[k]))
                b[k] = nb
            if worst <= 1e-16 * max(np.abs(b).max(), 1e-300):
                break
    out[S] = b
    return out


def is_swap_inescapable(H, c, alpha, big_M, beta, tol, swaps=True):
    """From ``beta`` alone: every active coordinate sits at its one-coordinate value with ``gain > alpha``, every inactive live
    one has ``gain <= alpha``, and (``swaps``) no column outside the support beats a column inside it with that one removed --
    each within ``tol``, relative to the decision's own scale.  Returns ``(ok, why)``."""
    H = np.asarray(H, dtype=float)
    beta = np.asarray(beta, dtype=float)
    d = np.diag(H)
    live = d > PIVOT * d.max()
    if np.any(beta[~live] != 0.0) or np.any(np.abs(beta) > big_M):
        return False, "a dead column is active or a coefficient is outside the box"
    r = c - H @ beta
    for j in np.flatnonzero(live):
        b, gain = _coord(r[j] + d[j] * beta[j], d[j], big_M)
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
        _, gi = _coord(rp[i], d[i], big_M)
        for j in outside:
            _, gj = _coord(rp[j], d[j], big_M)
            if gj > gi + SWAP_TOL * max(abs(gi), alpha) + tol * max(abs(gi), alpha):
                return False, f"column {j} (gain {gj}) beats column {i} (gain {gi})"
    return True, ""


def gram(X, y, sample_weight=None, fit_intercept=False):
    """``(G, c, yy, x_mean, y_mean)`` as the engine forms them: weights normalised to sum n, weighted centring with an intercept."""
    X = np.asarray(X, dtype=float)
    y = np.asarray(y, dtype=float)
    n = X.shape[0]
    w = np.ones(n) if sample_weight is None else np.asarray(sample_weight, dtype=float) * (n / np.sum(sample_weight))
    x_mean = (w @ X) / n if fit_intercept else np.zeros(X.shape[1])
    y_mean = float(w @ y) / n if fit_intercept else 0.0
    Xc, yc = X - x_mean, y - y_mean
    return (Xc.T * w) @ Xc / n, (Xc.T * w) @ yc / n, float((w * yc) @ yc) / n, x_mean, y_mean


def solve_cells(X, y, alphas, etas, big_M=100.0, starts=None, swaps=True, sample_weight=None, fit_intercept=False):
    """Every cell ``(alphas[e], etas[e])`` from the zero start (``starts`` None) or from ``starts[e]`` (S x p): the winner by
    (F, then the lowest start index), polished.  One dict per cell: ``beta``, ``objective``, ``start``, ``swaps``, ``sweeps``,
    ``status``, ``margin`` (over every start's run), ``F`` (per start), ``H``, ``c``."""
    G, c, yy, _, _ = gram(X, y, sample_weight, fit_intercept)
    p = len(c)
    cells = []
    for e, (alpha, eta) in enumerate(zip(alphas, etas)):
        H = G + 2.0 * eta * np.eye(p)
        runs = [local_search(H, c, alpha, big_M, yy, None if starts is None else s, swaps) for s in ([None] if starts is None else starts[e])]
        F = np.array([run["F"] for run in runs])
        win = int(np.argmin(F))  # (the first of the lowest)
        beta = polish(H, c, big_M, runs[win]["beta"])
        lead = np.inf if len(F) == 1 else float(np.min(_rel(np.delete(F, win), F[win])))
        cells.append({"beta": beta, "objective": objective(H, c, alpha, beta), "start": win, "swaps": runs[win]["swaps"],
                      "sweeps": runs[win]["sweeps"], "status": runs[win]["status"], "margin": min(run["margin"] for run in runs),
                      "F": F, "lead": lead, "H": H, "c": c})
    return cells


def hard_law(seed, n=30, p=14, rho=0.9, k=4, snr=2.0):
    """The law the hit counts are measured on: AR(1) columns with correlation ``rho``, ``k`` true columns spread evenly with
    unit coefficients of alternating sign, noise at signal-to-noise ratio ``snr``."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, p))
    X = np.empty((n, p))
    X[:, 0] = Z[:, 0]
    for j in range(1, p):
        X[:, j] = rho * X[:, j - 1] + np.sqrt(1.0 - rho * rho) * Z[:, j]
    beta = np.zeros(p)
    beta[np.linspace(0, p - 1, k).round().astype(int)] = (-1.0) ** np.arange(k)
    signal = X @ beta
    y = signal + rng.standard_normal(n) * np.sqrt(np.var(signal) / snr)
    return X, y
