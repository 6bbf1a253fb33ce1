"""Local subsets (the cardinality form of the l0 local search) restated in numpy, from its specification and not from the
kernel: what the GPU tests compare against.

For one cell ``(k, eta)``, with ``H = G + 2 eta I`` (``G = X^T W X / n``, ``c = X^T W y / n``):

    minimise over beta, |beta_j| <= big_M, ||beta||_0 <= k:   Q(beta) = 1/2 beta^T H beta - c^T beta

State: ``beta``, ``r = c - H beta``, ``d = diag H``; a column with ``d_j <= PIVOT max d`` stays out.  For coordinate j given the
others ``u``, ``b = clip(u / d_j, +-big_M)``, ``gain = u b - 1/2 d_j b^2``; ``tol = CD_TOL sqrt(yy)``.  From a start of any
support size inside the box (zero when none is given):

1. Shrink: while ``nnz > k`` the support column with the smallest gain at ``u = r_i + d_i beta_i`` leaves (ties: the lowest
   index); one row update each.
2. Descent on the support: j over the support cyclically, ``beta_j <- b`` with ``u = r_j + d_j beta_j``; no threshold, no column
   enters, ``b == 0`` leaves.  A sweep ends the descent when the support stood still and ``max |delta_j| sqrt(d_j) <= tol``;
   ``CD_SWEEPS`` sweeps end it unconverged.
3. Grow: if ``nnz < k`` the outside column with the largest gain at ``u = r_j`` (ties: the lowest j) enters at ``b_j`` if
   ``|b_j| sqrt(d_j) > tol``; back to 2.
4. Swap scan, once 3 adds nothing: for i in the support, ascending, with i removed (``r' = r + H[:, i] beta_i``): ``g_i`` and
   the best ``g_j`` over j outside, ties to the lowest j.  If ``g_j > g_i + 1e-10 |g_i|``: i leaves, j enters at ``b_j``, back to
   2.  No swap: done.  ``SWAP_CAP`` accepted swaps end it unconverged.  ``swaps=False`` stops after 3.

``local_subsets`` also reports ``margin``: the smallest relative margin of any decision -- the lead of every column that left
in 1 over the next weakest, the lead of every column that 3 picked over the runner-up and the distance of its ``tol`` test,
every accepted or refused swap, and for an accepted swap the lead of the entering column.  (The descent takes no decision but
``b == 0``, which is not counted.)  ``is_subset_inescapable`` is a certificate written independently of the rule: from ``beta``
alone, ``nnz <= k``, every active coordinate is at its one-coordinate value, no entry and no (i, j) swap is possible.
"""

import numpy as np

from _l0_local_reference import CD_SWEEPS, CD_TOL, PIVOT, SWAP_CAP, SWAP_TOL, _coord, _rel, gram, polish

__all__ = ["local_subsets", "is_subset_inescapable", "quadratic", "solve_cells", "best_subset", "best_subsets"]


def _lead(values, pick, largest):
    """The relative lead of ``values[pick]`` over the best of the others (inf when alone)."""
    rest = np.delete(values, pick)
    rest = rest[np.isfinite(rest)]
    if rest.size == 0:
        return np.inf
    return float(_rel(values[pick], rest.max() if largest else rest.min()))


def local_subsets(H, c, k, big_M, yy, start=None, swaps=True):
    """The rule on one problem.  Returns a dict: ``beta``, ``Q``, ``sweeps``, ``swaps``, ``grows``, ``drops``, ``status`` (0;
    1: a descent ran out of sweeps; 2: the swap cap), ``nnz``, ``margin``."""
    H = np.asarray(H, dtype=float)
    c = np.asarray(c, dtype=float)
    p = len(c)
    d = np.diag(H).copy()
    live = d > PIVOT * (d.max() if p else 0.0)
    dsafe = np.where(live, d, 1.0)
    beta = np.zeros(p) if start is None else np.where(live, np.asarray(start, dtype=float), 0.0)
    r = c.copy()
    for j in np.flatnonzero(beta):
        r -= H[j] * beta[j]
    tol = CD_TOL * np.sqrt(yy)
    out = {"sweeps": 0, "swaps": 0, "grows": 0, "drops": 0, "status": 0, "margin": np.inf}

    def note(m):
        out["margin"] = min(out["margin"], float(m))

    while True:
        # 1. shrink
        while np.count_nonzero(beta) > k:
            S = np.flatnonzero(beta)
            _, g = _coord(r[S] + d[S] * beta[S], d[S], big_M)
            a = int(np.argmin(g))  # (the first of the smallest: the lowest index)
            note(_lead(g, a, largest=False))
            i = S[a]
            r += H[i] * beta[i]
            beta[i] = 0.0
            out["drops"] += 1
        # 2. descent on the support
        for sweep in range(CD_SWEEPS + 1):
            if sweep == CD_SWEEPS:
                out["status"] |= 1
                break
            moved, maxd = False, 0.0
            for j in np.flatnonzero(beta):  # (nothing enters during a sweep, so the support at its start is every candidate)
                if beta[j] == 0.0:
                    continue
                b, _ = _coord(r[j] + d[j] * beta[j], d[j], big_M)
                b = float(b)
                if b == beta[j]:
                    continue
                delta = b - beta[j]
                if b == 0.0:
                    moved = True
                    out["drops"] += 1
                maxd = max(maxd, abs(delta) * np.sqrt(d[j]))
                beta[j] = b
                r -= H[j] * delta
            out["sweeps"] += 1
            if not moved and maxd <= tol:
                break
        if out["status"]:
            break
        outside = live & (beta == 0.0)
        # 3. grow
        if np.count_nonzero(beta) < k and outside.any():
            b, g = _coord(r, dsafe, big_M)
            g = np.where(outside, g, -np.inf)
            j = int(np.argmax(g))  # (the first of the largest: the lowest j)
            note(_lead(g, j, largest=True))
            move = abs(b[j]) * np.sqrt(d[j])
            note(_rel(move, tol))
            if move > tol:
                beta[j] = b[j]
                r -= H[j] * b[j]
                out["grows"] += 1
                continue
        if not swaps:
            break
        # 4. swap scan
        swapped = False
        for i in np.flatnonzero(beta):
            if not outside.any():
                break
            bi = beta[i]
            _, gi = _coord(r[i] + d[i] * bi, d[i], big_M)
            bj, gj = _coord(r + H[i] * bi, dsafe, big_M)
            gj = np.where(outside, gj, -np.inf)
            j = int(np.argmax(gj))
            bar = gi + SWAP_TOL * abs(gi)
            note(_rel(gj[j], bar))
            if not gj[j] > bar:
                continue
            note(_lead(gj, j, largest=True))
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
    out["nnz"] = int(np.count_nonzero(beta))
    out["Q"] = float(-0.5 * beta @ (c + r))
    return out


def quadratic(H, c, beta):
    return float(0.5 * beta @ H @ beta - c @ beta)


def is_subset_inescapable(H, c, k, big_M, yy, beta, tol, swaps=True):
    """From ``beta`` alone: at most k non-zeros, none on a dead column or outside the box; every active coordinate at its
    one-coordinate value; below k no live column outside would move by more than the descent's tolerance; and (``swaps``) no
    column outside beats a column inside with that one removed -- each within ``tol``, relative to the decision's own scale.
    Returns ``(ok, why)``."""
    H = np.asarray(H, dtype=float)
    beta = np.asarray(beta, dtype=float)
    d = np.diag(H)
    live = d > PIVOT * d.max()
    S = np.flatnonzero(beta)
    if S.size > k:
        return False, f"{S.size} non-zeros, more than k = {k}"
    if np.any(beta[~live] != 0.0) or np.any(np.abs(beta) > big_M):
        return False, "a dead column is active or a coefficient is outside the box"
    r = c - H @ beta
    for j in S:
        b = float(np.clip((r[j] + d[j] * beta[j]) / d[j], -big_M, big_M))
        if abs(b - beta[j]) > tol * max(abs(b), abs(beta[j])):
            return False, f"active column {j} is not at its one-coordinate value: {beta[j]} against {b}"
    outside = np.flatnonzero(live & (beta == 0.0))
    if S.size < k:
        for j in outside:
            b = float(np.clip(r[j] / d[j], -big_M, big_M))
            if abs(b) * np.sqrt(d[j]) > (CD_TOL + tol) * np.sqrt(yy):
                return False, f"column {j} could still enter ({S.size} < k = {k}): it would move by {abs(b) * np.sqrt(d[j])}"
    if not swaps:
        return True, ""
    for i in S:
        rp = r + H[:, i] * beta[i]
        bi = float(np.clip(rp[i] / d[i], -big_M, big_M))
        gi = rp[i] * bi - 0.5 * d[i] * bi * bi
        for j in outside:
            bj = float(np.clip(rp[j] / d[j], -big_M, big_M))
            gj = rp[j] * bj - 0.5 * d[j] * bj * bj
            if gj > gi + (SWAP_TOL + tol) * abs(gi):
                return False, f"column {j} (gain {gj}) beats column {i} (gain {gi})"
    return True, ""


def solve_cells(G, c, yy, sizes, etas, big_M=100.0, starts=None, swaps=True):
    """Every cell ``(sizes[e], etas[e])`` of one row set's ``(G, c, yy)`` from the zero start (``starts`` None) or from
    ``starts[e]`` (S x p): the winner by (Q, then the lowest start index), polished.  One dict per cell: ``beta``,
    ``objective``, ``start``, the winner's ``swaps``, ``sweeps``, ``grows``, ``drops``, ``status``, ``margin`` (over every
    start's run), ``lead`` (of the winner's Q over the other starts'), ``Q`` and ``stats`` (per start), ``H``."""
    p = len(c)
    cells = []
    for e, (k, eta) in enumerate(zip(sizes, etas)):
        H = G + 2.0 * eta * np.eye(p)
        runs = [local_subsets(H, c, int(k), big_M, yy, s, swaps) for s in ([None] if starts is None else starts[e])]
        Q = np.array([run["Q"] for run in runs])
        win = int(np.argmin(Q))  # (the first of the lowest)
        beta = polish(H, c, big_M, runs[win]["beta"])
        lead = np.inf if len(Q) == 1 else float(np.min(_rel(np.delete(Q, win), Q[win])))
        cells.append({"beta": beta, "objective": quadratic(H, c, beta), "start": win, "margin": min(run["margin"] for run in runs),
                      "lead": lead, "Q": Q, "H": H, "stats": np.array([[run[key] for key in ("sweeps", "swaps", "status", "nnz", "grows", "drops")]
                                                                        for run in runs]),
                      **{key: runs[win][key] for key in ("swaps", "sweeps", "grows", "drops", "status")}})
    return cells


def best_subsets(H, c, kmax, big_M=100.0):
    """``out[k]``, k = 0 .. kmax: the optimum over every support of at most k columns, by enumeration (small p only; the box
    must not bind).  The supports of one size are solved as one batch."""
    from itertools import combinations

    p = len(c)
    out = np.zeros(kmax + 1)
    for m in range(1, kmax + 1):
        out[m] = out[m - 1]
        if m > p:
            continue
        S = np.array(list(combinations(range(p), m)))
        b = np.linalg.solve(H[S[:, :, None], S[:, None, :]], c[S][:, :, None])[:, :, 0]
        assert np.all(np.abs(b) <= big_M)
        out[m] = min(out[m], float(np.min(-0.5 * np.sum(c[S] * b, axis=1))))
    return out


def best_subset(H, c, k, big_M=100.0):
    """The optimum over every support of at most k columns."""
    return float(best_subsets(H, c, k, big_M)[k])


__all__ += ["gram"]
