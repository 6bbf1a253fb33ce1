"""The l0 local search with groups and a hierarchy restated in numpy, from its specification (not from the kernel): what the GPU
tests and the host twin's test compare against.

For one cell, with ``H = G + 2 eta I``:

    minimise over beta, |beta_j| <= big_M:   F(beta) = 1/2 beta^T H beta - c^T beta + alpha |cl(S(beta))|

``S(beta)``: the groups that hold a non-zero coefficient; ``cl``: its closure under the hierarchy.  Groups are contiguous column
ranges ``gstart[g] .. gstart[g + 1] - 1``; ``closed[g]`` is the transitively closed list of the groups ``g`` needs, without ``g``.

State: ``beta``, ``r = c - H beta``, ``d = diag H``; per group ``nz`` (non-zero coefficients) and ``held`` (the groups ``h != g``
with ``nz_h > 0`` that need ``g``); ``z_g = nz_g > 0 or held_g > 0``.  The price of a group that is empty or has just been emptied:
``m_g = [held_g == 0] (1 + #{h in closed[g]: nz_h == 0 and held_h == 0})``.

1. Group descent, g cyclically: a group with ``z_g`` gets a step, an inactive one only when ``C_g = sum_{j in g, live} gain(r_j, d_j)
   > alpha m_g / SCREEN``.  The step: up to ``INNER`` passes ``beta_j <- b_j`` over the group's live columns, ascending, no threshold,
   ended by a pass with ``max |delta| sqrt(d) <= tol``; then ``v_g = 1/2 beta_g^T (r_g + r'_g)``, ``r' = r + H[:, g] beta_g``; keep iff
   ``v_g > alpha m_g``, else ``beta_g <- 0``, ``r <- r'``.  A sweep ends the descent when no group entered or left and the kept
   steps' ``max |delta| sqrt(d) <= tol``.
2. Group swap scan: i ascending over ``nz_i > 0 and held_i == 0``: remove i (``v_i``, ``m_i``); the candidate j is the empty group other
   than i with the largest ``C_j(r') - alpha m_j`` (ties: the lowest); fit j from zero (``v_j``); accept iff
   ``v_j - alpha m_j > v_i - alpha m_i + 1e-10 max(|v_i|, alpha)`` and go back to 1, else restore exactly.

``local_group_search`` records ``margin``: the smallest relative margin of any decision (screen, keep / drop, candidate lead, swap).
``is_group_swap_inescapable`` is the independent certificate; ``brute_force`` the ground truth over all closed group supports.
"""

import itertools

import numpy as np

from _l0_local_reference import CD_SWEEPS, CD_TOL, PIVOT, SWAP_CAP, SWAP_TOL, _rel, gram

SCREEN = 4.0
INNER = 8


def close_hierarchy(n_groups, need):
    """``need[g]``: the groups ``g`` needs directly (None: no hierarchy).  Returns the closed lists: everything reachable, without
    ``g`` itself, ascending."""
    if need is None:
        return [[] for _ in range(n_groups)]
    closed = []
    for g in range(n_groups):
        seen, stack = set(), [g]
        while stack:
            for t in need[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        closed.append(sorted(seen - {g}))
    return closed


def closure(beta, gstart, closed):
    """cl(S(beta)) as a bool per group."""
    ng = len(gstart) - 1
    inside = np.zeros(ng, dtype=bool)
    for g in range(ng):
        if np.any(beta[gstart[g]:gstart[g + 1]] != 0.0):
            inside[g] = True
            inside[closed[g]] = True
    return inside


def _gain(u, d, big_M):
    b = min(max(u / d, -big_M), big_M)
    return b, u * b - 0.5 * d * b * b


class _State:
    """beta, r and the group tables of one problem, with the moves of the rule."""

    def __init__(self, H, c, gstart, closed, alpha, big_M, yy, start):
        self.H, self.c, self.gstart, self.closed, self.alpha, self.big_M = H, c, gstart, closed, alpha, big_M
        self.ng = len(gstart) - 1
        self.d = np.diag(H).copy()
        self.live = self.d > PIVOT * (self.d.max() if len(c) else 0.0)
        self.beta = np.zeros(len(c)) if start is None else np.where(self.live, np.asarray(start, dtype=float), 0.0)
        self.r = c.copy()
        for j in np.flatnonzero(self.beta):
            self.r -= H[j] * self.beta[j]
        self.tol = CD_TOL * np.sqrt(yy)
        self.nz = np.array([np.count_nonzero(self.beta[gstart[g]:gstart[g + 1]]) for g in range(self.ng)], dtype=int)
        self.held = np.zeros(self.ng, dtype=int)
        for g in np.flatnonzero(self.nz):
            self.held[closed[g]] += 1
        self.trials = 0

    def cols(self, g):
        return range(self.gstart[g], self.gstart[g + 1])

    def price(self, g):
        """m_g: of an empty group, or of a non-empty one as if it had just been emptied."""
        if self.held[g] > 0:
            return 0
        own = 1 if self.nz[g] > 0 else 0
        return 1 + sum(1 for h in self.closed[g] if self.nz[h] == 0 and self.held[h] == own)

    def gains(self, g):
        total = 0.0
        for j in self.cols(g):
            if self.live[j]:
                total += _gain(self.r[j], self.d[j], self.big_M)[1]
        return total

    def fit(self, g):
        worst = 0.0
        for _ in range(INNER):
            mp = 0.0
            for j in self.cols(g):
                if not self.live[j]:
                    continue
                b, _ = _gain(self.r[j] + self.d[j] * self.beta[j], self.d[j], self.big_M)
                delta = b - self.beta[j]
                if delta == 0.0:
                    continue
                self.beta[j] = b
                self.r -= self.H[j] * delta
                mp = max(mp, abs(delta) * np.sqrt(self.d[j]))
            worst = max(worst, mp)
            if mp <= self.tol:
                break
        return worst

    def value(self, g):
        """(v_g, r')"""
        rp = self.r.copy()
        for j in self.cols(g):
            if self.beta[j] != 0.0:
                rp += self.H[j] * self.beta[j]
        v = 0.0
        for j in self.cols(g):
            v += self.beta[j] * (self.r[j] + rp[j])
        return 0.5 * v, rp

    def empty(self, g, rp):
        self.beta[self.gstart[g]:self.gstart[g + 1]] = 0.0
        self.r = rp

    def count(self, g):
        return int(np.count_nonzero(self.beta[self.gstart[g]:self.gstart[g + 1]]))


def local_group_search(H, c, gstart, closed, alpha, big_M, yy, start=None, swaps=True):
    """The rule on one problem.  Returns a dict: ``beta``, ``F``, ``sweeps``, ``swaps``, ``status`` (0; 1: a descent ran out of
    sweeps; 2: the swap cap), ``closed`` (cl(S), bool per group), ``trials``, ``margin``."""
    H = np.asarray(H, dtype=float)
    c = np.asarray(c, dtype=float)
    s = _State(H, c, gstart, closed, alpha, big_M, yy, start)
    out = {"sweeps": 0, "swaps": 0, "status": 0, "margin": np.inf}

    def note(a, b):
        out["margin"] = min(out["margin"], float(_rel(a, b)))

    while True:
        for sweep in range(CD_SWEEPS + 1):
            if sweep == CD_SWEEPS:
                out["status"] |= 1
                break
            moved, maxd = False, 0.0
            for g in range(s.ng):
                was = s.nz[g] > 0
                m = s.price(g)
                if not was and s.held[g] == 0:
                    C = s.gains(g)
                    note(C, alpha * m / SCREEN)
                    if not C > alpha * m / SCREEN:
                        continue
                    s.trials += 1
                worst = s.fit(g)
                v, rp = s.value(g)
                note(v, alpha * m)
                if v > alpha * m:
                    now = s.count(g)
                    if (now > 0) != was:
                        s.held[closed[g]] += 1 if now > 0 else -1
                        moved = True
                    s.nz[g] = now
                    maxd = max(maxd, worst)
                else:
                    s.empty(g, rp)
                    s.nz[g] = 0
                    if was:
                        s.held[closed[g]] -= 1
                        moved = True
            out["sweeps"] += 1
            if not moved and maxd <= s.tol:
                break
        if not swaps or out["status"]:
            break
        swapped = False
        for i in range(s.ng):
            if s.nz[i] == 0 or s.held[i] > 0:
                continue
            saved = (s.beta.copy(), s.r.copy(), int(s.nz[i]))
            mi = s.price(i)
            vi, rp = s.value(i)
            s.empty(i, rp)
            s.nz[i] = 0
            s.held[closed[i]] -= 1
            scores = np.array([s.gains(j) - alpha * s.price(j) if j != i and s.nz[j] == 0 else -np.inf for j in range(s.ng)])
            ok = False
            if np.isfinite(scores).any():
                j = int(np.argmax(scores))  # (the first of the largest: ties to the lowest j)
                rest = np.delete(scores, j)
                rest = rest[np.isfinite(rest)]
                mj = s.price(j)
                s.trials += 1
                s.fit(j)
                vj, _ = s.value(j)
                bar = vi - alpha * mi + SWAP_TOL * max(abs(vi), alpha)
                note(vj - alpha * mj, bar)
                ok = vj - alpha * mj > bar
                if ok and rest.size:
                    note(scores[j], rest.max())  # the lead of the entering group over the runner-up
            if ok:
                s.nz[j] = s.count(j)
                if s.nz[j] > 0:
                    s.held[closed[j]] += 1
                out["swaps"] += 1
                swapped = True
                break
            s.beta, s.r, s.nz[i] = saved
            s.held[closed[i]] += 1
        if not swapped:
            break
        if out["swaps"] == SWAP_CAP:
            out["status"] |= 2
            break
    inside = (s.nz > 0) | (s.held > 0)
    out.update(beta=s.beta, closed=inside, trials=s.trials, nnz=int(np.count_nonzero(s.beta)),
               F=float(-0.5 * s.beta @ (c + s.r) + alpha * np.count_nonzero(inside)))
    return out


def objective(H, c, alpha, beta, gstart, closed):
    return float(0.5 * beta @ H @ beta - c @ beta + alpha * np.count_nonzero(closure(beta, gstart, closed)))


def polish(H, c, big_M, beta, gstart, closed):
    """The exact minimiser of the quadratic on ALL live columns of the groups in cl(S(beta)), inside the box."""
    inside = closure(beta, gstart, closed)
    d = np.diag(H)
    live = d > PIVOT * d.max()
    S = np.array([j for g in np.flatnonzero(inside) for j in range(gstart[g], gstart[g + 1]) if live[j] or beta[j] != 0.0], dtype=int)
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


def is_group_swap_inescapable(H, c, alpha, big_M, beta, gstart, closed, tol, swaps=True):
    """From ``beta`` alone: every live column of a group in cl(S) sits at its one-coordinate value; every group that holds
    non-zeros is worth its price; no inactive group that passes the screen is worth its price once fitted; and (``swaps``) no
    scanned swap would be accepted -- each within ``tol``, relative to the decision's own scale.  Returns ``(ok, why)``."""
    H = np.asarray(H, dtype=float)
    c = np.asarray(c, dtype=float)
    beta = np.asarray(beta, dtype=float)
    yy_free_tol = 0.0  # (the inner passes of a trial fit run to their cap: a zero tolerance)
    base = _State(H, c, gstart, closed, alpha, big_M, yy_free_tol, beta)
    if np.any(beta[~base.live] != 0.0) or np.any(np.abs(beta) > big_M):
        return False, "a dead column is active or a coefficient is outside the box"
    ng = base.ng

    def fresh():
        t = _State(H, c, gstart, closed, alpha, big_M, yy_free_tol, beta)
        return t

    for g in range(ng):
        if base.nz[g] > 0 or base.held[g] > 0:
            for j in base.cols(g):
                if not base.live[j]:
                    continue
                b, _ = _gain(base.r[j] + base.d[j] * beta[j], base.d[j], big_M)
                if abs(b - beta[j]) > tol * max(abs(b), abs(beta[j])):
                    return False, f"column {j} of group {g} is not at its one-coordinate value: {beta[j]} against {b}"
        if base.nz[g] > 0:
            v, _ = base.value(g)
            m = base.price(g)
            if not v > alpha * m - tol * max(abs(v), alpha * m):
                return False, f"group {g} has value {v} <= alpha m = {alpha * m}"
        elif base.held[g] == 0:
            m, C = base.price(g), base.gains(g)
            if not C > alpha * m / SCREEN + tol * max(C, alpha * m):
                continue  # not screened (or on the screen's edge: the rule may not have tried it)
            t = fresh()
            t.fit(g)
            v, _ = t.value(g)
            if v > alpha * m + tol * max(abs(v), alpha * m):
                return False, f"inactive group {g} passes the screen and is worth {v} > alpha m = {alpha * m}"
    if not swaps:
        return True, ""
    for i in range(ng):
        if base.nz[i] == 0 or base.held[i] > 0:
            continue
        t = fresh()
        mi = t.price(i)
        vi, rp = t.value(i)
        t.empty(i, rp)
        t.nz[i] = 0
        t.held[closed[i]] -= 1
        scores = np.array([t.gains(j) - alpha * t.price(j) if j != i and t.nz[j] == 0 else -np.inf for j in range(ng)])
        if not np.isfinite(scores).any():
            continue
        lead = scores.max()
        scale = max(abs(lead), abs(vi), alpha)
        for j in np.flatnonzero(scores >= lead - tol * scale):  # the candidate, and whatever ties with it within tol
            u = _State(H, c, gstart, closed, alpha, big_M, yy_free_tol, t.beta)
            mj = u.price(j)
            u.fit(j)
            vj, _ = u.value(j)
            if vj - alpha * mj > vi - alpha * mi + SWAP_TOL * max(abs(vi), alpha) + tol * max(abs(vi), abs(vj), alpha):
                return False, f"group {j} (value {vj}, price {mj}) replaces group {i} (value {vi}, price {mi})"
    return True, ""


def brute_force(H, c, alpha, gstart, closed):
    """The minimum of F over ALL closed group supports by unconstrained least squares on their columns (``big_M`` inactive).
    Returns ``(F, the support as a bool per group)``."""
    ng = len(gstart) - 1
    best, arg = 0.0, np.zeros(ng, dtype=bool)
    for bits in itertools.product((False, True), repeat=ng):
        T = np.array(bits)
        if not T.any() or any(T[g] and not all(T[h] for h in closed[g]) for g in range(ng)):
            continue
        S = np.array([j for g in np.flatnonzero(T) for j in range(gstart[g], gstart[g + 1])])
        b = np.linalg.lstsq(H[np.ix_(S, S)], c[S], rcond=None)[0]
        F = float(0.5 * b @ H[np.ix_(S, S)] @ b - c[S] @ b + alpha * T.sum())
        if F < best:
            best, arg = F, T
    return best, arg


def solve_group_cells(X, y, gstart, need, alphas, etas, big_M=100.0, starts=None, swaps=True, sample_weight=None, fit_intercept=False):
    """Every cell ``(alphas[e], etas[e])`` from the zero start (``starts`` None) or from ``starts[e]`` (S x p): the winner by
    (F, then the lowest start), polished on the columns of cl(S).  One dict per cell: ``beta``, ``objective``, ``closed`` (of the
    polished coefficients), ``start``, ``swaps``, ``sweeps``, ``status``, ``trials``, ``margin`` (over every start's run), ``lead``,
    ``F`` (per start), ``H``, ``c``."""
    G, c, yy, _, _ = gram(X, y, sample_weight, fit_intercept)
    p = len(c)
    closed = close_hierarchy(len(gstart) - 1, need)
    cells = []
    for e, (alpha, eta) in enumerate(zip(alphas, etas)):
        H = G + 2.0 * eta * np.eye(p)
        runs = [local_group_search(H, c, gstart, closed, alpha, big_M, yy, None if starts is None else s, swaps)
                for s in ([None] if starts is None else starts[e])]
        F = np.array([run["F"] for run in runs])
        win = int(np.argmin(F))  # (the first of the lowest)
        beta = polish(H, c, big_M, runs[win]["beta"], gstart, closed)
        lead = np.inf if len(F) == 1 else float(np.min(_rel(np.delete(F, win), F[win])))
        cells.append({"beta": beta, "objective": objective(H, c, alpha, beta, gstart, closed), "closed": closure(beta, gstart, closed),
                      "start": win, "swaps": runs[win]["swaps"], "sweeps": runs[win]["sweeps"], "status": runs[win]["status"],
                      "trials": runs[win]["trials"], "margin": min(run["margin"] for run in runs), "F": F, "lead": lead, "H": H, "c": c,
                      "yy": yy, "descent_beta": runs[win]["beta"], "closed_lists": closed})
    return cells


def group_law(seed, n=40, n_groups=7, size=2, rho=0.9, k=2, snr=2.0, spread=True):
    """AR(1) columns with correlation ``rho`` in ``n_groups`` groups of ``size`` consecutive columns; ``k`` true groups spread
    evenly (``spread=False``: the first ``k``, which a chain hierarchy leaves closed), every column of them with a unit coefficient
    of alternating sign; noise at signal-to-noise ratio ``snr``."""
    rng = np.random.default_rng(seed)
    p = n_groups * size
    Z = rng.standard_normal((n, p))
    X = np.empty((n, p))
    X[:, 0] = Z[:, 0]
    for j in range(1, p):
        X[:, j] = rho * X[:, j - 1] + np.sqrt(1.0 - rho * rho) * Z[:, j]
    beta = np.zeros(p)
    for t, g in enumerate(np.linspace(0, n_groups - 1, k).round().astype(int) if spread else range(k)):
        beta[g * size:(g + 1) * size] = (-1.0) ** (t + np.arange(size))
    signal = X @ beta
    y = signal + rng.standard_normal(n) * np.sqrt(np.var(signal) / snr)
    return X, y, np.arange(0, p + 1, size)
