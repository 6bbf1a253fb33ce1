"""The local proof with groups (``slm_solve_l0_local_group_nodes``, ``slm_solve_l0_local_group_prove``) restated in numpy,
independently of the engine.

(1) The mathematics as the issue states it: the group penalty ``phi_g`` by a scan of z, its conjugate, ``node_lower_bound`` by
plain numpy products, the objective with ``|cl(S)|``, the covering check of a set of leaves over the CLOSED group supports and
the brute force over closed supports.  (2) ``node_rule``: the group node kernel's rule in its arithmetic (the wave's order of
summation, an exact fused multiply-add for the rank-one update), for a whole BATCH of nodes in lockstep -- every statement is
elementwise over the nodes, so each node sees exactly the sequential rule -- so that kernel, host twin and this restatement
agree bit for bit.  (3) ``tree``: the branch-and-bound tree over group nodes restated.
"""

import itertools

import numpy as np
from _l0_local_bound_reference import PIVOT, SWEEPS, _coord, cell_constants, fma
from _l0_local_groups_reference import close_hierarchy
from _l0_local_prove_reference import FREE, IN, MAX_BATCH, OUT, polish_on, prove_value, pruned  # noqa: F401

BISECT = 48  # L0_GN_BISECT


def group_words(flags):
    """bool [ng] -> 16 words of 64 bits: bit ``g & 63`` of word ``g >> 6`` is group ``g``."""
    bits = np.zeros(16 * 64, dtype=np.uint8)
    bits[: len(flags)] = np.asarray(flags, dtype=bool)
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


# ---- (1) the mathematics --------------------------------------------------------------------------------------------------------
def h_of(t, eta, M):
    at = np.abs(np.asarray(t, dtype=float))
    if eta > 0.0:
        return np.where(at <= 2.0 * eta * M, at ** 2 / (4.0 * eta), at * M - eta * M ** 2)
    return at * M


def phi_g_scan(b, alpha, eta, M, points=200001):
    """phi_g(b) = min over z in [||b||_inf / M, 1] of eta ||b||^2 / z + alpha z, by a scan of z."""
    b = np.asarray(b, dtype=float)
    n2, inf = float(b @ b), float(np.max(np.abs(b)))
    if n2 == 0.0:
        return 0.0
    z = np.linspace(inf / M, 1.0, points)
    return float(np.min(eta * n2 / z + alpha * z))


def phi_g_conj(t, alpha, eta, M):
    """phi_g*(t_g) = max(0, sum_j h(t_j) - alpha)."""
    return max(0.0, float(np.sum(h_of(t, eta, M))) - alpha)


def closure_groups(beta, gstart, closed):
    ng = len(gstart) - 1
    inside = np.zeros(ng, dtype=bool)
    for g in range(ng):
        if np.any(beta[gstart[g]:gstart[g + 1]] != 0.0):
            inside[g] = True
            inside[closed[g]] = True
    return inside


def objective(G, c, alpha, eta, beta, gstart, closed):
    beta = np.asarray(beta, dtype=float)
    return float(0.5 * (beta @ G @ beta) + eta * (beta @ beta) - c @ beta + alpha * np.count_nonzero(closure_groups(beta, gstart, closed)))


def node_lower_bound(G, c, alpha, eta, M, gstart, gin, gout, u):
    """L_node(u): at or below the minimum of F over the node for every u."""
    u = np.asarray(u, dtype=float)
    Gu = G @ u
    hv = h_of(c - Gu, eta, M)
    total = -0.5 * (u @ Gu)
    for g in range(len(gstart) - 1):
        v = float(np.sum(hv[gstart[g]:gstart[g + 1]])) - alpha
        if gin[g]:
            total -= v
        elif not gout[g]:
            total -= max(v, 0.0)
    return float(total)


def closed_supports(ng, closed):
    """Every group support closed under the hierarchy, as bool rows (the empty one first)."""
    rows = []
    for bits in itertools.product((False, True), repeat=ng):
        T = np.array(bits)
        if all(not T[g] or all(T[h] for h in closed[g]) for g in range(ng)):
            rows.append(T)
    return np.array(rows)


def node_brute_force(G, c, alpha, eta, M, gstart, closed, gin, gout):
    """min F over the node by enumeration of the closed supports T with OUT groups outside: box least squares on the columns of
    T, and alpha |T u IN|.  ``M`` must be loose (the unconstrained solve must lie inside the box; asserted)."""
    ng = len(gstart) - 1
    best = np.inf
    H = G + 2.0 * eta * np.eye(len(c))
    for T in closed_supports(ng, closed):
        if np.any(T & gout):
            continue
        S = np.array([j for g in np.flatnonzero(T) for j in range(gstart[g], gstart[g + 1])], dtype=int)
        val = 0.0
        if len(S):
            b = np.linalg.lstsq(H[np.ix_(S, S)], c[S], rcond=None)[0]
            assert np.all(np.abs(b) <= M)
            val = float(0.5 * b @ H[np.ix_(S, S)] @ b - c[S] @ b)
        best = min(best, val + alpha * np.count_nonzero(T | gin))
    return best


def brute_force(G, c, alpha, eta, M, gstart, closed):
    ng = len(gstart) - 1
    none = np.zeros(ng, dtype=bool)
    return node_brute_force(G, c, alpha, eta, M, gstart, closed, none, none)


def leaves_cover(gin, gout, closed):
    """How many leaves hold each CLOSED group support (a leaf holds T when its IN groups lie in T and its OUT groups outside)?
    A proof's leaves partition the closed supports: every count is 1.  Returns the counts."""
    gin, gout = np.asarray(gin, dtype=bool), np.asarray(gout, dtype=bool)
    sup = closed_supports(gin.shape[1], closed)
    inside = ~(gin[None, :, :] & ~sup[:, None, :]).any(axis=2) & ~(gout[None, :, :] & sup[:, None, :]).any(axis=2)
    return inside.sum(axis=1)


# ---- (2) the group node kernel's rule, a batch of nodes in lockstep ----------------------------------------------------------------
def _col(v):
    return np.asarray(v, dtype=float).reshape(-1, 1)


def _h(t, eta, M):
    at = np.abs(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        pos = np.where(at <= 2.0 * eta * M, at * at / (4.0 * eta), at * M - eta * M * M)
    return np.where(eta > 0.0, pos, np.where(at > 0.0, at * M, 0.0))


def _bstar(t, eta, M):
    with np.errstate(divide="ignore", invalid="ignore"):
        b = t / (2.0 * eta)
    pos = np.where(b < -M, -M, np.where(b > M, M, b))
    return np.where(eta > 0.0, pos, np.where(t > 0.0, M, np.where(t < 0.0, -M, 0.0)))


def _jump(S, alpha, eta, M, amax, n):
    dn = float(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = np.where(eta > 0.0, dn * amax * S / eta, dn * dn * amax * M * M)
        e = (S - alpha) / den
    return np.where(S > alpha, np.where(e < 1.0, e, 1.0), 0.0)


def _below(x, mag, a, R, m, alpha, eta, M):
    w = mag - a * x
    with np.errstate(divide="ignore", invalid="ignore"):
        flat = np.where(x > m, alpha / M, 0.0) <= w
        N2 = R + x * x
        inf = np.where(x > m, x, m)
        ridge = 2.0 * eta * x <= w
        link = np.where(x > m, eta * M * (1.0 - R / (x * x)) + alpha / M, 2.0 * eta * M * x / m) <= w
        mid = (w >= 0.0) & (4.0 * alpha * eta * x * x <= w * w * N2)
        out = np.where(eta * N2 >= alpha, ridge, np.where(eta * N2 * M * M <= alpha * inf * inf, link, mid))
    return np.where(eta > 0.0, out, flat)


def _gn_coord(s, a, R, m, alpha, eta, M):
    mag = np.abs(s)
    hi = mag / a
    hi = np.where(hi > M, M, hi)
    lo = np.zeros_like(hi)
    top = _below(hi, mag, a, R, m, alpha, eta, M)
    for _ in range(BISECT):
        mid = 0.5 * (lo + hi)
        ok = _below(mid, mag, a, R, m, alpha, eta, M)
        lo = np.where(ok, mid, lo)
        hi = np.where(ok, hi, mid)
    lo = np.where(top, np.where(mag / a > M, M, mag / a), lo)
    return np.where(s < 0.0, -lo, lo)


def _wave_sums(terms):
    """``wave_sum`` of every row of ``terms`` [N, p]."""
    N, p = terms.shape
    slots = -(-p // 64)
    padded = np.zeros((N, slots * 64))
    padded[:, :p] = terms
    v = np.zeros((N, 64))
    for s in range(slots):
        v = v + padded[:, s * 64:(s + 1) * 64]
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ off]
    return v[:, 0]


def _values(u, t, c, alpha, eta, lam, tauc, M, gstart, state, ncl):
    """(P, L, F) per node; alpha, eta, lam, tauc: [N]; state: [N, ng]."""
    N, p = u.shape
    E = _col(eta)
    sp, sc = np.zeros((N, p)), np.zeros((N, p))
    hv = _h(t, E, M)
    for g in range(len(gstart) - 1):
        lo, hi = int(gstart[g]), int(gstart[g + 1])
        st = state[:, g]
        free, inn = st == FREE, st == IN
        al, et = alpha, eta
        if hi - lo == 1:
            b = u[:, lo]
            ab = np.abs(b)
            ph = np.where(ab <= tauc, lam * ab, et * ab * ab + al)
            ph = np.where(free, ph, np.where(inn, et * b * b + al, 0.0))
            v = hv[:, lo] - al
            cj = np.where(free, np.where(v > 0.0, v, 0.0), np.where(inn, v, 0.0))
        else:
            N2, inf, S = np.zeros(N), np.zeros(N), np.zeros(N)
            for k in range(lo, hi):
                x = u[:, k]
                ax = np.abs(x)
                N2 = N2 + x * x
                inf = np.where(ax > inf, ax, inf)
                S = S + hv[:, k]
            with np.errstate(divide="ignore", invalid="ignore"):
                pos = np.where(et * N2 >= al, et * N2 + al,
                               np.where(et * N2 * M * M <= al * inf * inf, et * M * N2 / inf + al * inf / M, np.sqrt(4.0 * al * et * N2)))
                fr = np.where(N2 > 0.0, np.where(et > 0.0, pos, al * inf / M), 0.0)
            ph = np.where(free, fr, np.where(inn, et * N2 + al, 0.0))
            v = S - al
            cj = np.where(free, np.where(v > 0.0, v, 0.0), np.where(inn, v, 0.0))
        sp[:, lo], sc[:, lo] = ph, cj
    qp, ql = _wave_sums(u * (c + t)), _wave_sums(u * (c - t))
    half = -0.5 * qp
    P = half + _wave_sums(sp)
    L = -0.5 * ql - _wave_sums(sc)
    F = (half + eta * _wave_sums(u * u)) + alpha * ncl
    return P, L, F


def node_rule(G, c, M, gstart, closed, alpha, eta, gin, gout, starts=None, max_sweeps=SWEEPS, gap_tol=1e-9):
    """The group node kernel's rule on a batch of N nodes.  ``alpha``, ``eta``: [N]; ``gin``, ``gout``: bool [N, ng]; ``starts``:
    [N, p] or None.  Returns a dict of arrays: ``u`` [N, p], ``lower`` (max(L_node(u), L_node(0)), before the parent's bound),
    ``primal``, ``upper``, ``sweeps``, ``status``."""
    G, c = np.asarray(G, dtype=float), np.asarray(c, dtype=float)
    alpha, eta = np.asarray(alpha, dtype=float).reshape(-1), np.asarray(eta, dtype=float).reshape(-1)
    gin, gout = np.asarray(gin, dtype=bool), np.asarray(gout, dtype=bool)
    N, p, ng = len(alpha), len(c), len(gstart) - 1
    consts = np.array([cell_constants(a_, e_, M) for a_, e_ in zip(alpha, eta)])
    lam, tauc = consts[:, 0], consts[:, 1]
    gof = np.repeat(np.arange(ng), np.diff(gstart))
    state = np.where(gout, OUT, np.where(gin, IN, FREE))
    diag = np.diag(G).copy()
    amax = max(0.0, float(diag.max()))
    a = np.tile(np.where(diag > PIVOT * amax, diag, 0.0), (N, 1))
    a[state[:, gof] == OUT] = 0.0
    u = np.zeros((N, p))
    t = np.tile(c, (N, 1))
    zero = np.zeros(N)
    L0 = _values(u, t, c, alpha, eta, lam, tauc, M, gstart, state, zero)[1]

    def apply(rows, j, w):  # t[rows] += w G[j], fused
        t[rows] = fma(w.reshape(-1, 1), G[j][None, :], t[rows])

    def build():
        t[:] = c
        for j in range(p):
            rows = np.flatnonzero(u[:, j] != 0.0)
            if rows.size:
                apply(rows, j, -u[rows, j])

    if starts is not None:
        st = np.clip(np.asarray(starts, dtype=float), -M, M)
        u = np.where(a > 0.0, st, 0.0)
    build()
    active = np.ones(N, dtype=bool)
    sweeps, status = np.zeros(N, dtype=int), np.zeros(N, dtype=int)
    while True:
        out = active & (sweeps == max_sweeps)
        status[out] = 1
        active &= ~out
        if not active.any():
            break
        skip = np.zeros(N, dtype=int)
        for j in range(p):
            rows = np.flatnonzero(active & (a[:, j] > 0.0) & (skip <= j))
            if rows.size == 0:
                continue
            g = int(gof[j])
            lo, hi = int(gstart[g]), int(gstart[g + 1])
            st = state[rows, g]
            al, et, aj, uj = alpha[rows], eta[rows], a[rows, j], u[rows, j]
            s = t[rows, j] + aj * uj
            with np.errstate(divide="ignore", invalid="ignore"):
                b = s / (aj + 2.0 * et)
            fixed = np.where(b < -M, -M, np.where(b > M, M, b))
            single = _coord(s, aj, et, lam[rows], tauc[rows], M)
            if hi - lo == 1:
                nb = np.where(st == FREE, single, fixed)
            else:
                R, m, S = np.zeros(rows.size), np.zeros(rows.size), np.zeros(rows.size)
                for k in range(lo, hi):
                    S = S + _h(t[rows, k], et, M)
                    if k == j:
                        continue
                    x = u[rows, k]
                    ax = np.abs(x)
                    R = R + x * x
                    m = np.where(ax > m, ax, m)
                free = st == FREE
                at_zero = free & ~(R > 0.0) & (uj == 0.0)
                eps = _jump(S, al, et, M, amax, hi - lo)
                moved = at_zero & ((eps * _bstar(t[rows, j], et, M)) != 0.0)
                if moved.any():  # the group moves as one: every live column from the t of now, then the columns into t, ascending
                    r = rows[moved]
                    new = {k: np.where(a[r, k] > 0.0, eps[moved] * _bstar(t[r, k], eta[r], M), u[r, k]) for k in range(lo, hi)}
                    for k in range(lo, hi):
                        u[r, k] = new[k]
                    for k in range(lo, hi):
                        rk = r[u[r, k] != 0.0]
                        if rk.size:
                            apply(rk, k, -u[rk, k])
                    skip[r] = hi
                with np.errstate(divide="ignore", invalid="ignore"):
                    inner = np.where(R > 0.0, _gn_coord(s, aj, np.where(R > 0.0, R, 1.0), np.where(R > 0.0, m, 1.0), al, et, M), single)
                nb = np.where(free, inner, fixed)
                nb = np.where(at_zero, uj, nb)  # (a zero group that stays, or one that has just moved: no change here)
            changed = (nb < uj) | (nb > uj)
            if changed.any():
                r = rows[changed]
                delta = nb[changed] - uj[changed]
                u[r, j] = nb[changed]
                apply(r, j, -delta)
        sweeps[active] += 1
        P, L, _ = _values(u, t, c, alpha, eta, lam, tauc, M, gstart, state, zero)
        with np.errstate(invalid="ignore"):
            done = P - L <= gap_tol * np.maximum(np.abs(P), alpha)
        active &= ~done
    build()
    ncl = np.array([float(np.count_nonzero(closure_groups(u[i], gstart, closed))) for i in range(N)])
    P, L, F = _values(u, t, c, alpha, eta, lam, tauc, M, gstart, state, ncl)
    return dict(u=u, lower=np.where(L > L0, L, L0), primal=P, upper=F, sweeps=sweeps, status=status)


# ---- (3) the tree -----------------------------------------------------------------------------------------------------------------
def branch(G, c, alpha, eta, M, tauc, gstart, gin, gout, u):
    """The group a node is split on (-1: none is FREE)."""
    ng = len(gstart) - 1
    pick, dist = -1, 1.0
    for g in range(ng):
        if gin[g] or gout[g]:
            continue
        ug = u[gstart[g]:gstart[g + 1]]
        z = 0.0
        if len(ug) == 1:
            au = abs(float(ug[0]))
            z = (au / tauc if au / tauc < 1.0 else 1.0) if tauc > 0.0 else (1.0 if au > 0.0 else 0.0)
        else:
            N2, inf = 0.0, 0.0
            for x in ug:
                N2 += float(x) * float(x)
                inf = max(inf, abs(float(x)))
            if N2 > 0.0:
                low = inf / M
                if not eta > 0.0:
                    z = low
                else:
                    zs = float(np.sqrt(eta * N2 / alpha)) if alpha > 0.0 else 1.0
                    z = low if zs < low else (1.0 if zs > 1.0 else zs)
        if not 0.0 < z < 1.0:
            continue
        d = abs(z - 0.5)
        if d < dist:
            dist, pick = d, g
    if pick >= 0:
        return pick
    top = 0.0
    for g in range(ng):
        if gin[g] or gout[g]:
            continue
        inf = float(np.max(np.abs(u[gstart[g]:gstart[g + 1]])))
        if inf > top:
            top, pick = inf, g
    if pick >= 0:
        return pick
    t = np.array(c, dtype=float)
    for k in np.flatnonzero(u):
        t = t - G[k] * u[k]
    hv = _h(t, np.float64(eta), M)
    top = -1.0
    for g in range(ng):
        if gin[g] or gout[g]:
            continue
        S = 0.0
        for k in range(gstart[g], gstart[g + 1]):
            S += float(hv[k])
        if S > top:
            top, pick = S, g
    return pick


def group_value(G, c, alpha, eta, beta, gstart, closed):
    """The host's value of an incumbent: the quadratic in l0_prove_value's order plus alpha |cl(S)|."""
    return prove_value(G, c, 0.0, eta, beta) + alpha * float(np.count_nonzero(closure_groups(beta, gstart, closed)))


def tree(G, c, cells, M, gstart, need=None, incumbents=None, rel_gap=1e-6, max_nodes=20000, width=32, max_sweeps=SWEEPS):
    """The host's l0_prove_tree with a group map, restated.  ``cells``: [(alpha, eta)]; ``need``: the direct need lists or None.
    Returns a list of dicts per cell (``beta``, ``objective``, ``lower_bound``, ``nodes``, ``rounds``, ``status``, ``leaves``:
    [(gin, gout, u, lower)]) and the batch sizes of the launches."""
    G, c = np.asarray(G, dtype=float), np.asarray(c, dtype=float)
    p, ng = len(c), len(gstart) - 1
    closed = close_hierarchy(ng, need)
    needed_by = [[h for h in range(ng) if g in closed[h]] for g in range(ng)]
    T = []
    for e, (alpha, eta) in enumerate(cells):
        t = dict(open=[], beta=np.zeros(p), best=0.0, stuck=np.inf, nodes=0, rounds=0, done=False, limit=False, leaves=[],
                 tauc=cell_constants(alpha, eta, M)[1])
        if incumbents is not None:
            F = group_value(G, c, alpha, eta, np.asarray(incumbents[e], dtype=float), gstart, closed)
            if F < 0.0:
                t["best"], t["beta"] = F, np.array(incumbents[e], dtype=float)
        T.append(t)
    seq, rnd, launches = 0, 0, []
    none = np.zeros(ng, dtype=bool)
    while True:
        batch = []  # (cell, gin, gout, parent lower, start)
        if rnd == 0:
            for e in range(len(cells)):
                batch.append((e, none, none, -np.inf, np.zeros(p)))
                T[e]["rounds"] += 1
        else:
            active = sum(not t["done"] for t in T)
            if active == 0:
                break
            fit = max(1, min(width, MAX_BATCH // 2 // active))
            for e, t in enumerate(T):
                if t["done"]:
                    continue
                popped = 0
                while t["open"] and popped < fit:
                    if t["nodes"] + 2 * (popped + 1) > max_nodes:
                        t["limit"] = True
                        break
                    if len(batch) + 2 > MAX_BATCH:
                        break
                    t["open"].sort(key=lambda nd: (nd[0], nd[1]))
                    lower, _, gin, gout, u = t["open"].pop(0)
                    g = branch(G, c, cells[e][0], cells[e][1], M, t["tauc"], gstart, gin, gout, u)
                    if g < 0:
                        t["stuck"] = min(t["stuck"], lower)
                        t["leaves"].append((gin, gout, u, lower))
                        continue
                    child_in, child_out = gin.copy(), gout.copy()
                    child_in[[g] + closed[g]] = True
                    child_out[[g] + needed_by[g]] = True
                    batch.append((e, child_in, gout, lower, u))
                    batch.append((e, gin, child_out, lower, u))
                    popped += 1
                if popped:
                    t["rounds"] += 1
                if (not t["open"] or t["limit"]) and popped == 0:
                    t["done"] = True
        rnd += 1
        if not batch:
            continue
        launches.append(len(batch))
        r = node_rule(G, c, M, gstart, closed, [cells[b[0]][0] for b in batch], [cells[b[0]][1] for b in batch],
                      np.array([b[1] for b in batch]), np.array([b[2] for b in batch]), np.array([b[4] for b in batch]),
                      max_sweeps=max_sweeps, gap_tol=rel_gap / 100.0)
        results = [(max(float(r["lower"][i]), batch[i][3]), float(r["upper"][i]), r["u"][i].copy()) for i in range(len(batch))]
        for (e, gin, gout, parent, start), (lower, upper, u) in zip(batch, results):
            t = T[e]
            t["nodes"] += 1
            if not upper < t["best"]:
                continue
            alpha, eta = cells[e]
            t["best"], t["beta"] = upper, u.copy()
            cols = [j for g in np.flatnonzero(closure_groups(u, gstart, closed)) for j in range(gstart[g], gstart[g + 1])]
            quad, pol = polish_on(G, c, eta, M, cols, u)
            F = quad + alpha * float(np.count_nonzero(closure_groups(pol, gstart, closed)))
            if F < t["best"]:
                t["best"], t["beta"] = F, pol
        for (e, gin, gout, parent, start), (lower, upper, u) in zip(batch, results):
            t = T[e]
            if pruned(t["best"], lower, cells[e][0], rel_gap):
                t["leaves"].append((gin, gout, u, lower))
            else:
                t["open"].append((lower, seq, gin, gout, u))
                seq += 1
        for e, t in enumerate(T):
            t["open"].sort(key=lambda nd: (nd[0], nd[1]))
            while t["open"] and pruned(t["best"], t["open"][-1][0], cells[e][0], rel_gap):
                lower, _, gin, gout, u = t["open"].pop()
                t["leaves"].append((gin, gout, u, lower))
    out = []
    for e, t in enumerate(T):
        low = min(t["best"], t["stuck"])
        if t["open"]:
            low = min(low, min(nd[0] for nd in t["open"]))
        optimal = not t["open"] and pruned(t["best"], t["stuck"], cells[e][0], rel_gap)
        out.append(dict(beta=t["beta"], objective=t["best"], lower_bound=low, nodes=t["nodes"], rounds=t["rounds"],
                        status=0 if optimal else 1, leaves=t["leaves"]))
    return out, launches
