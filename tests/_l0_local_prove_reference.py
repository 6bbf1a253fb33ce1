"""The local proof (``slm_solve_l0_local_nodes``, ``slm_solve_l0_local_prove``) restated in numpy, independently of the engine.

Three things live here.  (1) The mathematics as the issue states it: ``node_lower_bound(G, c, alpha, eta, M, in_, out_, u)`` by
plain numpy products -- the certificate every node result and every leaf of a proof is checked against -- and the covering
check of a set of leaves.  (2) ``node_rule``: the node kernel's own rule, statement by statement in its arithmetic (the wave's
order of summation, an exact fused multiply-add for the rank-one update: both imported from the bound's restatement), so that
kernel, host twin and this restatement agree bit for bit on the same ``G`` and ``c``.  (3) ``tree``: the branch-and-bound tree
restated -- the branching rule, the rounds, the incumbent's polish (``polish_on``: the host's ``l0_ls_polish_on`` in Python
floats, operation for operation), pruning and the reported bound -- so that an engine's ``nodes``, ``rounds``, coefficients and
bounds can be compared exactly.
"""

import math

import numpy as np
from _l0_local_bound_reference import PIVOT, SWEEPS, _coord, cell_constants, fma, wave_sum  # noqa: F401

FREE, IN, OUT = 0, 1, 2
WORDS = 16
MAX_BATCH = 8192
CD_SWEEPS, CD_TOL = 10000, 1e-12  # the boxed descent of the polish (L0_CD_SWEEPS, L0_CD_TOL)


# ---- masks ----------------------------------------------------------------------------------------------------------------------
def to_words(flags):
    """bool [p] -> 16 words of 64 bits: bit ``j & 63`` of word ``j >> 6`` is column ``j``."""
    bits = np.zeros(WORDS * 64, dtype=np.uint8)
    bits[: len(flags)] = np.asarray(flags, dtype=bool)
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


def from_words(words, p):
    w = np.ascontiguousarray(words, dtype="<u8")
    return np.unpackbits(w.view(np.uint8), bitorder="little")[:p].astype(bool)


# ---- (1) the mathematics --------------------------------------------------------------------------------------------------------
def h_of(t, eta, M):
    """The conjugate of eta b^2 on the box |b| <= M."""
    at = np.abs(np.asarray(t, dtype=float))
    if eta > 0.0:
        return np.where(at <= 2.0 * eta * M, at ** 2 / (4.0 * eta), at * M - eta * M ** 2)
    return at * M


def node_lower_bound(G, c, alpha, eta, M, in_, out_, u):
    """L_node(u) = -1/2 u^T G u - sum over FREE of max(0, h(t_j) - alpha) - sum over IN of (h(t_j) - alpha), t = c - G u: at or
    below the minimum of F over the node for every u."""
    u = np.asarray(u, dtype=float)
    in_, out_ = np.asarray(in_, dtype=bool), np.asarray(out_, dtype=bool)
    Gu = G @ u
    v = h_of(c - Gu, eta, M) - alpha
    free = ~in_ & ~out_
    return float(-0.5 * (u @ Gu) - np.sum(np.maximum(v[free], 0.0)) - np.sum(v[in_]))


def objective(G, c, alpha, eta, beta):
    beta = np.asarray(beta, dtype=float)
    return float(0.5 * (beta @ G @ beta) + eta * (beta @ beta) - c @ beta + alpha * np.count_nonzero(beta))


def leaves_cover(in_, out_):
    """Do the leaves ``(in_, out_)`` (bool, leaves x p) partition the space of supports?  Their sum of 2^-depth must be 1 and no
    two may overlap (two leaves overlap unless some column is IN in one and OUT in the other).  Returns (sum, overlapping pairs)."""
    in_, out_ = np.asarray(in_, dtype=bool), np.asarray(out_, dtype=bool)
    depth = in_.sum(axis=1) + out_.sum(axis=1)
    total = float(np.sum(np.ldexp(1.0, -depth)))  # (exact: powers of two, depth <= 1024)
    i8, o8 = in_.astype(np.int32), out_.astype(np.int32)
    apart = (i8 @ o8.T + o8 @ i8.T) > 0
    overlapping = int((~apart).sum() - len(in_)) // 2
    return total, overlapping


# ---- (2) the node kernel's rule in the kernel's arithmetic ------------------------------------------------------------------------
def _node_values(u, t, c, alpha, eta, M, lam, tauc, state):
    ab, at = np.abs(u), np.abs(t)
    free, inn = state == FREE, state == IN
    ph = np.where(ab <= tauc, lam * ab, eta * ab * ab + alpha)
    ph = np.where(free, ph, np.where(inn, eta * u * u + alpha, 0.0))
    if eta > 0.0:
        h = np.where(at <= 2.0 * eta * M, at * at / (4.0 * eta), at * M - eta * M * M)
    else:
        h = np.where(at > 0.0, at * M, 0.0)
    v = h - alpha
    cj = np.where(free, np.where(v > 0.0, v, 0.0), np.where(inn, v, 0.0))
    qp, ql = wave_sum(u * (c + t)), wave_sum(u * (c - t))
    half = -0.5 * qp
    P = half + wave_sum(ph)
    L = -0.5 * ql - wave_sum(cj)
    F = (half + eta * wave_sum(u * u)) + alpha * wave_sum((u != 0.0).astype(float))
    return P, L, F


def _node_coord(s, a, eta, lam, tauc, M, state, plain=False):
    free = _coord(s, a, eta, lam, tauc, M)
    if plain:  # (every live column is FREE: the bound's own step)
        return free
    with np.errstate(divide="ignore", invalid="ignore"):
        b = s / (a + 2.0 * eta)
    fixed = np.where(b < -M, -M, np.where(b > M, M, b))
    return np.where(state == FREE, free, np.where(state == IN, fixed, 0.0))


def _fma_row(w, row, t):
    """``fma(w, row, t)`` for a scalar ``w``: the bound restatement's arithmetic without its broadcasting (the same bits)."""
    w = float(w)
    ph = w * row
    x = 134217729.0 * w
    wh = x - (x - w)
    wl = w - wh
    x = 134217729.0 * row
    rh = x - (x - row)
    rl = row - rh
    pl = ((wh * rh - ph) + wh * rl + wl * rh) + wl * rl
    th = t + ph
    bb = th - t
    tl = (t - (th - bb)) + (ph - bb)
    sm = tl + pl
    bb = sm - tl
    e = (tl - (sm - bb)) + (pl - bb)
    even = (sm.view(np.int64) & 1) == 0
    v = np.where((e != 0.0) & even, np.nextafter(sm, np.where(e > 0.0, np.inf, -np.inf)), sm)
    return th + v


def node_rule(G, c, alpha, eta, M, in_, out_, start=None, max_sweeps=SWEEPS, gap_tol=1e-9):
    """The node kernel's rule on one node.  ``in_``, ``out_``: bool [p].  Returns a dict: ``u``, ``lower`` (max(L_node(u),
    L_node(0)), before the parent's bound), ``primal``, ``upper``, ``sweeps``, ``status``, ``changes``."""
    G = np.asarray(G, dtype=float)
    c = np.asarray(c, dtype=float)
    p = len(c)
    lam, tauc = cell_constants(alpha, eta, M)
    state = np.where(np.asarray(out_, dtype=bool), OUT, np.where(np.asarray(in_, dtype=bool), IN, FREE))
    a = np.diag(G).copy()
    a[~(a > PIVOT * max(0.0, a.max()))] = 0.0
    a[state == OUT] = 0.0
    live = a > 0.0
    u = np.zeros(p)
    L0 = _node_values(u, c, c, alpha, eta, M, lam, tauc, state)[1]

    def build():
        t = c.copy()
        for j in np.flatnonzero(u):
            t = _fma_row(-u[j], G[j], t)
        return t

    if start is not None:
        u[live] = np.clip(np.asarray(start, dtype=float), -M, M)[live]
    t = build()
    plain = not (state[live] == IN).any()
    sweeps = status = changes = 0
    while True:
        if sweeps == max_sweeps:
            status = 1
            break
        cursor = 0
        while cursor < p:
            nb = _node_coord(t + a * u, a, eta, lam, tauc, M, state, plain)
            changed = live & ((nb < u) | (nb > u))
            changed[:cursor] = False
            hit = np.flatnonzero(changed)
            if hit.size == 0:
                break
            j = int(hit[0])
            delta = nb[j] - u[j]
            u[j] = nb[j]
            t = _fma_row(-delta, G[j], t)
            changes += 1
            cursor = j + 1
        sweeps += 1
        P, L, _ = _node_values(u, t, c, alpha, eta, M, lam, tauc, state)
        if P - L <= gap_tol * max(abs(P), alpha):
            break
    t = build()
    P, L, F = _node_values(u, t, c, alpha, eta, M, lam, tauc, state)
    return dict(u=u, lower=L if L > L0 else L0, primal=P, upper=F, sweeps=sweeps, status=status, changes=changes)


# ---- (3) the tree -----------------------------------------------------------------------------------------------------------------
def _boxed(H, c, M, b):
    """The host's l0_boxed(..., polish = true) on the whole of H (m x m lists of floats), operation for operation."""
    m = len(c)
    b = [min(max(x, -M), M) for x in b]
    g = []
    for r in range(m):
        t = -c[r]
        for k in range(m):
            t += H[r][k] * b[k]
        g.append(t)
    for _ in range(CD_SWEEPS):
        maxd = maxb = 0.0
        for k in range(m):
            nb = min(max(b[k] - g[k] / H[k][k], -M), M)
            dk = nb - b[k]
            if dk != 0.0:
                for r in range(m):
                    g[r] += H[r][k] * dk
                b[k] = nb
            maxd = max(maxd, abs(dk))
            maxb = max(maxb, abs(nb))
        if maxd <= CD_TOL * maxb or maxd == 0.0:
            break
    fr = [k for k in range(m) if abs(b[k]) < M]
    if fr and len(fr) < m:
        f = len(fr)
        A = [[H[fr[i]][fr[j]] for j in range(f)] for i in range(f)]
        rhs = []
        for i in range(f):
            t = c[fr[i]]
            for k in range(m):
                if abs(b[k]) >= M:
                    t -= H[fr[i]][k] * b[k]
            rhs.append(t)
        ok = True
        for i in range(f):
            for j in range(i + 1):
                t = A[i][j]
                for k in range(j):
                    t -= A[i][k] * A[j][k]
                if i == j:
                    if not t > 0.0:
                        ok = False
                        break
                    A[i][i] = math.sqrt(t)
                else:
                    A[i][j] = t / A[j][j]
            if not ok:
                break
        if ok:
            for i in range(f):
                t = rhs[i]
                for k in range(i):
                    t -= A[i][k] * rhs[k]
                rhs[i] = t / A[i][i]
            for i in range(f - 1, -1, -1):
                t = rhs[i]
                for k in range(i + 1, f):
                    t -= A[k][i] * rhs[k]
                rhs[i] = t / A[i][i]
            if all(abs(x) <= M for x in rhs):
                for i in range(f):
                    b[fr[i]] = rhs[i]
    val = 0.0
    for r in range(m):
        t = 0.0
        for k in range(m):
            t += H[r][k] * b[k]
        val += b[r] * (0.5 * t - c[r])
    return val, b


def polish_on(G, c, eta, M, cols, beta):
    """The host's l0_ls_polish_on in Python floats, operation for operation.  Returns (the quadratic value, beta polished)."""
    beta = np.array(beta, dtype=float)
    m = len(cols)
    if m == 0:
        return 0.0, beta
    H = [[float(G[cols[a], cols[k]]) + (2.0 * eta if a == k else 0.0) for k in range(m)] for a in range(m)]
    cs = [float(c[j]) for j in cols]
    val, b = _boxed(H, cs, M, [float(beta[j]) for j in cols])
    if all(abs(x) < M for x in b):
        L = [row[:] for row in H]
        ok = True
        for i in range(m):
            for j in range(i + 1):
                t = L[i][j]
                for k in range(j):
                    t -= L[i][k] * L[j][k]
                if i == j:
                    if not t > PIVOT * L[i][i]:
                        ok = False
                        break
                    L[i][i] = math.sqrt(t)
                else:
                    L[i][j] = t / L[j][j]
            if not ok:
                break
        if ok:
            x = cs[:]
            for i in range(m):
                t = x[i]
                for k in range(i):
                    t -= L[i][k] * x[k]
                x[i] = t / L[i][i]
            for i in range(m - 1, -1, -1):
                t = x[i]
                for k in range(i + 1, m):
                    t -= L[k][i] * x[k]
                x[i] = t / L[i][i]
            if all(abs(v) <= M and v != 0.0 for v in x):
                b = x
                val = 0.0
                for a in range(m):
                    t = 0.0
                    for k in range(m):
                        t += H[a][k] * b[k]
                    val += b[a] * (0.5 * t - cs[a])
    beta[list(cols)] = b
    return val, beta


def prove_value(G, c, alpha, eta, beta):
    """The host's l0_prove_value: F(beta) summed over the support in its order."""
    cols = [int(j) for j in np.flatnonzero(beta)]
    val = 0.0
    for r in cols:
        t = 0.0
        for k in cols:
            t += (float(G[r, k]) + (2.0 * eta if r == k else 0.0)) * float(beta[k])
        val += float(beta[r]) * (0.5 * t - float(c[r]))
    return val + alpha * float(len(cols))


def branch(G, c, tauc, in_, out_, u):
    """The column a node is split on (-1: none is FREE)."""
    free = ~in_ & ~out_
    au = np.abs(u)
    if tauc > 0.0:
        q = au / tauc
        z = np.where(q < 1.0, q, 1.0)
    else:
        z = (au > 0.0).astype(float)
    frac = free & (z > 0.0) & (z < 1.0)
    if frac.any():
        d = np.where(frac, np.abs(z - 0.5), np.inf)
        return int(np.argmin(d))  # (the first of equal distances: the lowest index)
    if (free & (au > 0.0)).any():
        return int(np.argmax(np.where(free, au, -1.0)))
    if not free.any():
        return -1
    t = np.array(c, dtype=float)
    for k in np.flatnonzero(u):
        t = t - G[k] * u[k]
    return int(np.argmax(np.where(free, np.abs(t), -1.0)))


def pruned(best, lower, alpha, rel_gap):
    return best - lower <= rel_gap * max(abs(best), alpha)


def tree(G, c, cells, M, incumbents=None, rel_gap=1e-6, max_nodes=20000, width=32, max_sweeps=SWEEPS, bound=None):
    """The host's l0_prove_tree restated.  ``cells``: [(alpha, eta)].  ``bound(cell index, in_, out_, start)`` -> the dict of
    ``node_rule`` (None: ``node_rule`` itself at gap_tol = rel_gap / 100).  Returns a list of dicts per cell (``beta``,
    ``objective``, ``lower_bound``, ``nodes``, ``rounds``, ``status``, ``leaves``: [(in_, out_, u, lower)]) and the batch sizes
    of the launches."""
    G, c = np.asarray(G, dtype=float), np.asarray(c, dtype=float)
    p = len(c)
    if bound is None:
        def bound(e, in_, out_, start):
            return node_rule(G, c, cells[e][0], cells[e][1], M, in_, out_, start=start, max_sweeps=max_sweeps, gap_tol=rel_gap / 100.0)
    T = []
    for e, (alpha, eta) in enumerate(cells):
        t = dict(open=[], beta=np.zeros(p), best=0.0, stuck=np.inf, nodes=0, rounds=0, done=False, limit=False, leaves=[],
                 tauc=cell_constants(alpha, eta, M)[1])
        if incumbents is not None:
            F = prove_value(G, c, alpha, eta, incumbents[e])
            if F < 0.0:
                t["best"], t["beta"] = F, np.array(incumbents[e], dtype=float)
        T.append(t)
    seq, rnd, launches = 0, 0, []
    none = np.zeros(p, dtype=bool)
    while True:
        batch = []  # (cell, in_, out_, parent lower, start)
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
                    lower, _, in_, out_, u = t["open"].pop(0)
                    j = branch(G, c, t["tauc"], in_, out_, u)
                    if j < 0:
                        t["stuck"] = min(t["stuck"], lower)
                        t["leaves"].append((in_, out_, u, lower))
                        continue
                    child_in, child_out = in_.copy(), out_.copy()
                    child_in[j] = True
                    child_out[j] = True
                    batch.append((e, child_in, out_, lower, u))
                    batch.append((e, in_, child_out, lower, u))
                    popped += 1
                if popped:
                    t["rounds"] += 1
                if (not t["open"] or t["limit"]) and popped == 0:
                    t["done"] = True
        rnd += 1
        if not batch:
            continue
        launches.append(len(batch))
        results = []
        for e, in_, out_, parent, start in batch:
            r = bound(e, in_, out_, start)
            results.append((max(r["lower"], parent), r["upper"], np.array(r["u"], dtype=float)))
        for (e, in_, out_, parent, start), (lower, upper, u) in zip(batch, results):
            t = T[e]
            t["nodes"] += 1
            if not upper < t["best"]:
                continue
            alpha, eta = cells[e]
            t["best"], t["beta"] = upper, u.copy()
            quad, pol = polish_on(G, c, eta, M, [int(j) for j in np.flatnonzero(u)], u)
            F = quad + alpha * float(np.count_nonzero(pol))
            if F < t["best"]:
                t["best"], t["beta"] = F, pol
        for (e, in_, out_, parent, start), (lower, upper, u) in zip(batch, results):
            t = T[e]
            if pruned(t["best"], lower, cells[e][0], rel_gap):
                t["leaves"].append((in_, out_, u, lower))
            else:
                t["open"].append((lower, seq, in_, out_, u))
                seq += 1
        for e, t in enumerate(T):
            t["open"].sort(key=lambda nd: (nd[0], nd[1]))
            while t["open"] and pruned(t["best"], t["open"][-1][0], cells[e][0], rel_gap):
                lower, _, in_, out_, u = t["open"].pop()
                t["leaves"].append((in_, out_, u, lower))
    out = []
    for e, t in enumerate(T):
        low = min(t["best"], t["stuck"])
        if t["open"]:
            low = min(low, min(nd[0] for nd in t["open"]))
        optimal = not t["open"] and pruned(t["best"], t["stuck"], cells[e][0], rel_gap)
        out.append(dict(beta=t["beta"], objective=t["best"], lower_bound=low, nodes=t["nodes"], rounds=t["rounds"],
                        status=0 if optimal else 1, leaves=t["leaves"]))
    return out, launches
