"""The local bound (``slm_solve_l0_local_bound``) restated in numpy, independently of the engine.

Four things live here.  (1) The mathematics as the issue states it: ``phi``, ``phi_conj`` and ``lower_bound(G, c, alpha, eta, M,
u)`` written from the definitions with plain numpy products -- the certificate every engine result is checked against.  (2) The
relaxation solved by a DIFFERENT algorithm from the kernel's: accelerated proximal gradient (FISTA with restarts) with the closed
prox of ``phi``, run to its own duality gap.  (3) Brute force over all supports inside the box for small ``p``: the optimum the
bound has to stay below.  (4) ``rule``: the kernel's own rule, statement by statement in its arithmetic -- the same order of
operations, the wave's order of summation (``wave_sum``), an exact fused multiply-add for the rank-one update (``fma``) -- so
that kernel, host twin and this restatement agree bit for bit on the same ``G`` and ``c``.
"""

import functools
import itertools

import numpy as np
from _l0_local_reference import gram, hard_law  # noqa: F401  (the law the bound is measured on)

PIVOT = 1e-12
SWEEPS = 10000
GAP_TOL = 1e-9

# the grid of the tests: eta x M x alpha
ETAS = (0.0, 0.01, 1.0)
BIG_MS = (0.7, 100.0)
ALPHAS = (1e-3, 0.1, 0.5)


# ---- (1) the mathematics ------------------------------------------------------------------------------------------------------
def phi(b, alpha, eta, M):
    """The relaxed penalty: min over z in [0, 1] with |b| <= M z of eta b^2 / z + alpha z."""
    ab = np.abs(np.asarray(b, dtype=float))
    tau = np.sqrt(alpha / eta) if eta > 0.0 else np.inf
    if M >= tau:
        return np.where(ab <= tau, 2.0 * np.sqrt(alpha * eta) * ab, eta * ab ** 2 + alpha)
    return (eta * M + alpha / M) * ab


def phi_conj(t, alpha, eta, M):
    """phi*(t) = max(0, h(t) - alpha)."""
    at = np.abs(np.asarray(t, dtype=float))
    if eta > 0.0:
        h = np.where(at <= 2.0 * eta * M, at ** 2 / (4.0 * eta), at * M - eta * M ** 2)
    else:
        h = at * M
    return np.maximum(0.0, h - alpha)


def lower_bound(G, c, alpha, eta, M, u):
    """L(u) = -1/2 u^T G u - sum_j phi*(c_j - (G u)_j): at or below min F for every u."""
    u = np.asarray(u, dtype=float)
    Gu = G @ u
    return float(-0.5 * (u @ Gu) - np.sum(phi_conj(c - Gu, alpha, eta, M)))


def relaxed(G, c, alpha, eta, M, b):
    """P(b) = 1/2 b^T G b - c^T b + sum phi(b_j)."""
    b = np.asarray(b, dtype=float)
    return float(0.5 * (b @ G @ b) - c @ b + np.sum(phi(b, alpha, eta, M)))


def objective(G, c, alpha, eta, beta):
    """F(beta) = 1/2 beta^T (G + 2 eta I) beta - c^T beta + alpha ||beta||_0."""
    beta = np.asarray(beta, dtype=float)
    return float(0.5 * (beta @ G @ beta) + eta * (beta @ beta) - c @ beta + alpha * np.count_nonzero(beta))


# ---- (2) the relaxation by accelerated proximal gradient -----------------------------------------------------------------------
def prox_phi(v, step, alpha, eta, M):
    """argmin over |b| <= M of 1/2 (b - v)^2 + step phi(b), elementwise and in closed form: on phi's linear piece a soft
    threshold, beyond it a shrinkage by the ridge, clipped between the pieces' joint and the box."""
    av = np.abs(v)
    tau = np.sqrt(alpha / eta) if eta > 0.0 else np.inf
    if M >= tau:
        slope, joint = 2.0 * np.sqrt(alpha * eta), tau
    else:
        slope, joint = eta * M + alpha / M, M
    soft = np.maximum(av - step * slope, 0.0)
    far = np.clip(av / (1.0 + 2.0 * eta * step), joint, M)
    return np.sign(v) * np.where(soft <= joint, soft, far)


def fista(G, c, alpha, eta, M, tol=1e-10, max_iter=400000):
    """The relaxation's optimum by FISTA with a restart whenever the value rises.  Stops at its own duality gap
    ``P(b) - L(b) <= tol max(|P(b)|, alpha)``.  Returns ``(P, b, relative gap)``."""
    p = len(c)
    step = 1.0 / max(float(np.linalg.eigvalsh(G)[-1]), 1e-300)
    b = np.zeros(p)
    z, tk = b.copy(), 1.0
    value = relaxed(G, c, alpha, eta, M, b)
    gap = np.inf
    for it in range(max_iter):
        nb = prox_phi(z - step * (G @ z - c), step, alpha, eta, M)
        nv = relaxed(G, c, alpha, eta, M, nb)
        if nv > value:  # restart: a plain proximal step from b
            z, tk = b.copy(), 1.0
            nb = prox_phi(b - step * (G @ b - c), step, alpha, eta, M)
            nv = relaxed(G, c, alpha, eta, M, nb)
        tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * tk * tk))
        z = nb + ((tk - 1.0) / tn) * (nb - b)
        b, tk, value = nb, tn, nv
        if it % 10 == 0:
            gap = (value - lower_bound(G, c, alpha, eta, M, b)) / max(abs(value), alpha)
            if gap <= tol:
                break
    return value, b, gap


# ---- (3) brute force over all supports inside the box --------------------------------------------------------------------------
def _box_qp(H, c, M):
    """min 1/2 b^T H b - c^T b over |b_j| <= M, H positive definite: the free solve where it lies inside, else an exact active-set
    solve (bounded-variable least squares on the Cholesky factor)."""
    b = np.linalg.solve(H, c)
    if np.all(np.abs(b) <= M):
        return float(-0.5 * (c @ b))
    from scipy.optimize import lsq_linear

    R = np.linalg.cholesky(H).T  # H = R^T R
    rhs = np.linalg.solve(R.T, c)
    b = lsq_linear(R, rhs, bounds=(-M, M), method="bvls", tol=1e-15).x
    return float(0.5 * (b @ H @ b) - c @ b)


@functools.lru_cache(maxsize=None)
def _support_table(seed, n, p, eta, M):
    """(sizes, Q_min) over every non-empty support of hard_law(seed, n, p): the box-constrained minimum of the quadratic on it."""
    X, y = hard_law(seed, n=n, p=p)
    G, c, _, _, _ = gram(X, y)
    sizes, values = [], []
    for k in range(1, p + 1):
        for S in itertools.combinations(range(p), k):
            S = np.array(S)
            sizes.append(k)
            values.append(_box_qp(G[np.ix_(S, S)] + 2.0 * eta * np.eye(k), c[S], M))
    return np.array(sizes), np.array(values)


def brute_force(seed, alpha, eta, M, n=30, p=10):
    """F* of the cell on hard_law(seed, n, p): the minimum over all supports (the empty one: 0) of Q_min(S) + alpha |S|."""
    assert p <= 12
    sizes, values = _support_table(seed, n, p, float(eta), float(M))
    return float(min(0.0, np.min(values + alpha * sizes)))


@functools.lru_cache(maxsize=None)
def hard_problem(seed, n=30, p=10):
    X, y = hard_law(seed, n=n, p=p)
    X.setflags(write=False)
    y.setflags(write=False)
    G, c, _, _, _ = gram(X, y)
    return X, y, G, c


def grid_cells():
    """The (eta, M, alpha) cells of the tests, in this order."""
    return [(eta, M, alpha) for eta in ETAS for M in BIG_MS for alpha in ALPHAS]


# ---- (4) the kernel's rule in the kernel's arithmetic --------------------------------------------------------------------------
def _split(a):
    t = 134217729.0 * a  # 2^27 + 1 (Veltkamp)
    hi = t - (t - a)
    return hi, a - hi


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma(a, b, c):
    """round(a * b + c) with ONE rounding, elementwise: the product exactly as a pair (Dekker), the sum of the three parts
    rounded once by way of rounding to odd (Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums", 2008).  No
    overflow or underflow handling: the tests' numbers are far from either."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=float), np.asarray(b, dtype=float), np.asarray(c, dtype=float))
    ph = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    pl = ((ah * bh - ph) + ah * bl + al * bh) + al * bl  # a * b = ph + pl exactly
    th, tl = _two_sum(c, ph)
    s, e = _two_sum(tl, pl)  # v = round-to-odd(tl + pl)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(e > 0.0, np.inf, -np.inf)
    v = np.where((e != 0.0) & even, np.nextafter(s, toward), s)
    return th + v


def wave_sum(terms):
    """The kernel's sum of one term per column: lane j & 63 adds its columns in ascending order from zero, then the butterfly
    v += v[lane ^ off], off = 32 .. 1."""
    terms = np.asarray(terms, dtype=float)
    slots = -(-len(terms) // 64)
    padded = np.zeros(slots * 64)
    padded[: len(terms)] = terms
    v = np.zeros(64)
    for row in padded.reshape(slots, 64):
        v = v + row
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ off]
    return float(v[0])


def cell_constants(alpha, eta, M):
    """(lam, tauc): the slope of phi at zero and min(tau, M), as the host computes them once per cell."""
    if eta > 0.0:
        tau = np.sqrt(alpha / eta)
        if M >= tau:
            return float(2.0 * np.sqrt(alpha * eta)), float(tau)
        return float(eta * M + alpha / M), float(M)
    return float(alpha / M), float(M)


def _coord(s, a, eta, lam, tauc, M):
    with np.errstate(divide="ignore", invalid="ignore"):
        mag = np.abs(s)
        b1 = np.where(mag > lam, (mag - lam) / a, 0.0)
        b2 = mag / (a + 2.0 * eta)
        b2 = np.where(b2 < tauc, tauc, np.where(b2 > M, M, b2))
        out = np.where(b1 <= tauc, b1, b2)
    return np.where(s < 0.0, -out, out)


def _values(u, t, c, alpha, eta, M, lam, tauc):
    ab, at = np.abs(u), np.abs(t)
    ph = np.where(ab <= tauc, lam * ab, eta * ab * ab + alpha)
    if eta > 0.0:
        h = np.where(at <= 2.0 * eta * M, at * at / (4.0 * eta), at * M - eta * M * M)
    else:
        h = np.where(at > 0.0, at * M, 0.0)
    v = h - alpha
    cj = np.where(v > 0.0, v, 0.0)
    P = -0.5 * wave_sum(u * (c + t)) + wave_sum(ph)
    L = -0.5 * wave_sum(u * (c - t)) - wave_sum(cj)
    return P, L


def rule(G, c, alpha, eta, M, start=None, max_sweeps=SWEEPS, gap_tol=GAP_TOL):
    """The kernel's rule on one cell.  Returns a dict: ``u``, ``lower``, ``primal``, ``sweeps``, ``status``, ``changes``, and
    ``gaps``: per sweep the relative gap the stopping rule saw."""
    G = np.asarray(G, dtype=float)
    c = np.asarray(c, dtype=float)
    p = len(c)
    lam, tauc = cell_constants(alpha, eta, M)
    a = np.diag(G).copy()
    a[~(a > PIVOT * max(0.0, a.max()))] = 0.0
    live = a > 0.0
    u = np.zeros(p)
    L0 = _values(u, c, c, alpha, eta, M, lam, tauc)[1]

    def build():
        t = c.copy()
        for j in np.flatnonzero(u):
            t = fma(-u[j], G[j], t)
        return t

    if start is not None:
        u[live] = np.clip(np.asarray(start, dtype=float), -M, M)[live]
    t = build()
    sweeps = status = changes = 0
    gaps = []
    while True:
        if sweeps == max_sweeps:
            status = 1
            break
        cursor = 0
        while cursor < p:
            nb = _coord(t + a * u, a, eta, lam, tauc, M)
            changed = live & ((nb < u) | (nb > u))
            changed[:cursor] = False
            hit = np.flatnonzero(changed)
            if hit.size == 0:
                break
            j = int(hit[0])
            delta = nb[j] - u[j]
            u[j] = nb[j]
            t = fma(-delta, G[j], t)
            changes += 1
            cursor = j + 1
        sweeps += 1
        P, L = _values(u, t, c, alpha, eta, M, lam, tauc)
        gaps.append((P - L) / max(abs(P), alpha) if max(abs(P), alpha) > 0.0 else 0.0)
        if P - L <= gap_tol * max(abs(P), alpha):
            break
    t = build()
    P, L = _values(u, t, c, alpha, eta, M, lam, tauc)
    return dict(u=u, lower=L if L > L0 else L0, primal=P, sweeps=sweeps, status=status, changes=changes, gaps=gaps, L0=L0)


def certificate_tolerance(G, alpha, u, L):
    """What separates an engine's ``lower`` from ``lower_bound`` at the same u: p <= 1024 terms at double rounding, with a wide
    margin -- 1e-10 max(|L|, alpha, 1/2 u^T G u)."""
    u = np.asarray(u, dtype=float)
    return 1e-10 * max(abs(L), alpha, 0.5 * float(u @ G @ u))
