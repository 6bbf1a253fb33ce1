"""A high-precision reference and a judge for the working-set model solver (ws_solve_kernel / ws_refine_lane).

The solver minimises, over the K positions of the working set W,

    m(x) = g0 . (x - z0) + 1/2 (x - z0)^T G (x - z0) + pen(x),
    pen(x) = sum_k a_k |x_k| + sum_g b_g ||x_g|| + 1/2 sum_g d_g ||x_g||^2

(a, b, d already scaled by the path point: a = sa * a0 and so on; without real groups every position is its own group).  A
``Model`` holds G, g0, z0, the penalty and the group index of the positions.

``model_minimiser`` finds the minimiser to the rounding level of ``np.longdouble``: an accelerated proximal-gradient run in
float64 identifies the face (support, signs, active groups); Newton steps on that face, taken in float64 from residuals
evaluated in long double (iterative refinement), polish it; the result is accepted only if ``model_kkt`` of it, evaluated in
long double, is at rounding level.  For a singular G the point is one of many and only ``value`` is meaningful.

``model_kkt`` is the distance from 0 to the subdifferential of m at x: ``oracle.kkt_residual``'s formula on the model gradient
g0 + G (x - z0), every operation in long double (``oracle.kkt_residual`` itself sums group norms through ``np.bincount``,
which is float64; tests/test_model_solver_cpu.py checks that the two agree).

``settled_bound`` is what a SETTLED solve must meet.  It is derived from the solver's stopping rule, not measured: the solver
stops when

    ||u - v|| <= r := max(WS_INNER_TOL * tol * ||u||, kRoundFloor * (||g0|| / L + ||u||))

and returns x = u = prox_{1/Ls}(v - grad m(v) / Ls).  The optimality condition of the prox puts Ls (v - u) - grad(v) into the
subdifferential of pen at u, so grad(u) - grad(v) + Ls (v - u) lies in the subdifferential of m + pen at u:

    dist(0, d(m + pen)(x)) <= (lambda_max(G) + Ls) ||u - v||,     Ls <= L <= 1.155 lambda_max(G)

(1.155 = 1.05 x 1.1: the start is 1.1 times a power estimate from below, the curvature guard sets L to 1.05 times a quotient
||G dv|| / ||dv|| <= lambda_max).  Hence

    model_kkt(x) <= 2.155 lambda_max(G) r + K eps || |G| |x - z0| + |g0| ||

where the last term allows for the rounding of the K-term products of the solver's own gradient.  L in r is the solver's own
(it reports it: WsCtl::Lw); the tests assert L <= 1.155 lambda_max beside the bound.  With G positive definite
||x - x*|| <= model_kkt(x) / lambda_min(G).  WS_INNER_TOL and kRoundFloor are read from the headers.

``model_value`` (long double) serves the monotone rule for solves that need not settle: m(x) <= m(x_start) + the same
rounding allowance, times max(||x - z0||, ||x_start - z0||) to make it a value.

``transcript_solve`` is a small numpy transcription of the kernel's iteration (power estimate, accelerated steps with the
curvature guard and restarts, the stopping rule, the write-back) that takes one FAULT at a time; ``judge`` applies the bound
and the write-back contract to a result, the transcription's or the GPU's.  tests/test_model_solver_cpu.py shows that the
faultless transcription passes and each fault is flagged.
"""

from __future__ import annotations

import os
import re
import types

import numpy as np

EPS = 2.0**-52
LD = np.longdouble
_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sparse-lm_amd", "csrc")


def _constant(header, name):
    text = open(os.path.join(_CSRC, header)).read()
    m = re.search(r"constexpr\s+(?:int|double)\s+%s\s*=\s*([^;]+);" % name, text)
    assert m, (header, name)
    return float(eval(m.group(1), {"__builtins__": {}}))  # ("16.0 * 2.22e-16": numbers and products only)


WS_INNER_TOL = _constant("ws_kernels.hpp", "WS_INNER_TOL")
WS_INNER_MAX = int(_constant("ws_kernels.hpp", "WS_INNER_MAX"))
WS_KLDS = int(_constant("ws_kernels.hpp", "WS_KLDS"))
WS_KCAP = int(_constant("ws_kernels.hpp", "WS_KCAP"))
WS_MAX_REPEATS = int(_constant("ws_kernels.hpp", "WS_MAX_REPEATS"))
K_ROUND_FLOOR = _constant("tail_kernels.hpp", "kRoundFloor")
L_FACTOR = 1.05 * 1.1  # L <= L_FACTOR * lambda_max (module docstring)


def ws_K(kreal):
    return max(16, (int(kreal) + 15) // 16 * 16)


def ws_tpc(K):
    """Threads per position of the solver's products: 4 up to 256 positions, 2 beyond."""
    return 4 if K <= 256 else 2


class Model:
    """The model on W: G (k, k), g0, z0, a (k,), b, d (groups,), gidx (k,) the group of each position (None: singletons)."""

    def __init__(self, G, g0, z0, a, b=None, d=None, gidx=None):
        self.G = np.asarray(G, dtype=np.float64)
        k = self.G.shape[0]
        self.k = k
        self.g0 = np.asarray(g0, dtype=np.float64).reshape(k)
        self.z0 = np.asarray(z0, dtype=np.float64).reshape(k)
        self.a = np.broadcast_to(np.asarray(a, dtype=np.float64), (k,)).copy()
        self.gidx = np.arange(k) if gidx is None else np.asarray(gidx, dtype=np.int64).reshape(k)
        self.ng = int(self.gidx.max()) + 1
        self.b = np.broadcast_to(np.asarray(0.0 if b is None else b, dtype=np.float64), (self.ng,)).copy()
        self.d = np.broadcast_to(np.asarray(0.0 if d is None else d, dtype=np.float64), (self.ng,)).copy()
        self.members = [np.flatnonzero(self.gidx == g) for g in range(self.ng)]


def _gnorm(x, mdl):
    out = np.zeros(mdl.ng, dtype=x.dtype)
    for g, mem in enumerate(mdl.members):
        out[g] = np.sqrt(np.sum(x[mem] * x[mem]))
    return out


def prox(v, step, mdl):
    """prox of step * pen at v (float64): soft threshold, group shrink, ridge factor -- oracle.penalty.prox on W."""
    u = np.sign(v) * np.maximum(np.abs(v) - step * mdl.a, 0.0)
    nrm = np.sqrt(np.bincount(mdl.gidx, weights=u * u, minlength=mdl.ng))
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.where(nrm > 0.0, np.maximum(0.0, 1.0 - step * mdl.b / nrm), 0.0) / (1.0 + step * mdl.d)
    return u * sc[mdl.gidx]


def model_gradient(mdl, x):
    """g0 + G (x - z0) in long double."""
    return mdl.g0.astype(LD) + mdl.G.astype(LD) @ (np.asarray(x, dtype=LD) - mdl.z0.astype(LD))


def model_value(mdl, x):
    """m(x) + pen(x) relative to the expansion point, long double."""
    x = np.asarray(x, dtype=LD)
    dx = x - mdl.z0.astype(LD)
    nrm = _gnorm(x, mdl)
    smooth = mdl.g0.astype(LD) @ dx + LD(0.5) * (dx @ (mdl.G.astype(LD) @ dx))
    return smooth + np.sum(mdl.a.astype(LD) * np.abs(x)) + np.sum(mdl.b.astype(LD) * nrm) + LD(0.5) * np.sum(mdl.d.astype(LD) * nrm * nrm)


def model_kkt(mdl, x):
    """dist(0, d(m + pen)(x)) in long double (oracle.kkt_residual's formula on the model gradient)."""
    x = np.asarray(x, dtype=LD)
    grad = model_gradient(mdl, x)
    a, b, d = mdl.a.astype(LD), mdl.b.astype(LD), mdl.d.astype(LD)
    nrm = _gnorm(x, mdl)
    total = LD(0.0)
    for g, mem in enumerate(mdl.members):
        if nrm[g] > 0:
            h = grad[mem] + (d[g] + b[g] / nrm[g]) * x[mem]
            viol = np.where(x[mem] != 0, h + a[mem] * np.sign(x[mem]), np.sign(h) * np.maximum(np.abs(h) - a[mem], LD(0.0)))
            total += np.sum(viol * viol)
        else:
            s = np.maximum(np.abs(grad[mem]) - a[mem], LD(0.0))
            total += max(LD(0.0), np.sqrt(np.sum(s * s)) - b[g]) ** 2
    return np.sqrt(total)


def rounding_allowance(mdl, x):
    """K eps || |G| |x - z0| + |g0| ||: the rounding of a K-term gradient on W."""
    return mdl.k * EPS * float(np.linalg.norm(np.abs(mdl.G) @ np.abs(np.asarray(x, dtype=np.float64) - mdl.z0) + np.abs(mdl.g0)))


def spectrum(mdl):
    w = np.linalg.eigvalsh(mdl.G)
    return float(w[0]), float(w[-1])


def settled_bound(mdl, x, tol, L):
    """The bound on model_kkt(x) of a settled solve (module docstring).  L: the curvature bound of the solver's stop rule."""
    x = np.asarray(x, dtype=np.float64)
    lam_max = spectrum(mdl)[1]
    un = float(np.linalg.norm(x))
    r = max(WS_INNER_TOL * tol * un, K_ROUND_FLOOR * (float(np.linalg.norm(mdl.g0)) / L + un))
    return (1.0 + L_FACTOR) * lam_max * r + rounding_allowance(mdl, x)


def _fista(mdl, x0, iters, L):
    x = np.array(x0, dtype=np.float64)
    v, t = x.copy(), 1.0
    for _ in range(iters):
        u = prox(v - (mdl.g0 + mdl.G @ (v - mdl.z0)) / L, 1.0 / L, mdl)
        if (v - u) @ (u - x) > 0.0:
            t = 1.0
        tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        v = u + (t - 1.0) / tn * (u - x)
        if np.array_equal(u, x) and t == 1.0:
            break
        x, t = u, tn
    return x


def _face_residual(mdl, x, free, sgn):
    """Gradient of the smooth restriction of m + pen to the face, on the free positions (long double)."""
    grad = model_gradient(mdl, x)
    nrm = _gnorm(x, mdl)
    safe = np.where(nrm > 0, nrm, LD(1.0))
    h = grad + (mdl.d.astype(LD)[mdl.gidx] + mdl.b.astype(LD)[mdl.gidx] / safe[mdl.gidx]) * x + mdl.a.astype(LD) * sgn
    return h[free]


def _face_hessian(mdl, x, free):
    xf = np.asarray(x, dtype=np.float64)
    H = mdl.G[np.ix_(free, free)].copy()
    H[np.diag_indices_from(H)] += mdl.d[mdl.gidx[free]]
    nrm = np.sqrt(np.bincount(mdl.gidx, weights=xf * xf, minlength=mdl.ng))
    where = {int(k): i for i, k in enumerate(free)}
    for g, mem in enumerate(mdl.members):
        if mdl.b[g] > 0.0 and nrm[g] > 0.0:
            mf = [k for k in mem if int(k) in where]
            ii = [where[int(k)] for k in mf]
            xg = xf[mf]
            H[np.ix_(ii, ii)] += mdl.b[g] * (np.eye(len(mf)) / nrm[g] - np.outer(xg, xg) / nrm[g] ** 3)
    return H


def model_minimiser(mdl, x0=None, iters=20000, polish=40):
    """The minimiser of the model: namespace(x [long double], value, kkt, unique, face_min_eig).  Raises AssertionError when the
    polished point's own KKT residual is not at the rounding level of long double."""
    lam_min, lam_max = spectrum(mdl)
    x = _fista(mdl, mdl.z0 if x0 is None else x0, iters, 1.02 * lam_max)
    eps_ld = float(np.finfo(LD).eps)
    for _ in range(8):  # (a face the polish leaves, or one that is not the minimiser's, is identified again from where it ended)
        free = np.flatnonzero(x != 0.0)
        sgn = np.sign(x).astype(LD)
        xl = x.astype(LD)
        if free.size:
            for _ in range(polish):
                r = _face_residual(mdl, xl, free, sgn)
                if float(np.linalg.norm(r)) == 0.0:
                    break
                H = _face_hessian(mdl, xl, free)
                step = np.linalg.lstsq(H, r.astype(np.float64), rcond=None)[0]
                xn = xl.copy()
                xn[free] -= step.astype(LD)
                if np.any(np.sign(xn[free]) != sgn[free]):
                    break
                xl = xn
        kkt = model_kkt(mdl, xl)
        scale = float(np.linalg.norm(np.abs(mdl.G) @ np.abs(xl.astype(np.float64) - mdl.z0) + np.abs(mdl.g0) + mdl.a + mdl.b[mdl.gidx]))
        if float(kkt) <= 64.0 * mdl.k * eps_ld * scale:
            break
        x = _fista(mdl, xl.astype(np.float64), iters, 1.02 * lam_max)
    assert float(kkt) <= 64.0 * mdl.k * eps_ld * scale, ("the reference did not reach its own rounding level", float(kkt), scale)
    face = 0.0
    if free.size:
        face = float(np.linalg.eigvalsh(_face_hessian(mdl, xl, free))[0])
    return types.SimpleNamespace(x=xl, value=model_value(mdl, xl), kkt=float(kkt), unique=lam_min > 1e-12 * lam_max,
                                 face_min_eig=face, support=free)


# ------------------------------------------------------------------------------------------------------------------------
# transcription of the kernel's iteration, with faults
# ------------------------------------------------------------------------------------------------------------------------
FAULTS = ("drop_nnz_tail", "drop_last_column", "no_z0_shift", "group_norm_short", "group_threshold_pa", "prox_unscaled",
          "no_ridge", "padding_nonzero", "outside_not_reset", "beta_in_mode1")


def transcript_solve(mdl, cols, p, zprev, gprev_full, z_start, tol, mode, fault=None, power_iters=12):
    """The kernel's iteration in numpy on K = ws_K(k) positions (the padding carries zeros), then its write-back into full
    vectors of p features.  ``fault``: one of FAULTS.  Returns a namespace like Dataset.working_set_model_solve's."""
    assert fault is None or fault in FAULTS, fault
    k = mdl.k
    K = ws_K(k)
    tpc = ws_tpc(K)
    G = np.zeros((K, K))
    G[:k, :k] = mdl.G
    z0 = np.zeros(K)
    g0 = np.zeros(K)
    z0[:k], g0[:k] = zprev[cols], gprev_full[cols]
    live = np.arange(K) < k
    a = np.zeros(K)
    a[:k] = mdl.a
    gidx = np.concatenate([mdl.gidx, mdl.ng + np.arange(K - k)])
    ng = mdl.ng + K - k
    b = np.concatenate([mdl.b, np.zeros(K - k)])
    d = np.concatenate([mdl.d, np.zeros(K - k)])
    first = np.array([np.flatnonzero(gidx == g)[0] for g in range(ng)])
    size = np.bincount(gidx, minlength=ng)
    group_pen = bool(np.any(b != 0.0) or np.any(d != 0.0))

    def matvec(val):
        delta = np.where(live, val if fault == "no_z0_shift" else val - z0, 0.0)
        nz = np.flatnonzero(delta)
        use = np.ones(K, dtype=bool)
        if fault == "drop_nnz_tail" and nz.size % (12 * tpc) == 1:
            use[nz[-1]] = False
        if fault == "drop_last_column":
            use[k - 1] = False
        return G[:, use] @ delta[use]

    def prox_w(v, s):
        u = np.where(live, np.sign(v) * np.maximum(np.abs(v) - (1.0 if fault == "prox_unscaled" else s) * a, 0.0), 0.0)
        if group_pen:
            sq = u * u
            if fault == "group_norm_short":
                last = first + size - 1
                short = sq.copy()
                short[last[size > 1]] = 0.0
                sq = short
            nrm = np.sqrt(np.bincount(gidx, weights=sq, minlength=ng))
            thr = np.bincount(gidx, weights=a, minlength=ng) / size if fault == "group_threshold_pa" else b
            with np.errstate(divide="ignore", invalid="ignore"):
                sc = np.where(nrm > 0.0, np.maximum(0.0, 1.0 - s * thr / nrm), 0.0)
            if fault != "no_ridge":
                sc = sc / (1.0 + s * d)
            u = u * sc[gidx]
        return u

    vec = np.where(live, 1.0 + 0.37 * ((((np.arange(K, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)) & np.uint64(0xFF)).astype(np.float64) / 255.0, 0.0)
    lam = 0.0
    for _ in range(power_iters):
        y = G @ vec
        lam = float(np.linalg.norm(y))
        vec = y / lam if lam > 0 else 0 * y
    L = 1.1 * lam
    x = np.zeros(K)
    x[:k] = z_start[cols]
    if fault == "padding_nonzero":
        x[k:] = 1e-3
    x_start = x.copy()
    v, t = x.copy(), 1.0
    scale = float(np.linalg.norm(g0)) / L
    v_prev = gv_prev = None
    settled, n_inner = False, 0
    for _ in range(WS_INNER_MAX):
        n_inner += 1
        gv = g0 + matvec(v)
        u = prox_w(v - gv / L, 1.0 / L)
        if fault == "padding_nonzero":
            u[k:] = 1e-3
        if v_prev is not None:
            dv, dg = v - v_prev, gv - gv_prev
            s4, s5 = float(dv @ dv), float(dg @ dg)
            if s4 > 1e-20 * max(float(u @ u), scale * scale) and np.sqrt(s5 / s4) > L:
                L = 1.05 * np.sqrt(s5 / s4)
                v_prev, gv_prev = v, gv
                v, t = x.copy(), 1.0
                continue
        v_prev, gv_prev = v, gv
        un = float(np.linalg.norm(u))
        conv = float(np.linalg.norm(u - v)) <= max(WS_INNER_TOL * tol * un, K_ROUND_FLOOR * (scale + un))
        t_use = 1.0 if (v - u) @ (u - x) > 0.0 else t
        tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t_use * t_use))
        v = u + (t_use - 1.0) / tn * (u - x)
        x, t = u, tn
        if conv:
            settled = True
            break
    out = types.SimpleNamespace(settled=settled, inner_iters=n_inner, Lw=np.array([L]), served=np.array([0]), x_positions=x.copy())
    z = np.array(z_start, dtype=np.float64)
    beta = np.full(p, np.nan)
    accept = settled or float(model_value(mdl, x[:k])) <= float(model_value(mdl, x_start[:k]))
    if accept:
        outside = np.ones(p, dtype=bool)
        outside[cols] = False
        if fault != "outside_not_reset":
            z[outside] = zprev[outside]
        z[cols] = x[:k]
        if mode == 0 or fault == "beta_in_mode1":
            beta[outside] = zprev[outside]
            beta[cols] = x[:k]
        out.served = np.array([1])
    out.z, out.beta = z[None, :], beta[None, :]
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the judge
# ------------------------------------------------------------------------------------------------------------------------
def check_writeback(cols, zprev, z_start, mode, z, beta, served, padding=None):
    """The write-back contract of one lane.  served: outside W z equals zprev exactly, beta equals z in mode 0 and is
    untouched (NaN) in mode 1; not served: z is the start and beta untouched.  ``padding``: the solver's values on the padding
    positions where they can be seen (the transcription): exactly zero.  Returns a list of violations (empty: none)."""
    bad = []
    p = z.size
    outside = np.ones(p, dtype=bool)
    outside[cols] = False
    if padding is not None and np.any(padding != 0.0):
        bad.append("a padding position holds a non-zero value")
    if not served:
        if not np.array_equal(z, z_start):
            bad.append("not served, but z differs from the start")
        if not np.all(np.isnan(beta)):
            bad.append("not served, but beta was written")
        return bad
    if not np.array_equal(z[outside], zprev[outside]):
        bad.append("outside W z is not the expansion point")
    if not np.all(np.isfinite(z)):
        bad.append("z is not finite")
    if mode == 0:
        if not np.array_equal(beta, z):
            bad.append("mode 0: beta differs from z")
    elif not np.all(np.isnan(beta)):
        bad.append("mode 1: beta was written")
    return bad


def judge_settled(mdl, cols, zprev, z_start, mode, tol, z, beta, served, L, padding=None):
    """A must-settle lane: the write-back contract, settled_bound and -- G positive definite -- the distance bound against the
    reference.  Returns (violations, figures)."""
    bad = check_writeback(cols, zprev, z_start, mode, z, beta, served, padding)
    fig = {}
    if not served:
        return bad + ["the lane was not served"], fig
    x = z[cols]
    kkt = float(model_kkt(mdl, x))
    bound = settled_bound(mdl, x, tol, L)
    lam_min, lam_max = spectrum(mdl)
    fig.update(kkt=kkt, bound=bound, lam_min=lam_min, lam_max=lam_max)
    if not (L <= L_FACTOR * lam_max * (1.0 + 1e-12)):
        bad.append(f"L = {L:.6g} above {L_FACTOR} lambda_max = {L_FACTOR * lam_max:.6g}")
    if not kkt <= bound:
        bad.append(f"model_kkt {kkt:.3e} above settled_bound {bound:.3e}")
    if lam_min > 1e-12 * lam_max:
        ref = model_minimiser(mdl, x0=x)
        dist = float(np.linalg.norm(x.astype(LD) - ref.x))
        fig.update(dist=dist, dist_bound=bound / lam_min, ref=ref)
        if not dist <= bound / lam_min + float(np.linalg.norm(ref.x)) * 4 * EPS:
            bad.append(f"distance to the minimiser {dist:.3e} above bound / lambda_min {bound / lam_min:.3e}")
    return bad, fig


def judge_monotone(mdl, cols, zprev, z_start, mode, z, beta, served):
    """A may-not-settle lane: the write-back contract and m(x) <= m(x_start) + rounding."""
    bad = check_writeback(cols, zprev, z_start, mode, z, beta, served)
    if served:
        x, xs = z[cols], z_start[cols]
        allow = max(rounding_allowance(mdl, x), rounding_allowance(mdl, xs)) * max(float(np.linalg.norm(x - mdl.z0)), float(np.linalg.norm(xs - mdl.z0)))
        m_end, m_start = float(model_value(mdl, x)), float(model_value(mdl, xs))
        if not m_end <= m_start + allow:
            bad.append(f"m(x) = {m_end:.17g} above m(start) = {m_start:.17g} + {allow:.3e}")
    return bad


# ------------------------------------------------------------------------------------------------------------------------
# models for the tests
# ------------------------------------------------------------------------------------------------------------------------
def spd(k, cond, seed):
    """A random symmetric positive definite k x k matrix with eigenvalues spread geometrically over [1/cond, 1] * scale."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((k, k)))
    w = np.geomspace(1.0, 1.0 / cond, k) * (0.5 + rng.random())
    G = (Q * w) @ Q.T
    return 0.5 * (G + G.T)


def pad_gram(G):
    k = G.shape[0]
    K = ws_K(k)
    out = np.zeros((K, K))
    out[:k, :k] = G
    return out


PENALTIES = ("lasso", "weighted_l1_ridge", "group", "sparse_group", "ridged_group")


def make_case(k, p, seed, cond=10.0, penalty="lasso", group_sizes=None, strength=0.3, G=None, tol=1e-10, mode=0, lane=0, gram_seed=None,
              least_squares=False):
    """One lane's inputs on a dataset of p features: W of k positions on scattered features (with ``group_sizes``: W's groups,
    whole and contiguous, the other features in groups of three), distinct values everywhere, the start different from the
    expansion point outside W.  ``seed`` fixes W and the groups, (``seed``, ``lane``) the values, ``gram_seed`` the Gram;
    ``least_squares``: g0 in the range a least-squares loss gives it.  Returns a namespace: cols, gid (None: singletons), n_groups, mdl, gram (padded), zprev, gprev,
    z_start, a0, b0, d0, point, tol, mode."""
    rng = np.random.default_rng(seed)
    grouped = penalty in ("group", "sparse_group", "ridged_group") and group_sizes is not None
    perm = rng.permutation(p)
    if grouped:
        assert sum(group_sizes) == k
        gid = np.full(p, -1, dtype=np.int32)
        order = rng.permutation(len(group_sizes))
        labels = rng.permutation(len(group_sizes))  # (W's groups are not the dataset's first ones in order)
        at, chunks = 0, {}
        for gi, sz in enumerate(group_sizes):
            feats = np.sort(perm[at:at + sz])
            gid[feats] = labels[gi]
            chunks[gi] = feats
            at += sz
        nxt = len(group_sizes)
        rest = perm[at:]
        for i in range(0, rest.size, 3):
            gid[rest[i:i + 3]] = nxt
            nxt += 1
        n_groups = nxt
        cols = np.concatenate([chunks[gi] for gi in order]).astype(np.int32)
        local = np.concatenate([np.full(group_sizes[gi], i) for i, gi in enumerate(order)])
        of_local = np.array([labels[gi] for gi in order])
    else:
        gid, n_groups = None, p
        cols = perm[:k].astype(np.int32)
        local = np.arange(k)
        of_local = cols
    rng = np.random.default_rng([seed, lane, 77])
    Gm = spd(k, cond, seed + 1 if gram_seed is None else gram_seed) if G is None else np.asarray(G, dtype=np.float64)
    g0 = rng.standard_normal(k) * np.sqrt(np.mean(np.diag(Gm)))
    if least_squares:
        # the gradient of a least-squares loss: G (z0 - x_ls) with the unpenalised minimiser x_ls a distance of order one away --
        # its components along G's small eigenvectors are small in proportion (a g0 drawn freely puts the model's minimiser
        # 1 / lambda_min away instead)
        g0 = -Gm @ rng.standard_normal(k)
    zprev = 0.05 * rng.standard_normal(p)
    gprev = rng.standard_normal(p)
    gprev[cols] = g0
    z_start = zprev + 0.01 * rng.standard_normal(p)  # (differs from zprev outside W on purpose)
    z_start[cols[::3]] = 0.0
    a0 = rng.uniform(0.5, 1.5, p)
    b0 = rng.uniform(0.5, 1.5, n_groups)
    d0 = rng.uniform(0.5, 1.5, n_groups)
    lvl = strength * float(np.sqrt(np.mean(g0 * g0)))
    sa, sb, sd = {"lasso": (lvl, 0.0, 0.0), "weighted_l1_ridge": (lvl, 0.0, 0.5 * np.mean(np.diag(Gm))),
                  "group": (0.0, lvl * 1.5, 0.0), "sparse_group": (0.5 * lvl, lvl, 0.0),
                  "ridged_group": (0.0, lvl, 0.5 * np.mean(np.diag(Gm)))}[penalty]
    mdl = Model(Gm, g0, zprev[cols], sa * a0[cols], sb * b0[of_local], sd * d0[of_local], local)
    return types.SimpleNamespace(cols=cols, gid=gid, n_groups=n_groups, mdl=mdl, gram=pad_gram(Gm), zprev=zprev, gprev=gprev,
                                 z_start=z_start, a0=a0, b0=b0, d0=d0, point=np.array([sa, sb, sd]), tol=tol, mode=mode, p=p, k=k)


def support_case(k, p, nnz, seed):
    """A lasso lane whose solution -- and every iterate from its start -- has exactly ``nnz`` non-zero coordinates of x - z0:
    G = I + small, z0 = 0 on W, |g0| far above the threshold on ``nnz`` positions and far below it elsewhere."""
    rng = np.random.default_rng([seed, nnz])
    S = rng.standard_normal((k, k))
    G = np.eye(k) + (0.05 / k) * (S + S.T)
    c = make_case(k, p, seed, penalty="lasso", G=G, tol=1e-8)
    g0 = rng.uniform(0.05, 0.3, k) * rng.choice([-1.0, 1.0], k)
    on = rng.permutation(k)[:nnz]
    g0[on] = rng.uniform(2.0, 3.0, nnz) * rng.choice([-1.0, 1.0], nnz)
    c.zprev[c.cols] = 0.0
    c.z_start[c.cols] = 0.0
    c.z_start[c.cols[on]] = -0.5 * g0[on] * rng.uniform(0.5, 1.0, nnz)
    c.gprev[c.cols] = g0
    c.a0[:] = 1.0
    c.point = np.array([1.0, 0.0, 0.0])
    c.mdl = Model(G, g0, np.zeros(k), np.ones(k))
    c.gram = pad_gram(G)
    c.nnz = nnz
    return c
