"""Linear constraints on the coefficients: ``lo <= A coef <= hi`` beside any penalty of the family.

The reference appends constraints to its cvxpy problem (src/sparselm/model/_base.py:469-510, ``add_constraints``); its
cluster-expansion example keeps the ground states on the predicted convex hull with them (examples/plot_chull.py:160-185).
Here they are ``scipy.optimize.LinearConstraint`` / ``Bounds`` objects, stacked into one ``A`` (m x p) with bounds
``lo`` and ``hi``, and the problem

    minimise 1/(2n)||X b - y||^2 + penalty(b)   subject to   lo <= A b <= hi

is solved by the over-relaxed splitting of ``_split.py`` with ``A`` in place of ``M`` and a clip in place of the group
shrink (alternating direction method of multipliers; ``s`` the copy of ``A b``, ``u`` the scaled multiplier):

    b  <- argmin 1/(2n)||X b - y||^2 + penalty(b) + rho/2 ||A b - s + u||^2
    v  =  A b;   vh = 1.6 v + (1 - 1.6) s
    s  <- clip(vh + u, lo, hi);   u <- u + vh - s;   lambda = rho u

The b-step is the estimator's own penalty on the design ``[X; sqrt(n rho) A]`` with targets ``sqrt(n rho) (s - u)`` in
the last rows: every penalty of the family (group, sparse-group, ridged, overlap) takes it.  ONE upload, then per sweep
new targets (``set_targets``) and a warm-started engine solve; a change of ``rho`` is carried by the row weights of the
constraint rows (``set_row_weights``: X is not uploaded again).  ``rho`` starts where ``rho A^T A`` has the trace of
``X^T X / n`` and is re-balanced at the sweeps of ``_split.py``.  The sweeps stop when ``||A b - s|| <= tol * ep`` and
``rho ||A^T (s - s_prev)|| <= tol * ed``, with ``ep = max(||A b||, ||s||, kap ||b||)`` (``kap`` the rms column norm of
A: a constraint binding at zero still has a scale) and ``ed = max(rho ||A^T u||, ||X^T y|| / n)`` (inactive constraints
leave ``u = 0``) -- and when ``rho ||A^T (A b - s)||``, the step of ``A^T lambda`` in the sweep, is below ``tol * ed`` too
(with every row pinned at a bound ``s`` stops moving, and the dual residual with it, before the multipliers settle).
At the solution ``0 in grad f + d penalty + A^T lambda``: ``lambda > 0`` only where ``hi`` binds, ``< 0`` only where
``lo`` binds.

The l1 estimators on the problem sizes of the on-chip solver run all sweeps in one launch (``slm_solve_constrained``,
csrc/small_constrained_kernels.hpp); the sweeps below are the general route and the A/B partner of that kernel
(``solver_options={"on_chip": False}``).
"""

from __future__ import annotations

import warnings

import numpy as np

from .._backend import default_tol, get_backend

_REBALANCE_AT = (5, 10, 20, 40, 80, 160, 320)
_RELAX = 1.6
_MAX_SWEEPS = 5000
_CHIP_P, _CHIP_NLD, _CHIP_M = 128, 131072, 512  # the scope of slm_solve_constrained


class ConstraintSet:
    """Every constraint object stacked: ``A`` (m x p), ``lo``, ``hi``, and for each object the rows of ``A`` it kept
    (``rows[k]``: indices into the object's own rows; a row with both sides infinite is dropped)."""

    def __init__(self, A, lo, hi, sizes, kept):
        self.A, self.lo, self.hi = A, lo, hi
        self.sizes, self.kept = sizes, kept

    @property
    def m(self):
        return self.A.shape[0]

    def split(self, lam):
        """Multipliers of the stacked rows -> one array per constraint object (zero on dropped rows)."""
        out, r0 = [], 0
        for size, kept in zip(self.sizes, self.kept):
            v = np.zeros(size)
            v[kept] = lam[r0:r0 + len(kept)]
            r0 += len(kept)
            out.append(v)
        return out

    def violation(self, coef):
        """Largest violation of ``lo <= A coef <= hi``."""
        if not self.m:
            return 0.0
        v = self.A @ coef
        return float(max(0.0, np.max(self.lo - v), np.max(v - self.hi)))


def _as_list(constraints):
    from scipy.optimize import Bounds, LinearConstraint

    if isinstance(constraints, (LinearConstraint, Bounds)):
        return [constraints]
    if isinstance(constraints, (list, tuple)):
        return list(constraints)
    raise TypeError(
        f"constraints must be scipy.optimize.LinearConstraint / Bounds objects or a list of them, not "
        f"{type(constraints).__name__}: write a cvxpy constraint such as `beta >= 0` as "
        "scipy.optimize.Bounds(0, np.inf) and `A @ beta <= ub` as scipy.optimize.LinearConstraint(A, -np.inf, ub)"
    )


def stack_constraints(constraints, n_features):
    """Validate and stack ``constraints`` (see ``ProxRegressor``) for ``n_features`` coefficients: ``TypeError`` for
    anything that is not a scipy constraint, ``ValueError`` for a wrong column count, ``lb > ub`` or a non-finite ``A``."""
    from scipy.optimize import Bounds, LinearConstraint

    p = int(n_features)
    blocks, sizes, kept = [], [], []
    for k, c in enumerate(_as_list(constraints)):
        if isinstance(c, LinearConstraint):
            A = c.A
            if hasattr(A, "toarray"):  # scipy.sparse
                A = A.toarray()
            A = np.atleast_2d(np.asarray(A, dtype=np.float64))
            if A.ndim != 2:
                raise ValueError(f"constraint {k}: A must be a matrix")
        elif isinstance(c, Bounds):
            A = np.eye(p)
        else:
            _as_list(c)  # (raises the TypeError that names the scipy form)
            raise TypeError(f"constraint {k} is a list inside the list of constraints")
        if A.shape[1] != p:
            raise ValueError(f"constraint {k}: A has {A.shape[1]} columns, the design has {p} features")
        if not np.all(np.isfinite(A)):
            raise ValueError(f"constraint {k}: A contains a NaN or an infinity")
        m = A.shape[0]
        lb = np.broadcast_to(np.asarray(c.lb, dtype=np.float64), (m,)).copy()
        ub = np.broadcast_to(np.asarray(c.ub, dtype=np.float64), (m,)).copy()
        if np.any(np.isnan(lb)) or np.any(np.isnan(ub)):
            raise ValueError(f"constraint {k}: a bound is NaN")
        if np.any(lb > ub):
            raise ValueError(f"constraint {k}: lb > ub in row(s) {np.flatnonzero(lb > ub).tolist()}")
        keep = np.flatnonzero(np.isfinite(lb) | np.isfinite(ub))
        blocks.append((A[keep], lb[keep], ub[keep]))
        sizes.append(m)
        kept.append(keep)
    if blocks:
        A = np.vstack([b[0] for b in blocks])
        lo = np.concatenate([b[1] for b in blocks])
        hi = np.concatenate([b[2] for b in blocks])
    else:
        A, lo, hi = np.zeros((0, p)), np.zeros(0), np.zeros(0)
    return ConstraintSet(A, lo, hi, sizes, kept)


def check_feasible(cs):
    """``ValueError`` when no coefficient vector satisfies every constraint (HiGHS, zero objective)."""
    if not cs.m:
        return
    from scipy.optimize import linprog

    A, lo, hi = cs.A, cs.lo, cs.hi
    eq = lo == hi
    up = ~eq & np.isfinite(hi)
    dn = ~eq & np.isfinite(lo)
    A_ub = np.vstack([A[up], -A[dn]])
    b_ub = np.concatenate([hi[up], -lo[dn]])
    res = linprog(
        np.zeros(A.shape[1]),
        A_ub=A_ub if len(b_ub) else None, b_ub=b_ub if len(b_ub) else None,
        A_eq=A[eq] if eq.any() else None, b_eq=lo[eq] if eq.any() else None,
        bounds=(None, None), method="highs",
    )
    if res.status == 2:
        raise ValueError("the constraints are infeasible: no coefficient vector satisfies all of them")


class ConstrainedProblem:
    """Looks like a backend problem (``solve(a, b, d, beta0, want_group_norms)``, ``close()``) to the estimators; every
    ``solve`` is a run of the splitting above, continuing from the splitting variables of the solve before (the
    re-weighting rounds of the adaptive estimators).  ``multipliers`` / ``info`` describe the last solve."""

    def __init__(self, X, y, gidx, n_groups, A, lo, hi, options):
        X = np.asarray(X, dtype=np.float64)
        self.X, self.y = X, np.asarray(y, dtype=np.float64)
        self.n, self.p = X.shape
        self.gidx, self.G = gidx, int(n_groups)
        self.A = np.ascontiguousarray(A, dtype=np.float64)
        self.lo, self.hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        self.m = self.A.shape[0]
        self.options = dict(options)
        self.multipliers = np.zeros(self.m)
        self.info = None
        # scales of the stopping rule and the first rho (the same on both routes)
        trK = float(np.sum(self.A * self.A))
        trG = float(np.sum(X * X)) / self.n
        self.rho0 = trG / trK if trK > 0.0 and trG > 0.0 else 1.0 / self.n
        self.kap = np.sqrt(trK / max(self.p, 1))
        self.cnorm = float(np.linalg.norm(X.T @ self.y)) / self.n
        self.inner = None
        self.dev = None
        self.dev_warm = False
        ld = (self.p + 15) // 16 * 16
        if (self.options.get("on_chip", True) is not False and gidx is None and self.p <= _CHIP_P
                and self.n * ld <= _CHIP_NLD and 0 < self.m <= _CHIP_M):
            self.dev = get_backend().problem(self.X, self.y, None, self.p, self.options)
            if not hasattr(getattr(self.dev, "ds", None), "solve_constrained"):  # (the tests' CPU stand-in)
                self.dev.close()
                self.dev = None
        self.s = None
        self.u = np.zeros(self.m)
        self.rho = self.rho0

    # ---- on chip --------------------------------------------------------------------------------------------------
    def _solve_on_chip(self, a, beta0, tol):
        o = self.options
        try:
            beta, lam, rec = self.dev.ds.solve_constrained(
                a, self.A, self.lo, self.hi, beta0=beta0, warm=self.dev_warm, tol=tol,
                tol_inner=float(o["tol"]) if "tol" in o else min(tol, 1e-10), max_sweeps=_MAX_SWEEPS,
            )
        except NotImplementedError:
            return None
        self.dev_warm = True
        if int(rec["status"]) != 0:
            return None
        self.multipliers = lam
        return beta, {"n_iter": int(rec["n_iter"]), "converged": True, "resid": float(rec["resid"]),
                      "inner_iterations": int(rec["rejects"]), "rho": float(rec["L"]), "route": "on_chip",
                      "sweeps": int(rec["n_iter"]), "primal_residual": float(rec["kkt"]),
                      "dual_residual": float(rec["mu"]), "launches": 1, "loss": float(rec["loss"])}

    # ---- general route --------------------------------------------------------------------------------------------
    def _host_setup(self):
        self.scale = np.sqrt((self.n + self.m) / self.n)  # the engine's loss is 1/(2 rows)
        self.root = np.sqrt(self.n * self.rho0)           # the constraint rows carry rho0; rho / rho0 is their row weight
        Xa = self.scale * np.vstack([self.X, self.root * self.A])
        ya = self.scale * np.concatenate([self.y, np.zeros(self.m)])
        inner_options = dict(self.options)
        inner_options.setdefault("tol", min(default_tol(self.n, self.p), 1e-10))
        # (not through the dataset cache: the targets and row weights of this dataset change under it)
        self.inner = get_backend().problem(Xa, ya, self.gidx, self.G, inner_options, cache=False)
        self.inner_rho = self.rho0
        if self.rho != self.rho0:
            self._set_rho()

    def _set_rho(self):
        if hasattr(self.inner, "set_row_weights"):
            w = np.ones(self.n + self.m)
            w[self.n:] = self.rho / self.rho0
            self.inner.set_row_weights(w)
        else:  # (a backend without row weights: the design again, with the new rho in its rows)
            self.inner.close()
            self.root = np.sqrt(self.n * self.rho)
            self.rho0 = self.rho
            Xa = self.scale * np.vstack([self.X, self.root * self.A])
            self.inner = get_backend().problem(Xa, self._targets(), self.gidx, self.G, self.inner.options, cache=False)
        self.inner_rho = self.rho

    def _targets(self):
        return self.scale * np.concatenate([self.y, self.root * (self.s - self.u)])

    def solve(self, a, b, d, beta0=None, want_group_norms=False):
        p, G = self.p, self.G
        a = np.zeros(p) if a is None else np.asarray(a, dtype=np.float64)
        b = np.zeros(G) if b is None else np.asarray(b, dtype=np.float64)
        d = np.zeros(G) if d is None else np.asarray(d, dtype=np.float64)
        tol = float(self.options.get("tol", default_tol(self.n, self.p)))
        beta = None if beta0 is None else np.asarray(beta0, dtype=np.float64)
        if self.dev is not None and not np.any(b) and not np.any(d) and not want_group_norms:
            done = self._solve_on_chip(a, beta, tol)
            if done is not None:
                self.info = done[1]
                return done[0], None, done[1]
            self.dev.close()  # (not a problem for the kernel: the sweeps below take this and every later call)
            self.dev = None
        if self.inner is None:
            self.s = np.clip(self.A @ beta if beta is not None else np.zeros(self.m), self.lo, self.hi)
            self._host_setup()
        inner_iters = 0
        converged = False
        rp = rd = np.inf
        sweeps = 0
        gn = None
        for sweeps in range(1, _MAX_SWEEPS + 1):
            self.inner.set_targets(self._targets())
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")  # an inner solve short of its tolerance is absorbed by the sweeps
                beta, gn, info = self.inner.solve(a, b, d, beta0=beta, want_group_norms=want_group_norms)
            inner_iters += int(info.get("n_iter", 0))
            v = self.A @ beta
            vh = _RELAX * v + (1.0 - _RELAX) * self.s
            s_new = np.clip(vh + self.u, self.lo, self.hi)
            self.u = self.u + vh - s_new
            rp = np.linalg.norm(v - s_new)
            rd = self.rho * np.linalg.norm(self.A.T @ (s_new - self.s))
            rm = self.rho * np.linalg.norm(self.A.T @ (v - s_new))  # how far A^T lambda still moves
            self.s = s_new
            ep = max(np.linalg.norm(v), np.linalg.norm(self.s), self.kap * np.linalg.norm(beta), 1e-300)
            ed = max(self.rho * np.linalg.norm(self.A.T @ self.u), self.cnorm, 1e-300)
            if rp <= tol * ep and rd <= tol * ed and rm <= tol * ed:
                converged = True
                break
            if sweeps in _REBALANCE_AT:
                ratio = (rp / ep) / max(max(rd, rm) / ed, 1e-300)
                if ratio > 5.0 or ratio < 0.2:
                    factor = min(10.0, max(0.1, np.sqrt(ratio)))
                    self.u = self.u / factor  # u is the multiplier divided by rho
                    self.rho *= factor
                    self._set_rho()
        if not converged:
            from sklearn.exceptions import ConvergenceWarning

            warnings.warn(
                f"the splitting for the linear constraints did not reach tol={tol:g} in {sweeps} sweeps "
                f"(primal residual {rp:.3e}, dual residual {rd:.3e})",
                ConvergenceWarning,
            )
        self.multipliers = self.rho * self.u
        self.info = {"n_iter": sweeps, "converged": converged, "resid": float(max(rp, rd)),
                     "inner_iterations": inner_iters, "rho": float(self.rho), "route": "host", "sweeps": sweeps,
                     "primal_residual": float(rp), "dual_residual": float(rd), "launches": None}
        return beta, gn, self.info

    def close(self):
        if self.dev is not None:
            self.dev.close()
            self.dev = None
        if self.inner is not None:
            self.inner.close()
            self.inner = None
