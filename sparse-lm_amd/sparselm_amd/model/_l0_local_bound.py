"""The LOCAL BOUND: a proven lower bound on the objective the l0 local search minimises, for up to 1024 columns over a whole
(alpha, eta) grid (``slm_solve_l0_local_bound``, csrc/l0_local_bound_kernels.hpp).

``l0_local_search`` returns a support and proves nothing.  This is the missing half: for every cell ``(alpha, eta)`` a number
that is PROVEN to lie at or below

    min over beta, |beta_j| <= big_M:   F(beta) = 1/2 beta^T (G + 2 eta I) beta - c^T beta + alpha ||beta||_0

so that ``gap(path)`` says how far a local minimum can be from the optimum at most.  The indicator is relaxed by the
perspective of the ridge term together with the big-M link (``z_j in [0, 1]``, ``|beta_j| <= big_M z_j``, cost
``eta beta_j^2 / z_j + alpha z_j``), which leaves a separable convex penalty ``phi``; with ``phi*`` its conjugate,
``phi*(t) = max(0, h(t) - alpha)``, ``h(t) = t^2 / (4 eta)`` for ``|t| <= 2 eta big_M``, else ``|t| big_M - eta big_M^2``, and for
EVERY vector ``u``, with ``t = c - G u``,

    L(u) = -1/2 u^T G u - sum_j max(0, h(t_j) - alpha)   <=   min F.

The kernel looks for the ``u`` that makes the bound tightest -- the minimiser of the relaxation, by cyclic coordinate descent,
one wavefront per cell, the whole grid in one launch -- and whatever ``u`` it ends at, the value it returns is a bound.

WHERE IT IS TIGHT AND WHERE NOT: with a ridge (``eta > 0``) or a box that binds the bound is close to the optimum; at
``eta = 0`` under a loose ``big_M`` the bound is weak: the penalty is ``(alpha / big_M) |b|``, next to nothing, and the bound lies
far below the optimum (DESIGN 4d "Local bound" has the measured gaps).  The bound is honest, not always useful.

Not built: groups and a hierarchy, the cardinality form, the l1 entry, row sets (folds), a Tikhonov matrix, strengthening
``eta = 0`` by extracting a diagonal from G, using the bound to prune or to seed the exact search.

Import path: ``sparselm_amd.miqp`` (``l0_local_bound``, ``L0LocalBound``).
"""

from __future__ import annotations

import warnings
from numbers import Integral, Real

import numpy as np
from sklearn.exceptions import ConvergenceWarning

from ._l0_local import _PMAX, L0LocalPath, _grid, _LocalProblem

__all__ = ["l0_local_bound", "L0LocalBound"]

_MAX_CELLS = 8192  # SLM_L0_LOCAL_MAX_PROBLEMS: the cells of one launch
_OPTIONS = {"device"}


class L0LocalBound:
    """What ``l0_local_bound`` returns: one proven lower bound per cell of the grid ``alphas_ x etas_``.

    ``lower_bounds_`` (A x E: at or below the optimum of the cell's l0 problem, in the units of ``L0LocalPath.objectives_``),
    ``relaxed_objectives_`` (the convex relaxation's value at ``relaxed_coefs_``: equal to the bound where ``converged_``),
    ``relaxed_coefs_`` (A x E x p: inside the box, usable as ``starts=`` of ``l0_local_search``), ``sweeps_`` and ``converged_``
    (False: the sweeps ran out before the relaxation was closed; the value is a bound all the same)."""

    def __init__(self, alphas, etas, lower_bounds, relaxed_objectives, relaxed_coefs, sweeps, converged):
        self.alphas_ = np.asarray(alphas, dtype=float)
        self.etas_ = np.asarray(etas, dtype=float)
        self.lower_bounds_ = np.asarray(lower_bounds, dtype=float)
        self.relaxed_objectives_ = np.asarray(relaxed_objectives, dtype=float)
        self.relaxed_coefs_ = np.asarray(relaxed_coefs, dtype=float)
        self.sweeps_ = np.asarray(sweeps, dtype=int)
        self.converged_ = np.asarray(converged, dtype=bool)

    def gap(self, path):
        """``(path.objectives_ - lower_bounds_) / max(|path.objectives_|, alpha)``, A x E: the proven relative distance of
        ``path`` (an ``L0LocalPath`` on the same data, ``big_M`` and grid) from the optimum, never negative beyond rounding.
        Raises when the grids differ."""
        al, et = np.asarray(path.alphas_, dtype=float), np.asarray(path.etas_, dtype=float)
        if al.shape != self.alphas_.shape or et.shape != self.etas_.shape or np.any(al != self.alphas_) or np.any(et != self.etas_):
            raise ValueError("the path and the bound are on different (alpha, eta) grids")
        obj = np.asarray(path.objectives_, dtype=float)
        return (obj - self.lower_bounds_) / np.maximum(np.abs(obj), self.alphas_[:, None])


def _starts(starts, A, E, p):
    """The cells' starting points, [A, E, p], or None: ``(p,)`` for every cell, ``(A, E, p)``, or an ``L0LocalPath``."""
    if starts is None:
        return None
    if isinstance(starts, L0LocalPath):
        starts = starts.coefs_
    st = np.asarray(starts, dtype=float)
    if st.shape == (p,):
        st = np.broadcast_to(st, (A, E, p))
    if st.shape != (A, E, p):
        raise ValueError(f"starts must have the shape ({p},) or ({A}, {E}, {p}), or be an L0LocalPath on this grid")
    if not np.all(np.isfinite(st)):
        raise ValueError("starts must be finite")
    return np.ascontiguousarray(st)


def l0_local_bound(X, y, *, alphas, etas=(0.0,), big_M=100, fit_intercept=False, sample_weight=None, starts=None, gap_tol=1e-9,
                   max_sweeps=None, solver_options=None) -> L0LocalBound:
    """A proven lower bound on the regularised l0 problem at every cell of ``alphas x etas``, for up to 1024 columns, on the GPU.

    The arguments are ``l0_local_search``'s, and validation, centring and weights are the same code, so both see the same
    ``G``, ``c`` and objective units.  ``starts``: where the descent on the relaxation begins -- ``(p,)``, ``(A, E, p)`` or an
    ``L0LocalPath``, whose ``coefs_`` are used; a point outside the box is clipped into it.  ``gap_tol``: a cell ends when the
    relaxation's duality gap is below ``gap_tol * max(|P|, alpha)`` (0: every sweep is run).  ``max_sweeps``: the cap on a
    cell's sweeps (None: 10000).  ``solver_options``: ``device``.  A ``ConvergenceWarning`` is raised when cells ran out of
    sweeps; their values are bounds all the same.  The bound is tight with a ridge or a box that binds and weak at
    ``eta = 0`` under a loose ``big_M``."""
    options = {} if solver_options is None else solver_options
    if not isinstance(options, dict):
        raise ValueError("solver_options must be a dict or None")
    unknown = set(options) - _OPTIONS
    if unknown:
        raise ValueError(f"unknown solver_options {sorted(unknown)}: the l0 local bound takes {sorted(_OPTIONS)}")
    if not isinstance(gap_tol, Real) or isinstance(gap_tol, bool) or not gap_tol >= 0.0:
        raise ValueError("gap_tol must be a number >= 0")
    if max_sweeps is not None and (not isinstance(max_sweeps, Integral) or isinstance(max_sweeps, bool) or max_sweeps < 1):
        raise ValueError("max_sweeps must be an integer >= 1 or None")
    spec = _LocalProblem(big_M=big_M, fit_intercept=fit_intercept, solver_options=options or None)
    # everything is validated before a device is touched
    X, y, dev_options, gidx, n_groups, need, _, w = spec._l0_setup(X, y, sample_weight)
    al, et = _grid(alphas, "alphas"), _grid(etas, "etas")
    A, E, p = len(al), len(et), X.shape[1]
    if p > _PMAX:
        raise NotImplementedError(f"the l0 local bound takes up to {_PMAX} columns (got {p})")
    if A * E > _MAX_CELLS:
        raise ValueError(f"the grid holds {A * E} cells: more than the {_MAX_CELLS} cells of one launch")
    big_M = float(big_M)
    st = _starts(starts, A, E, p)
    cell_alpha, cell_eta = np.repeat(al, E), np.tile(et, A)

    with spec._l0_dataset(X, y, w, gidx, n_groups, need, dev_options) as (ds, _, _, _, _):
        lower, primal, u, stats, infos = ds.solve_l0_local_bound(cell_alpha, cell_eta, big_M=big_M, starts=None if st is None else st.reshape(A * E, p),
                                                                 max_sweeps=0 if max_sweeps is None else int(max_sweeps), gap_tol=float(gap_tol))
    converged = np.array([i["converged"] for i in infos], dtype=bool).reshape(A, E)
    if not converged.all():
        a, e = np.argwhere(~converged)[0]
        warnings.warn(f"the local bound ran out of sweeps in {int((~converged).sum())} of {A * E} cells (the first: alpha index {a}, eta index "
                      f"{e}): the relaxation is not closed there, the values are bounds all the same", ConvergenceWarning)
    return L0LocalBound(al, et, np.array(lower).reshape(A, E), np.array(primal).reshape(A, E), np.array(u).reshape(A, E, p),
                        np.array(stats)[:, 0].reshape(A, E), converged)
