"""The l0 local search WITH AN L1 TERM: approximate ``L1L0`` fits for up to 1024 columns over a whole (alpha, eta) grid
(``slm_solve_l0_local_l1``, ``l0_local_l1_kernel`` in csrc/l0_local_kernels.hpp).

``L1L0`` is solved exactly by the search over supports and stops at 64 columns; ``l1l0_profile`` with ``wide`` reaches 128 columns
and supports of 64.  This is the approximate answer beyond that, the L0L1 penalty of the local-search literature (Hazimeh and
Mazumder, "Fast best subset selection: coordinate descent and local combinatorial optimization", 2020): for every cell
``(alpha, eta)``

    minimise over beta, |beta_j| <= big_M:   1/2 beta^T (G + 2 ridge I) beta - c^T beta + eta ||beta||_1 + alpha ||beta||_0

-- with ``ridge = 0`` it is ``L1L0.solver_info_["objective"]`` with singleton groups (the reference's objective over 2n).  ``eta``
is the L1 WEIGHT, as in ``L1L0`` and ``l1l0_profile``, not the ridge weight that ``l0_local_search`` calls ``eta``; ``ridge`` is one
scalar for the whole grid.  The rule is ``l0_local_search``'s with one change, the coordinate: a soft threshold by ``eta`` before
the clip, and ``eta |b|`` off the gain that is compared with ``alpha`` (csrc/l0_host.hpp, "local search with an l1 term").  With
``eta = 0`` every decision is ``l0_local_search``'s.  The winner of a cell is polished on its support: the soft-threshold descent to
its last digit, then the exact solve on its sign pattern; a coefficient the polish brings to zero comes back as zero.

NOTHING IS PROVEN: ``proven_optimal_`` is False, there is no lower bound, and on hard designs the objective is often above the
optimum -- on a hard law of ten columns the rule reached the optimum in 48 of 72 cases (tests/test_l1l0_local_cpu.py prints the
count).  Where the columns fit, ``L1L0`` and ``l1l0_profile`` say by how much.

Rounds as for ``l0_local_search``: round 0 starts every cell from zero and from the caller's ``starts``; each further round, up to
``max_rounds``, starts every cell from the previous winners of its grid neighbours in ``alpha`` and in ``eta`` and keeps a result
only where the objective improves by more than 1e-12 relative.

Out of scope: groups or a hierarchy with the l1 term, the cardinality form with it, a Tikhonov matrix, constraints, seeding the
exact search, rerouting ``GridSearchCV``.  (Cross-validation: ``l1l0_local_cv``, ``model/_l1l0_local_cv.py``.)

Import path: ``sparselm_amd.miqp`` (``l1l0_local_search``, ``L1L0LocalPath``).
"""

from __future__ import annotations

import warnings
from numbers import Real

import numpy as np
from sklearn.exceptions import ConvergenceWarning

from ._l0_local import _IMPROVE, _MAX_PROBLEMS, _PMAX, L0LocalPath, _first_starts, _grid, _LocalProblem, _neighbour_starts, _options, _round_moves

__all__ = ["l1l0_local_search", "L1L0LocalPath"]

_WHAT = "the l0 local search with an l1 term"


class L1L0LocalPath(L0LocalPath):
    """What ``l1l0_local_search`` returns: ``L0LocalPath``'s tables over the grid ``alphas_ x etas_`` -- ``etas_`` are the L1
    WEIGHTS -- and ``ridge_``.  ``coefs_`` are the polished winners (a coefficient the polish brought to zero is zero, and
    ``supports_`` says so), ``objectives_`` are in the units of ``L1L0.solver_info_["objective"]``, and ``proven_optimal_ = False``."""

    proven_optimal_ = False

    def __init__(self, *tables, ridge=0.0):
        super().__init__(*tables)
        self.ridge_ = float(ridge)


class _L1Plan:
    """The arguments both entries share, validated before a device is touched."""

    def __init__(self, X, y, alphas, etas, ridge, big_M, fit_intercept, sample_weight, starts, max_rounds, solver_options):
        self.swaps, device = _options(solver_options, max_rounds, what=_WHAT)
        self.spec = _LocalProblem(big_M=big_M, fit_intercept=fit_intercept, solver_options=device)
        self.X, self.y, self.dev_options, self.gidx, self.n_groups, self.need, _, self.w = self.spec._l0_setup(X, y, sample_weight)
        self.al, self.et = _grid(alphas, "alphas"), _grid(etas, "etas")
        if not isinstance(ridge, Real) or isinstance(ridge, bool) or not np.isfinite(ridge) or ridge < 0.0:
            raise ValueError("ridge must be one finite number >= 0")
        self.ridge = float(ridge)
        self.A, self.E, self.p = len(self.al), len(self.et), self.X.shape[1]
        if self.p > _PMAX:
            raise NotImplementedError(f"{_WHAT} takes up to {_PMAX} columns (got {self.p})")
        self.big_M = float(big_M)
        self.first, self.moves = _first_starts(starts, self.A, self.E, self.p, self.big_M), _round_moves(self.A, self.E, max_rounds)
        self.most = max(self.first.shape[2], len(self.moves))  # (a round starts a cell from its neighbours in the grid)
        self.cell_alpha, self.cell_l1 = np.repeat(self.al, self.E), np.tile(self.et, self.A)
        self.cell_ridge = np.full(self.A * self.E, self.ridge)


def l1l0_local_search(X, y, *, alphas, etas, ridge=0.0, big_M=100, fit_intercept=False, sample_weight=None, starts=None, max_rounds=2,
                      solver_options=None) -> L1L0LocalPath:
    """A local minimum of the ``L1L0`` problem at every cell of ``alphas x etas``, for up to 1024 columns, on the GPU.

    ``alphas``: the prices of a non-zero coefficient; ``etas``: the L1 WEIGHTS, as in ``L1L0`` and ``l1l0_profile`` (both finite,
    >= 0); ``ridge``: one ridge weight for the whole grid (0: the reference's ``L1L0``).  ``big_M``, ``fit_intercept``,
    ``sample_weight``: the estimators'.  ``starts``, ``max_rounds`` and ``solver_options`` (``device``, ``swaps``) as for
    ``l0_local_search``.  A ``ConvergenceWarning`` is raised when a cell's result ran into a sweep or swap cap.  Nothing is proven
    optimal."""
    # everything is validated before a device is touched
    plan = _L1Plan(X, y, alphas, etas, ridge, big_M, fit_intercept, sample_weight, starts, max_rounds, solver_options)
    A, E, p, al = plan.A, plan.E, plan.p, plan.al
    if A * E * plan.most > _MAX_PROBLEMS:
        raise ValueError(f"the grid holds {A * E} cells with up to {plan.most} starts each: more than the {_MAX_PROBLEMS} problems of one launch")

    with plan.spec._l0_dataset(plan.X, plan.y, plan.w, plan.gidx, plan.n_groups, plan.need, plan.dev_options) as (ds, x_mean, y_mean, _, _):

        def launch(points):
            b, _, o, _, _, info = ds.solve_l0_local_l1([None], [0], plan.cell_alpha, plan.cell_l1, plan.cell_ridge, big_M=plan.big_M,
                                                       starts=points.reshape(1, A * E, -1, p), swaps=plan.swaps)
            return np.array(b).reshape(A, E, p), np.array(o).reshape(A, E), np.array(info[0], dtype=object).reshape(A, E)

        coefs, objectives, infos = launch(plan.first)
        history = [objectives.copy()]
        for _ in range(int(max_rounds) if plan.moves else 0):
            c2, o2, i2 = launch(_neighbour_starts(coefs, plan.moves))
            better = o2 < objectives - _IMPROVE * np.maximum(np.abs(objectives), al[:, None])
            coefs[better], objectives[better], infos[better] = c2[better], o2[better], i2[better]
            history.append(objectives.copy())
            if not better.any():
                break
    unconverged = [(a, e) for a in range(A) for e in range(E) if not infos[a, e]["converged"]]
    if unconverged:
        a, e = unconverged[0]
        warnings.warn(f"{_WHAT} ran into a cap in {len(unconverged)} of {A * E} cells (the first: alpha index {a}, eta index {e}, "
                      f"{infos[a, e]['status']}): their last points are returned", ConvergenceWarning)
    take = np.vectorize(lambda d, k: d[k])
    # (with the estimators' own expression, so that an intercept equals a fitted estimator's on the same coefficients)
    intercepts = np.array([[float(y_mean - np.dot(x_mean, coefs[a, e])) if fit_intercept else 0.0 for e in range(E)] for a in range(A)])
    return L1L0LocalPath(al, plan.et, coefs, intercepts, objectives, take(infos, "loss").astype(float), len(history), np.array(history),
                         take(infos, "swaps").astype(int), take(infos, "sweeps").astype(int), take(infos, "converged").astype(bool),
                         ridge=plan.ridge)
