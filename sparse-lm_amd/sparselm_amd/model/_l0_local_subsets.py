"""LOCAL SUBSETS: approximate best subsets of every size for up to 1024 columns, on the GPU (``slm_solve_l0_local_subsets``,
csrc/l0_local_kernels.hpp).

``l0_profile`` returns the proven best support of every size and stops at 64 columns, 128 with ``wide``; ``l0_local_search``
goes to 1024 columns but answers the penalised form only, and an alpha scan of it skips sizes.  This is the cardinality form
beyond 128 columns -- the reference's ``BestSubsetSelection(sparse_bound=k)`` and, with ``eta > 0``,
``RidgedBestSubsetSelection`` (identity Tikhonov matrix, singleton groups) -- as an incumbent: for every cell ``(k, eta)``

    minimise over beta, |beta_j| <= big_M, ||beta||_0 <= k:   Q(beta) = 1/2 beta^T (G + 2 eta I) beta - c^T beta

with ``G = X^T W X / n`` and ``c = X^T W y / n``.  ``Q`` is in the units of
``RidgedBestSubsetSelection.solver_info_["objective"]``: ``_miqp.py`` states the objective of all its classes as
``1/2 beta^T (G + 2 eta W^T W) beta - c^T beta + alpha |S|`` with ``alpha = 0`` for the two best-subset classes, which at
``W = I`` is this ``Q`` (the loss ``1/(2n)||X b - y||^2 + eta ||b||^2`` less its constant ``yy / 2``); ``losses_`` carries
``1/(2n)||X b - y||^2``.

The rule, per problem, from a start of any support size: SHRINK to k columns (the weakest one-coordinate gain leaves), DESCEND
on the support, GROW while there are fewer than k (the outside column with the largest gain enters, if it would move at all),
then one-for-one SWAPS until none helps; ``solver_options={"swaps": False}`` stops before the swaps, which is greedy forward
selection with re-fitting.  NOTHING IS PROVEN: ``proven_optimal_`` is False and on hard designs ``Q`` is often above the
optimum; where the columns fit, ``BestSubsetSelection`` and ``l0_profile`` say by how much.

One launch runs every (cell, start) problem, one wavefront each.  Round 0 starts every cell from zero and from the caller's
``starts``; each further round, up to ``max_rounds``, starts every cell from the winners of its neighbours in size (the next
smaller size's winner is grown, the next larger one's is shrunk) and in ``eta``, and keeps a result only where ``Q`` falls by
more than 1e-12 relative; the rounds stop when no cell improved.  When they stop THAT way and ``sizes`` is ascending and
consecutive, ``objectives_`` is non-increasing in k for each eta: a cell above its smaller neighbour would have been improved
by that neighbour's winner, from which the rule only descends.

Not built: groups and a hierarchy, a Tikhonov matrix, an l1 term, constraints, handing the result to the exact search as its
seed.  (Cross-validation over the sizes: ``l0_local_subsets_cv``, ``model/_l0_local_subsets_cv.py``; groups and a hierarchy in the
penalised form: ``l0_local_group_search``, ``model/_l0_local_groups.py``.)

Import path: ``sparselm_amd.miqp`` (``l0_local_subsets``, ``L0LocalSubsets``).
"""

from __future__ import annotations

import warnings
from numbers import Integral

import numpy as np
from sklearn.exceptions import ConvergenceWarning

from ._l0_local import _IMPROVE, _MAX_PROBLEMS, _PMAX, _first_starts, _grid, _LocalProblem, _neighbour_starts, _options, _round_moves

__all__ = ["l0_local_subsets", "L0LocalSubsets"]


class L0LocalSubsets:
    """What ``l0_local_subsets`` returns: one incumbent per cell of the grid ``sizes_ x etas_``.

    ``coefs_`` (K x E x p: the exact minimiser on each cell's support, inside the box), ``intercepts_``, ``supports_`` (bool, at
    most ``sizes_[k]`` columns each), ``objectives_`` (Q: the units of ``RidgedBestSubsetSelection.solver_info_["objective"]``),
    ``losses_`` (1/(2n)||X b - y||^2 on the fitted rows), ``rounds_`` (rounds run, the first included), ``round_objectives_``
    (rounds_ x K x E: never rising along the first axis), per cell ``swaps_``, ``sweeps_``, ``grows_``, ``drops_`` and
    ``converged_`` of the kept result, and ``proven_optimal_ = False``."""

    proven_optimal_ = False

    def __init__(self, sizes, etas, coefs, intercepts, objectives, losses, rounds, round_objectives, swaps, sweeps, grows, drops, converged):
        self.sizes_ = np.asarray(sizes, dtype=int)
        self.etas_ = np.asarray(etas, dtype=float)
        self.coefs_ = np.asarray(coefs, dtype=float)
        self.intercepts_ = np.asarray(intercepts, dtype=float)
        self.supports_ = self.coefs_ != 0.0
        self.objectives_ = np.asarray(objectives, dtype=float)
        self.losses_ = np.asarray(losses, dtype=float)
        self.rounds_ = int(rounds)
        self.round_objectives_ = np.asarray(round_objectives, dtype=float)
        self.swaps_ = np.asarray(swaps, dtype=int)
        self.sweeps_ = np.asarray(sweeps, dtype=int)
        self.grows_ = np.asarray(grows, dtype=int)
        self.drops_ = np.asarray(drops, dtype=int)
        self.converged_ = np.asarray(converged, dtype=bool)

    def predict(self, X, size_index, eta_index=0):
        """``X @ coefs_[size_index, eta_index] + intercepts_[size_index, eta_index]``."""
        X = np.asarray(X, dtype=float)
        if X.ndim != 2 or X.shape[1] != self.coefs_.shape[2]:
            raise ValueError(f"X must have {self.coefs_.shape[2]} columns")
        return X @ self.coefs_[size_index, eta_index] + self.intercepts_[size_index, eta_index]


def _sizes(values):
    raw = np.atleast_1d(np.asarray(values))
    if raw.ndim != 1 or raw.size == 0 or raw.dtype == bool or not all(isinstance(v, (Integral, np.integer)) for v in raw.tolist()):
        raise ValueError("sizes must be a non-empty list of integers")
    if np.any(raw < 1) or np.any(raw >= 2 ** 31):
        raise ValueError("sizes must be >= 1")
    return raw.astype(np.int64)


def _subsets_grid(sizes, etas, big_M, starts, max_rounds, p, row_sets=1):
    """``(sizes, etas, round-0 starts [K, E, S, p], the moves of a round)``, validated against the launch's limits."""
    ks, et = _sizes(sizes), _grid(etas, "etas")
    K, E = len(ks), len(et)
    if p > _PMAX:
        raise NotImplementedError(f"local subsets takes up to {_PMAX} columns (got {p})")
    first, moves = _first_starts(starts, K, E, p, float(big_M)), _round_moves(K, E, max_rounds)
    most = max(first.shape[2], len(moves))
    if row_sets * K * E * most > _MAX_PROBLEMS:
        raise ValueError(f"{row_sets} row set(s) x {K * E} cells x up to {most} starts each: more than the {_MAX_PROBLEMS} problems of one launch")
    return ks, et, first, moves


def _improved(new, old):
    return new < old - _IMPROVE * np.abs(old)


def l0_local_subsets(X, y, *, sizes, etas=(0.0,), big_M=100, fit_intercept=False, sample_weight=None, starts=None, max_rounds=2,
                     solver_options=None) -> L0LocalSubsets:
    """An incumbent for the best subset of at most k columns at every cell of ``sizes x etas``, for up to 1024 columns.

    ``sizes``: integers >= 1 (a size above the column count is legal); ``etas``: finite, >= 0, the ridge weight of
    ``RidgedBestSubsetSelection`` with an identity Tikhonov matrix.  ``big_M``, ``fit_intercept``, ``sample_weight``: the
    estimators'.  ``starts``: extra starting points for round 0, ``(S, p)`` for every cell or ``(K, E, S, p)``, inside the box,
    of any support size.  ``max_rounds``: rounds after the first in which every cell restarts from its neighbours' winners.
    ``solver_options``: ``device``, ``swaps`` (default True).  ``objectives_`` is in the units of
    ``RidgedBestSubsetSelection.solver_info_["objective"]``.  When the rounds end because no cell improved and ``sizes`` is
    ascending and consecutive, ``objectives_`` is non-increasing in k for each eta.  A ``ConvergenceWarning`` is raised when a
    cell's result ran into a sweep or swap cap.  Nothing is proven optimal."""
    # everything is validated before a device is touched
    swaps, device = _options(solver_options, max_rounds, "local subsets")
    spec = _LocalProblem(big_M=big_M, fit_intercept=fit_intercept, solver_options=device)
    X, y, dev_options, gidx, n_groups, need, _, w = spec._l0_setup(X, y, sample_weight)
    p = X.shape[1]
    ks, et, first, moves = _subsets_grid(sizes, etas, big_M, starts, max_rounds, p)
    K, E = len(ks), len(et)
    big_M = float(big_M)
    cell_size, cell_eta = np.repeat(ks, E), np.tile(et, K)

    with spec._l0_dataset(X, y, w, gidx, n_groups, need, dev_options) as (ds, x_mean, y_mean, _, _):

        def launch(points):
            b, _, o, _, _, info = ds.solve_l0_local_subsets([None], [0], cell_size, cell_eta, big_M=big_M,
                                                            starts=points.reshape(1, K * E, -1, p), swaps=swaps)
            return np.array(b).reshape(K, E, p), np.array(o).reshape(K, E), np.array(info[0], dtype=object).reshape(K, E)

        coefs, objectives, infos = launch(first)
        history = [objectives.copy()]
        for _ in range(int(max_rounds) if moves else 0):
            c2, o2, i2 = launch(_neighbour_starts(coefs, moves))
            better = _improved(o2, objectives)
            coefs[better], objectives[better], infos[better] = c2[better], o2[better], i2[better]
            history.append(objectives.copy())
            if not better.any():
                break
    unconverged = [(a, e) for a in range(K) for e in range(E) if not infos[a, e]["converged"]]
    if unconverged:
        a, e = unconverged[0]
        warnings.warn(f"local subsets ran into a cap in {len(unconverged)} of {K * E} cells (the first: size index {a}, eta index {e}, "
                      f"{infos[a, e]['status']}): their last points are returned", ConvergenceWarning)
    take = np.vectorize(lambda d, k: d[k])
    # (with the estimators' own expression, so that an intercept equals a fitted estimator's on the same coefficients)
    intercepts = np.array([[float(y_mean - np.dot(x_mean, coefs[a, e])) if fit_intercept else 0.0 for e in range(E)] for a in range(K)])
    return L0LocalSubsets(ks, et, coefs, intercepts, objectives, take(infos, "loss").astype(float), len(history), np.array(history),
                          take(infos, "swaps").astype(int), take(infos, "sweeps").astype(int), take(infos, "grows").astype(int),
                          take(infos, "drops").astype(int), take(infos, "converged").astype(bool))
