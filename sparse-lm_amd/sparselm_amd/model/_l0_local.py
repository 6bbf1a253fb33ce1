"""The l0 LOCAL SEARCH: approximate regularised-l0 fits for up to 1024 columns over a whole (alpha, eta) grid
(``slm_solve_l0_local``, csrc/l0_local_kernels.hpp).

Everything else in ``sparselm_amd.miqp`` is an exact search over supports and stops at 64 columns, 128 with ``wide``.  This
is the other kind of answer, in the spirit of L0Learn (Hazimeh and Mazumder, "Fast best subset selection: coordinate descent
and local combinatorial optimization", 2020): for every cell ``(alpha, eta)``

    minimise over beta, |beta_j| <= big_M:   1/2 beta^T (G + 2 eta I) beta - c^T beta + alpha ||beta||_0

(``solver_info_["objective"]`` of ``RegularizedL0`` / ``L2L0`` with singleton groups) by cyclic coordinate descent with hard
thresholding, then one-for-one swaps until no swap helps.  The result is a local minimum that no single coordinate change and
no single swap improves.  NOTHING IS PROVEN: ``proven_optimal_`` is False, there is no lower bound, and on hard designs
(strongly correlated columns) the objective is often above the optimum -- where the columns fit, the exact estimators say by
how much.

One launch runs every (cell, start) problem, one wavefront each.  Round 0 starts every cell from zero and from the caller's
``starts``; each further round, up to ``max_rounds``, starts every cell from the previous winners of its grid neighbours in
``alpha`` and in ``eta`` and keeps a cell's new result only where the objective improves (by more than 1e-12 relative:
rounding is no improvement); the rounds end early when no cell improved.

Not built: groups and a hierarchy, an l1 term, a general Tikhonov matrix, constraints, handing the result to the exact search
as its seed.  (Cross-validation folds in the launch: ``l0_local_cv``, ``model/_l0_local_cv.py``; a bound on the cardinality, the
best-subset form: ``l0_local_subsets``, ``model/_l0_local_subsets.py``; groups and a hierarchy: ``l0_local_group_search``,
``model/_l0_local_groups.py``; an l1 term: ``l1l0_local_search``, ``model/_l1l0_local.py``.)  (The lower bound this search lacks,
and with it a proven gap per cell: ``l0_local_bound``, ``model/_l0_local_bound.py``; branch and bound on that bound, which
proves a cell optimal where its tree closes: ``l0_local_prove``, ``model/_l0_local_prove.py``.)

Import path: ``sparselm_amd.miqp`` (``l0_local_search``, ``L0LocalPath``).
"""

from __future__ import annotations

import warnings
from numbers import Integral

import numpy as np
from sklearn.exceptions import ConvergenceWarning

from ._miqp import _ExactL0

__all__ = ["l0_local_search", "L0LocalPath"]

_PMAX = 1024  # SLM_L0_LOCAL_PMAX
_MAX_PROBLEMS = 8192  # SLM_L0_LOCAL_MAX_PROBLEMS: (cell, start) problems of one launch
_OPTIONS = {"device", "swaps"}
_IMPROVE = 1e-12  # a round's result replaces a cell's only when it is lower by more than this, relative to max(|objective|, alpha)
_MOVES = ((-1, 0), (1, 0), (0, -1), (0, 1))  # a cell's neighbours: along the grid's first axis (alpha, or the size), in eta


class _LocalProblem(_ExactL0):
    """The arguments of ``l0_local_search`` as an estimator, so that validation, sample-weight normalisation and centring are
    ``_ExactL0``'s own code.  Not exported, never fitted."""

    _parameter_constraints: dict = {"fit_intercept": ["boolean"], "solver_options": [dict, None]}
    _hyper_parameter_constraints: dict = {**_ExactL0._hyper_parameter_constraints}

    def __init__(self, groups=None, big_M=100, hierarchy=None, fit_intercept=False, solver_options=None):
        self.groups = groups
        self.big_M = big_M
        self.hierarchy = hierarchy
        self.fit_intercept = fit_intercept
        self.solver_options = solver_options


class L0LocalPath:
    """What ``l0_local_search`` returns: one local minimum per cell of the grid ``alphas_ x etas_``.

    ``coefs_`` (A x E x p: the exact minimiser on each cell's support, inside the box), ``intercepts_``, ``supports_`` (bool),
    ``objectives_`` (the units of ``RegularizedL0.solver_info_["objective"]``), ``losses_`` (1/(2n)||X b - y||^2 on the fitted
    rows), ``rounds_`` (rounds run, the first included), ``round_objectives_`` (rounds_ x A x E: never rising along the first
    axis), per cell ``swaps_``, ``sweeps_`` and ``converged_`` of the kept result, and ``proven_optimal_ = False``."""

    proven_optimal_ = False

    def __init__(self, alphas, etas, coefs, intercepts, objectives, losses, rounds, round_objectives, swaps, sweeps, converged):
        self.alphas_ = np.asarray(alphas, dtype=float)
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
        self.converged_ = np.asarray(converged, dtype=bool)

    def predict(self, X, alpha_index, eta_index=0):
        """``X @ coefs_[alpha_index, eta_index] + intercepts_[alpha_index, eta_index]``."""
        X = np.asarray(X, dtype=float)
        if X.ndim != 2 or X.shape[1] != self.coefs_.shape[2]:
            raise ValueError(f"X must have {self.coefs_.shape[2]} columns")
        return X @ self.coefs_[alpha_index, eta_index] + self.intercepts_[alpha_index, eta_index]


def _grid(values, name):
    arr = np.atleast_1d(np.asarray(values, dtype=float))
    if arr.ndim != 1 or arr.size == 0:
        raise ValueError(f"{name} must be a non-empty list of numbers")
    if not np.all(np.isfinite(arr)) or np.any(arr < 0.0):
        raise ValueError(f"{name} must be finite and >= 0")
    return arr


def _options(solver_options, max_rounds, what="the l0 local search"):
    """``(swaps, the device options or None)`` of a call, validated.  ``what``: the caller, as its messages name it."""
    options = {} if solver_options is None else solver_options
    if not isinstance(options, dict):
        raise ValueError("solver_options must be a dict or None")
    unknown = set(options) - _OPTIONS
    if unknown:
        raise ValueError(f"unknown solver_options {sorted(unknown)}: {what} takes {sorted(_OPTIONS)}")
    swaps = options.get("swaps", True)
    if not isinstance(swaps, (bool, np.bool_)):
        raise ValueError("solver_options['swaps'] must be a bool")
    if not isinstance(max_rounds, Integral) or isinstance(max_rounds, bool) or max_rounds < 0:
        raise ValueError("max_rounds must be an integer >= 0")
    return bool(swaps), {k: v for k, v in options.items() if k == "device"} or None


def _first_starts(starts, A, E, p, big_M):
    """Round 0's starts, [A, E, S, p]: the zero start, then the caller's -- ``(S, p)`` for every cell or ``(A, E, S, p)``."""
    first = np.zeros((A, E, 1, p))
    if starts is None:
        return first
    st = np.asarray(starts, dtype=float)
    if st.ndim == 2 and st.shape[1] == p:
        st = np.broadcast_to(st, (A, E) + st.shape)
    if st.ndim != 4 or st.shape[:2] != (A, E) or st.shape[3] != p:
        raise ValueError(f"starts must have the shape (S, {p}) or ({A}, {E}, S, {p})")
    if not np.all(np.abs(st) <= big_M):  # (a NaN fails too)
        raise ValueError(f"starts must lie inside the box |beta_j| <= big_M = {big_M:g}")
    return np.concatenate([first, st], axis=2)


def _round_moves(A, E, max_rounds):
    """The neighbours a round starts every cell from: none without rounds, or along an axis of length one."""
    return [(da, de) for da, de in _MOVES if (A > 1 and da) or (E > 1 and de)] if max_rounds else []


def _neighbour_starts(coefs, moves):
    """``coefs``: [..., A, E, p].  Every cell's starts of a round: its neighbours' winners, [..., A, E, len(moves), p]; beyond the
    grid's edge the cell's own winner stands in."""
    A, E = coefs.shape[-3], coefs.shape[-2]
    return np.stack([np.take(np.take(coefs, np.clip(np.arange(A) + da, 0, A - 1), axis=-3), np.clip(np.arange(E) + de, 0, E - 1), axis=-2)
                     for da, de in moves], axis=-2)


def _search_rounds(ds, al, et, big_M, first, moves, max_rounds, swaps):
    """The rounds of ``l0_local_search`` on the open dataset ``ds`` (``l0_local_prove`` runs them on its own handle for its
    incumbents): ``(coefs [A, E, p], objectives [A, E], infos [A, E], the objectives after every round)``."""
    A, E, p = len(al), len(et), first.shape[-1]
    cell_alpha, cell_eta = np.repeat(al, E), np.tile(et, A)

    def launch(points):
        return ds.solve_l0_local(cell_alpha, cell_eta, big_M=big_M, starts=points.reshape(A * E, -1, p), swaps=swaps)

    coefs, objectives, _, infos = launch(first)
    coefs = np.array(coefs).reshape(A, E, p)
    objectives = np.array(objectives).reshape(A, E)
    infos = np.array(infos, dtype=object).reshape(A, E)
    history = [objectives.copy()]
    for _ in range(int(max_rounds) if moves else 0):
        c2, o2, _, i2 = launch(_neighbour_starts(coefs, moves))
        c2, o2 = np.array(c2).reshape(A, E, p), np.array(o2).reshape(A, E)
        better = o2 < objectives - _IMPROVE * np.maximum(np.abs(objectives), al[:, None])
        coefs[better], objectives[better] = c2[better], o2[better]
        infos[better] = np.array(i2, dtype=object).reshape(A, E)[better]
        history.append(objectives.copy())
        if not better.any():
            break
    return coefs, objectives, infos, history


def l0_local_search(X, y, *, alphas, etas=(0.0,), big_M=100, fit_intercept=False, sample_weight=None, starts=None, max_rounds=2,
                    solver_options=None) -> L0LocalPath:
    """A local minimum of the regularised l0 problem at every cell of ``alphas x etas``, for up to 1024 columns, on the GPU.

    ``alphas``, ``etas``: the grid (finite, >= 0); ``eta`` is the ridge weight of ``L2L0`` with an identity Tikhonov matrix.
    ``big_M``, ``fit_intercept``, ``sample_weight``: the estimators'.  ``starts``: extra starting points for round 0, ``(S, p)``
    for every cell or ``(A, E, S, p)``, inside the box.  ``max_rounds``: rounds after the first in which every cell restarts
    from its grid neighbours' winners.  ``solver_options``: ``device``, ``swaps`` (default True; False stops every problem at
    its descent's fixed point).  A ``ConvergenceWarning`` is raised when a cell's result ran into a sweep or swap cap.  Nothing
    is proven optimal."""
    swaps, device = _options(solver_options, max_rounds)
    spec = _LocalProblem(big_M=big_M, fit_intercept=fit_intercept, solver_options=device)
    # everything is validated before a device is touched
    X, y, dev_options, gidx, n_groups, need, _, w = spec._l0_setup(X, y, sample_weight)
    al, et = _grid(alphas, "alphas"), _grid(etas, "etas")
    A, E, p = len(al), len(et), X.shape[1]
    if p > _PMAX:
        raise NotImplementedError(f"the l0 local search takes up to {_PMAX} columns (got {p})")
    big_M = float(big_M)
    first, moves = _first_starts(starts, A, E, p, big_M), _round_moves(A, E, max_rounds)
    most = max(first.shape[2], len(moves))  # (a round starts a cell from its neighbours in the grid)
    if A * E * most > _MAX_PROBLEMS:
        raise ValueError(f"the grid holds {A * E} cells with up to {most} starts each: more than the {_MAX_PROBLEMS} problems of one launch")

    with spec._l0_dataset(X, y, w, gidx, n_groups, need, dev_options) as (ds, x_mean, y_mean, _, _):
        coefs, objectives, infos, history = _search_rounds(ds, al, et, big_M, first, moves, max_rounds, swaps)
    unconverged = [(a, e) for a in range(A) for e in range(E) if not infos[a, e]["converged"]]
    if unconverged:
        a, e = unconverged[0]
        warnings.warn(f"the local search ran into a cap in {len(unconverged)} of {A * E} cells (the first: alpha index {a}, eta index {e}, "
                      f"{infos[a, e]['status']}): their last points are returned", ConvergenceWarning)
    take = np.vectorize(lambda d, k: d[k])
    # (with the estimators' own expression, so that an intercept equals a fitted estimator's on the same coefficients)
    intercepts = np.array([[float(y_mean - np.dot(x_mean, coefs[a, e])) if fit_intercept else 0.0 for e in range(E)] for a in range(A)])
    return L0LocalPath(al, et, coefs, intercepts, objectives, take(infos, "loss").astype(float), len(history), np.array(history),
                       take(infos, "swaps").astype(int), take(infos, "sweeps").astype(int), take(infos, "converged").astype(bool))
