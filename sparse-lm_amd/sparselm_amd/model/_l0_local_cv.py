"""The l0 local search, cross-validated: every fold's (alpha, eta) grid and the grid of all rows from ONE launch per round
(``slm_solve_l0_local_folds``, csrc/l0_local_kernels.hpp).

``l0_local_search`` returns a local minimum at every cell of a grid and says nothing about which cell to use.  A
cross-validation asks the same grid of every fold's training rows, and a refit asks it of all rows: ``l0_local_cv`` builds ONE
dataset (of ``[X | 1]`` when an intercept is fitted -- the engine eliminates that column per row set, which is centring by the
set's own weighted means), hands the folds' training masks and the all-rows set to one call per round, and scores every cell of
every fold on its held-out rows with numpy.  Round 0 and each neighbour round of ``l0_local_search`` run over all row sets at
once; each row set's cells start from THAT row set's neighbours' winners, and a result is kept under the same 1e-12 rule.  A
whole cross-validation is therefore 1 + rounds launches, whatever the number of folds.  ``L0LocalCV.search`` then reads the
grid off the scores: scikit-learn-shaped ``cv_results_``, the selection rules of ``model_selection.py``, and the selected model
from the grid of all rows.

Against ``l0_local_search`` on a fold's rows alone the supports and objectives agree (objectives to 1e-10 where no decision of
the rule is closer than that to a tie); the coefficients are NOT the same bytes: a fold's Gram is built from the complement of
its held-out rows, and centring is by elimination of the ones column instead of on the rows.  Nothing is proven optimal.

Limits: the local search's 1024 columns, at most 15 splits (folds plus all rows fill the Gram store's 16 entries),
``(splits + 1) x cells x starts <= 8192`` problems per launch; held-out scores are unweighted.  Not built: groups, an l1 term,
rerouting ``GridSearchCV``.  (A bound on the cardinality: ``l0_local_subsets_cv``; groups and a hierarchy: ``l0_local_group_cv``; an l1
term: ``l1l0_local_cv``.)

Import path: ``sparselm_amd.miqp`` (``l0_local_cv``, ``L0LocalCV``).
"""

from __future__ import annotations

import warnings

import numpy as np
from sklearn.exceptions import ConvergenceWarning
from sklearn.model_selection import check_cv

from ._l0_cv import _SCORINGS, _SELECTIONS, MAX_SPLITS, _score
from ._l0_local import _IMPROVE, _MAX_PROBLEMS, _PMAX, L0LocalPath, _first_starts, _grid, _LocalProblem, _neighbour_starts, _options, _round_moves

__all__ = ["l0_local_cv", "L0LocalCV"]


class L0LocalSearch:
    """What ``L0LocalCV.search`` returns: ``cv_results_`` in scikit-learn's layout (``params``, ``split{f}_test_score``,
    ``mean_test_score``, ``std_test_score``, ``rank_test_score``), ``best_index_``, ``best_params_``, ``best_score_``,
    ``best_score_std_``, and the selected model from the grid of all rows: ``coef_``, ``intercept_``, ``predict``.
    ``proven_optimal_`` is False: the model is a local minimum."""

    proven_optimal_ = False

    def __init__(self, cv_results, best_index, coef, intercept):
        self.cv_results_ = cv_results
        self.best_index_ = int(best_index)
        self.best_params_ = cv_results["params"][self.best_index_]
        self.best_score_ = cv_results["mean_test_score"][self.best_index_]
        self.best_score_std_ = cv_results["std_test_score"][self.best_index_]
        self.coef_, self.intercept_ = coef, intercept

    def predict(self, X):
        return np.asarray(X, dtype=np.float64) @ self.coef_ + self.intercept_


class L0LocalCV:
    """What ``l0_local_cv`` returns: ``paths_`` (one ``L0LocalPath`` per fold, on its training rows), ``full_`` (the
    ``L0LocalPath`` of all rows), ``splits_`` (``(train, test)`` index pairs), ``cell_scores_`` (folds x A x E: the unweighted
    held-out score of each cell's fit), ``alphas_``, ``etas_``, ``scoring_``, ``solver_info_`` (``launches``; ``rounds``;
    ``problems``: the problems of one launch at most; ``max_sweeps`` and ``max_swaps``: the largest counts of ANY problem of the
    call, a losing start included, beside ``winner_max_sweeps`` / ``winner_max_swaps`` of the kept results;
    ``proven_optimal``: False) and ``proven_optimal_ = False``."""

    proven_optimal_ = False

    def __init__(self, paths, full, splits, cell_scores, scoring, solver_info):
        self.paths_ = paths
        self.full_ = full
        self.splits_ = splits
        self.cell_scores_ = cell_scores
        self.alphas_, self.etas_ = full.alphas_, full.etas_
        self.scoring_ = scoring
        self.solver_info_ = solver_info

    def search(self, opt_selection_method="max_score"):
        """The grid ``alphas_ x etas_`` read off ``cell_scores_``: an ``L0LocalSearch`` whose ``cv_results_["params"]`` are
        ``{"alpha", "eta"}`` dicts in the order of ``ParameterGrid({"alpha": alphas_, "eta": etas_})`` -- ``alpha`` outermost --
        under either selection rule of ``model_selection.py``; the selected model is ``full_``'s at the chosen cell."""
        from ..model_selection import _format_results, select_best_index_onestd

        if opt_selection_method not in _SELECTIONS:
            raise ValueError(f"opt_selection_method must be one of {list(_SELECTIONS)} (got {opt_selection_method!r})")
        A, E = len(self.alphas_), len(self.etas_)
        params = [{"alpha": float(a), "eta": float(e)} for a in self.alphas_ for e in self.etas_]
        scores = np.asarray(self.cell_scores_, dtype=float).reshape(len(self.paths_), A * E).T
        results = _format_results(params, scores, np.zeros_like(scores))
        if opt_selection_method == "one_std_score":
            best = select_best_index_onestd(results)
        else:
            best = int(results["rank_test_score"].argmin())
        a, e = divmod(int(best), E)
        return L0LocalSearch(results, best, self.full_.coefs_[a, e].copy(), float(self.full_.intercepts_[a, e]))


def _fold_splits(cv, X, y, name):
    """The ``(train, test)`` index pairs of ``cv`` (anything ``check_cv`` takes): 1 .. 15 of them."""
    splitter = check_cv(cv, y, classifier=False)
    n_splits = int(splitter.get_n_splits(X, y))
    if not 1 <= n_splits <= MAX_SPLITS:
        raise ValueError(f"{name} takes 1 .. {MAX_SPLITS} splits (got {n_splits}): the folds and all rows share one launch of "
                         f"at most {MAX_SPLITS + 1} row sets")
    return [(np.asarray(tr), np.asarray(te)) for tr, te in splitter.split(X, y)]


def _row_sets(splits, n, w):
    """``(row_weights, n_effs)`` of the folds' training rows, then all rows: the sample weights on a set's rows, scaled to sum
    to its row count."""
    base = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    row_weights, n_effs = [], []
    for rows in [tr for tr, _ in splits] + [np.arange(n)]:
        m = np.zeros(n)
        m[rows] = base[rows]
        total = float(m.sum())
        if not total > 0.0:
            raise ValueError("a training set has no weight")
        row_weights.append(m * (len(rows) / total))
        n_effs.append(len(rows))
    return row_weights, n_effs


def _held_out_scores(scoring, X, y, splits, paths):
    """folds x A x E: the unweighted score of every cell of ``paths[f]`` on fold f's held-out rows, by numpy."""
    A, E = paths[0].coefs_.shape[:2]
    scores = np.empty((len(splits), A, E))
    for f, (_, te) in enumerate(splits):
        for a in range(A):
            for e in range(E):
                scores[f, a, e] = _score(scoring, y[te] - (X[te] @ paths[f].coefs_[a, e] + paths[f].intercepts_[a, e]))
    return scores


def _cv_rounds(X, y, splits, w, fit_intercept, device, solve, first, moves, max_rounds, improved):
    """The launches of a cross-validation, for both forms of the local search: ONE dataset (of ``[X | 1]`` with an intercept),
    round 0 from ``first`` [A, E, S, p] on every row set -- the folds' training rows, then all rows -- and up to ``max_rounds``
    rounds that start every cell from its neighbours' winners IN ITS OWN ROW SET and keep a result where ``improved(new, old)``.
    ``solve(ds, row_weights, n_effs, starts [R, A * E, S, p])`` is the dataset's call.  Returns ``(coefs [R, A, E, p], intercepts,
    objectives, infos [R, A, E], history [rounds, R, A, E], the launch counts of solver_info)``."""
    from .. import _engine

    n, R = len(X), len(splits) + 1
    A, E, _, p = first.shape
    row_weights, n_effs = _row_sets(splits, n, w)  # the folds' training rows, then all rows
    eng = _engine.get_engine(device)
    Xd = np.hstack([X, np.ones((n, 1))]) if fit_intercept else X
    counts = {"launches": 0, "rounds": 0, "problems": 0, "max_sweeps": 0, "max_swaps": 0}
    with eng.dataset(Xd, y) as ds:

        def launch(points):  # points: R x A x E x S x p
            b, i, o, _, stats, info = solve(ds, row_weights, n_effs, points.reshape(R, A * E, -1, p))
            counts["launches"] += 1
            counts["problems"] = max(counts["problems"], stats.shape[0] * stats.shape[1] * stats.shape[2])
            counts["max_sweeps"] = max(counts["max_sweeps"], int(stats[..., 0].max()))
            counts["max_swaps"] = max(counts["max_swaps"], int(stats[..., 1].max()))
            return (np.array(b).reshape(R, A, E, p), np.array(i).reshape(R, A, E), np.array(o).reshape(R, A, E),
                    np.array(info, dtype=object).reshape(R, A, E))

        coefs, icpts, objectives, infos = launch(np.broadcast_to(first, (R,) + first.shape))
        history = [objectives.copy()]
        for _ in range(int(max_rounds) if moves else 0):
            c2, i2, o2, f2 = launch(_neighbour_starts(coefs, moves))
            better = improved(o2, objectives)
            coefs[better], icpts[better], objectives[better], infos[better] = c2[better], i2[better], o2[better], f2[better]
            history.append(objectives.copy())
            if not better.any():
                break
    counts["rounds"] = len(history)
    return coefs, icpts, objectives, infos, np.array(history), counts


def _warn_capped(infos, what, axis):
    """One ``ConvergenceWarning`` for the (row set, cell) pairs whose kept result ran into a cap.  ``what``: the caller, ``axis``:
    its grid's first axis, as the message names them."""
    R, A, E = infos.shape
    names = [f"fold {f}" for f in range(R - 1)] + ["all rows"]
    capped = [(names[r], a, e) for r in range(R) for a in range(A) for e in range(E) if not infos[r, a, e]["converged"]]
    if capped:
        shown = ", ".join(f"{nm}: {axis} index {a}, eta index {e}" for nm, a, e in capped[:8]) + (", ..." if len(capped) > 8 else "")
        warnings.warn(f"{what} ran into a cap in {len(capped)} of {R * A * E} (row set, cell) pairs ({shown}): their last points "
                      "are returned", ConvergenceWarning)


def l0_local_cv(X, y, *, alphas, etas=(0.0,), cv=5, big_M=100, fit_intercept=False, sample_weight=None, starts=None, max_rounds=2,
                scoring="neg_root_mean_squared_error", solver_options=None) -> L0LocalCV:
    """``l0_local_search`` on every cross-validation fold's training rows and on all rows, one launch per round on the GPU.

    The arguments of ``l0_local_search``, and ``cv`` (anything ``sklearn.model_selection.check_cv`` takes; at most 15 splits)
    and ``scoring`` (``"neg_root_mean_squared_error"`` or ``"neg_mean_squared_error"``, unweighted on the held-out rows).
    ``sample_weight`` weighs the training rows of every problem; ``starts`` are shared by the row sets.  One
    ``ConvergenceWarning`` names the (row set, cell) pairs whose kept result ran into a sweep or swap cap.  The coefficients of
    a fold are not byte for byte those of ``l0_local_search`` on its rows (see the module's text); nothing is proven optimal."""
    swaps, device = _options(solver_options, max_rounds)
    if scoring not in _SCORINGS:
        raise ValueError(f"scoring must be one of {list(_SCORINGS)} (got {scoring!r})")
    spec = _LocalProblem(big_M=big_M, fit_intercept=fit_intercept, solver_options=device)
    # everything is validated before a device is touched
    X, y, dev_options, _, _, _, _, w = spec._l0_setup(X, y, sample_weight)
    al, et = _grid(alphas, "alphas"), _grid(etas, "etas")
    A, E, p = len(al), len(et), X.shape[1]
    if p > _PMAX:
        raise NotImplementedError(f"the l0 local search takes up to {_PMAX} columns (got {p})")
    big_M = float(big_M)
    first, moves = _first_starts(starts, A, E, p, big_M), _round_moves(A, E, max_rounds)
    splits = _fold_splits(cv, X, y, "l0_local_cv")
    R = len(splits) + 1
    most = max(first.shape[2], len(moves))  # (a round starts a cell from its neighbours in the grid)
    if R * A * E * most > _MAX_PROBLEMS:
        raise ValueError(f"{R} row sets x {A * E} cells x up to {most} starts each: more than the {_MAX_PROBLEMS} problems of one launch")
    cell_alpha, cell_eta = np.repeat(al, E), np.tile(et, A)

    def solve(ds, row_weights, n_effs, points):
        return ds.solve_l0_local_folds(row_weights, n_effs, cell_alpha, cell_eta, intercept=fit_intercept, big_M=big_M, starts=points, swaps=swaps)

    def improved(new, old):
        return new < old - _IMPROVE * np.maximum(np.abs(old), al[None, :, None])

    coefs, icpts, objectives, infos, history, counts = _cv_rounds(X, y, splits, w, fit_intercept, dev_options.get("device"), solve, first,
                                                                 moves, max_rounds, improved)
    _warn_capped(infos, "the local search", "alpha")
    take = np.vectorize(lambda d, k: d[k])
    tables = [L0LocalPath(al, et, coefs[r], icpts[r], objectives[r], take(infos[r], "loss").astype(float), len(history), history[:, r],
                          take(infos[r], "swaps").astype(int), take(infos[r], "sweeps").astype(int), take(infos[r], "converged").astype(bool))
              for r in range(R)]
    paths, full = tables[:-1], tables[-1]
    cell_scores = _held_out_scores(scoring, X, y, splits, paths)
    solver_info = {**counts, "winner_max_sweeps": int(max(t.sweeps_.max() for t in tables)),
                   "winner_max_swaps": int(max(t.swaps_.max() for t in tables)), "proven_optimal": False}
    return L0LocalCV(paths, full, splits, cell_scores, scoring, solver_info)
