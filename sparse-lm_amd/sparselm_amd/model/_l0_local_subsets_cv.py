"""Local subsets, cross-validated: every fold's (size, eta) grid and the grid of all rows from ONE launch per round
(``slm_solve_l0_local_subsets``, csrc/l0_local_kernels.hpp).

``l0_local_subsets`` returns an incumbent for every size and says nothing about which size to use.  ``l0_local_subsets_cv``
asks the same grid of every fold's training rows and of all rows as ``l0_local_cv`` does for the penalised form: ONE dataset
(of ``[X | 1]`` when an intercept is fitted; the engine eliminates that column per row set), the folds' training weights and
the all-rows set in one call per round, each row set's cells restarted from THAT row set's neighbours' winners, and every cell
of every fold scored on its held-out rows with numpy.  A whole cross-validation is 1 + rounds launches, whatever the number of
folds.  ``L0LocalSubsetsCV.search`` reads the grid off the scores: scikit-learn-shaped ``cv_results_`` over
``{"sparse_bound", "eta"}``, the selection rules of ``model_selection.py``, and the selected model from the grid of all rows.

Against ``l0_local_subsets`` on a fold's rows alone the supports agree and the objectives agree to 1e-10 where no decision of
the rule is closer than that to a tie; the coefficients are not the same bytes (a fold's Gram is built from the complement of
its held-out rows, and centring is by elimination of the ones column).  Nothing is proven optimal.

Limits: 1024 columns, at most 15 splits, ``(splits + 1) x cells x starts <= 8192`` problems per launch; held-out scores are
unweighted.  Not built: groups, an l1 term, rerouting ``GridSearchCV``.  (Groups and a hierarchy in the penalised form:
``l0_local_group_cv``.)

Import path: ``sparselm_amd.miqp`` (``l0_local_subsets_cv``, ``L0LocalSubsetsCV``).
"""

from __future__ import annotations

import numpy as np

from ._l0_cv import _SCORINGS, _SELECTIONS
from ._l0_local import _LocalProblem, _options
from ._l0_local_cv import L0LocalSearch, _cv_rounds, _fold_splits, _held_out_scores, _warn_capped
from ._l0_local_subsets import L0LocalSubsets, _improved, _subsets_grid

__all__ = ["l0_local_subsets_cv", "L0LocalSubsetsCV"]


class L0LocalSubsetsCV:
    """What ``l0_local_subsets_cv`` returns: ``paths_`` (one ``L0LocalSubsets`` per fold, on its training rows), ``full_`` (the
    ``L0LocalSubsets`` of all rows), ``splits_`` (``(train, test)`` index pairs), ``cell_scores_`` (folds x K x E: the
    unweighted held-out score of each cell's fit), ``sizes_``, ``etas_``, ``scoring_``, ``solver_info_`` (``launches``;
    ``rounds``; ``problems``: the problems of one launch at most; ``max_sweeps`` and ``max_swaps``: the largest counts of ANY
    problem of the call; ``proven_optimal``: False) and ``proven_optimal_ = False``."""

    proven_optimal_ = False

    def __init__(self, paths, full, splits, cell_scores, scoring, solver_info):
        self.paths_ = paths
        self.full_ = full
        self.splits_ = splits
        self.cell_scores_ = cell_scores
        self.sizes_, self.etas_ = full.sizes_, full.etas_
        self.scoring_ = scoring
        self.solver_info_ = solver_info

    def search(self, opt_selection_method="max_score"):
        """The grid ``sizes_ x etas_`` read off ``cell_scores_``: an ``L0LocalSearch`` whose ``cv_results_["params"]`` are
        ``{"sparse_bound", "eta"}`` dicts in the order of ``ParameterGrid({"sparse_bound": sizes_, "eta": etas_})`` --
        ``eta`` outermost, as ``ParameterGrid`` sorts the names -- under either selection rule of ``model_selection.py``; the
        selected model is ``full_``'s at the chosen cell."""
        from ..model_selection import _format_results, select_best_index_onestd

        if opt_selection_method not in _SELECTIONS:
            raise ValueError(f"opt_selection_method must be one of {list(_SELECTIONS)} (got {opt_selection_method!r})")
        K, E = len(self.sizes_), len(self.etas_)
        params = [{"eta": float(e), "sparse_bound": int(k)} for e in self.etas_ for k in self.sizes_]
        scores = np.asarray(self.cell_scores_, dtype=float).transpose(0, 2, 1).reshape(len(self.paths_), E * K).T
        results = _format_results(params, scores, np.zeros_like(scores))
        if opt_selection_method == "one_std_score":
            best = select_best_index_onestd(results)
        else:
            best = int(results["rank_test_score"].argmin())
        e, k = divmod(int(best), K)
        return L0LocalSearch(results, best, self.full_.coefs_[k, e].copy(), float(self.full_.intercepts_[k, e]))


def l0_local_subsets_cv(X, y, *, sizes, etas=(0.0,), cv=5, big_M=100, fit_intercept=False, sample_weight=None, starts=None, max_rounds=2,
                        scoring="neg_root_mean_squared_error", solver_options=None) -> L0LocalSubsetsCV:
    """``l0_local_subsets`` on every cross-validation fold's training rows and on all rows, one launch per round on the GPU.

    The arguments of ``l0_local_subsets``, and ``cv`` (anything ``sklearn.model_selection.check_cv`` takes; at most 15 splits)
    and ``scoring`` (``"neg_root_mean_squared_error"`` or ``"neg_mean_squared_error"``, unweighted on the held-out rows).
    ``sample_weight`` weighs the training rows of every problem; ``starts`` are shared by the row sets.  One
    ``ConvergenceWarning`` names the (row set, cell) pairs whose kept result ran into a sweep or swap cap.  Nothing is proven
    optimal."""
    # everything is validated before a device is touched
    swaps, device = _options(solver_options, max_rounds, "local subsets")
    if scoring not in _SCORINGS:
        raise ValueError(f"scoring must be one of {list(_SCORINGS)} (got {scoring!r})")
    spec = _LocalProblem(big_M=big_M, fit_intercept=fit_intercept, solver_options=device)
    X, y, dev_options, _, _, _, _, w = spec._l0_setup(X, y, sample_weight)
    splits = _fold_splits(cv, X, y, "l0_local_subsets_cv")
    R = len(splits) + 1
    ks, et, first, moves = _subsets_grid(sizes, etas, big_M, starts, max_rounds, X.shape[1], row_sets=R)
    K, E = len(ks), len(et)
    big_M = float(big_M)
    cell_size, cell_eta = np.repeat(ks, E), np.tile(et, K)

    def solve(ds, row_weights, n_effs, points):
        return ds.solve_l0_local_subsets(row_weights, n_effs, cell_size, cell_eta, intercept=fit_intercept, big_M=big_M, starts=points, swaps=swaps)

    coefs, icpts, objectives, infos, history, counts = _cv_rounds(X, y, splits, w, fit_intercept, dev_options.get("device"), solve, first,
                                                                 moves, max_rounds, _improved)
    _warn_capped(infos, "local subsets", "size")
    take = np.vectorize(lambda d, k: d[k])
    tables = [L0LocalSubsets(ks, et, coefs[r], icpts[r], objectives[r], take(infos[r], "loss").astype(float), len(history), history[:, r],
                             take(infos[r], "swaps").astype(int), take(infos[r], "sweeps").astype(int), take(infos[r], "grows").astype(int),
                             take(infos[r], "drops").astype(int), take(infos[r], "converged").astype(bool))
              for r in range(R)]
    paths, full = tables[:-1], tables[-1]
    cell_scores = _held_out_scores(scoring, X, y, splits, paths)
    solver_info = {**counts, "proven_optimal": False}
    return L0LocalSubsetsCV(paths, full, splits, cell_scores, scoring, solver_info)
