"""The l0 local search with an l1 term, cross-validated: every fold's (alpha, eta) grid and the grid of all rows from ONE launch
per round (``slm_solve_l0_local_l1`` on up to 16 row sets, csrc/l0_local_kernels.hpp).

``l1l0_local_search`` (``model/_l1l0_local.py``) on every fold's training rows and on all rows, exactly as ``l0_local_cv`` does it for
``l0_local_search``: ONE dataset (of ``[X | 1]`` with an intercept -- the engine eliminates that column per row set), the folds'
training masks and the all-rows set in one call per round, every cell of every fold scored on its held-out rows with numpy;
``L1L0LocalCV.search`` reads the grid ``{alpha, eta}`` -- ``eta`` the L1 WEIGHT, as in ``L1L0`` -- off the scores under both selection
rules of ``model_selection.py``.  A whole cross-validation is 1 + rounds launches, whatever the number of folds.

NOTHING IS PROVEN: every model is a local minimum.  Limits are the two parents': 1024 columns, at most 15 splits,
``(splits + 1) x cells x starts <= 8192`` problems per launch, unweighted held-out scores.  A fold's coefficients are not byte for
byte those of ``l1l0_local_search`` on its rows (the Gram of a fold is built from a row mask, centring is by elimination); supports
and objectives agree where no decision of the rule is close to a tie.  Out of scope: groups or a hierarchy with the l1 term, the
cardinality form with it, a Tikhonov matrix, constraints, rerouting ``GridSearchCV``, more than 16 row sets.

Import path: ``sparselm_amd.miqp`` (``l1l0_local_cv``, ``L1L0LocalCV``).
"""

from __future__ import annotations

import numpy as np

from ._l0_cv import _SCORINGS
from ._l0_local import _IMPROVE, _MAX_PROBLEMS
from ._l0_local_cv import L0LocalCV, _cv_rounds, _fold_splits, _held_out_scores, _warn_capped
from ._l1l0_local import _WHAT, L1L0LocalPath, _L1Plan

__all__ = ["l1l0_local_cv", "L1L0LocalCV"]


class L1L0LocalCV(L0LocalCV):
    """What ``l1l0_local_cv`` returns: ``L0LocalCV``'s attributes with ``L1L0LocalPath`` tables (``paths_`` per fold, ``full_`` of all
    rows); ``etas_`` are the l1 weights.  ``search()`` is ``L0LocalCV``'s, over ``{alpha, eta}``."""


def l1l0_local_cv(X, y, *, alphas, etas, ridge=0.0, cv=5, big_M=100, fit_intercept=False, sample_weight=None, starts=None, max_rounds=2,
                  scoring="neg_root_mean_squared_error", solver_options=None) -> L1L0LocalCV:
    """``l1l0_local_search`` on every cross-validation fold's training rows and on all rows, one launch per round on the GPU.

    The arguments of ``l1l0_local_search``, and ``cv`` / ``scoring`` as for ``l0_local_cv``.  One ``ConvergenceWarning`` names the
    (row set, cell) pairs whose kept result ran into a cap.  Nothing is proven optimal."""
    if scoring not in _SCORINGS:
        raise ValueError(f"scoring must be one of {list(_SCORINGS)} (got {scoring!r})")
    # everything is validated before a device is touched
    plan = _L1Plan(X, y, alphas, etas, ridge, big_M, fit_intercept, sample_weight, starts, max_rounds, solver_options)
    A, E, al = plan.A, plan.E, plan.al
    splits = _fold_splits(cv, plan.X, plan.y, "l1l0_local_cv")
    R = len(splits) + 1
    if R * A * E * plan.most > _MAX_PROBLEMS:
        raise ValueError(f"{R} row sets x {A * E} cells x up to {plan.most} starts each: more than the {_MAX_PROBLEMS} problems of one launch")

    def solve(ds, row_weights, n_effs, points):
        return ds.solve_l0_local_l1(row_weights, n_effs, plan.cell_alpha, plan.cell_l1, plan.cell_ridge, intercept=fit_intercept,
                                    big_M=plan.big_M, starts=points, swaps=plan.swaps)

    def improved(new, old):
        return new < old - _IMPROVE * np.maximum(np.abs(old), al[None, :, None])

    coefs, icpts, objectives, infos, history, counts = _cv_rounds(plan.X, plan.y, splits, plan.w, fit_intercept, plan.dev_options.get("device"),
                                                                 solve, plan.first, plan.moves, max_rounds, improved)
    _warn_capped(infos, _WHAT, "alpha")
    take = np.vectorize(lambda d, k: d[k])
    tables = [L1L0LocalPath(al, plan.et, coefs[r], icpts[r], objectives[r], take(infos[r], "loss").astype(float), len(history), history[:, r],
                            take(infos[r], "swaps").astype(int), take(infos[r], "sweeps").astype(int),
                            take(infos[r], "converged").astype(bool), ridge=plan.ridge)
              for r in range(R)]
    paths, full = tables[:-1], tables[-1]
    cell_scores = _held_out_scores(scoring, plan.X, plan.y, splits, paths)
    solver_info = {**counts, "winner_max_sweeps": int(max(t.sweeps_.max() for t in tables)),
                   "winner_max_swaps": int(max(t.swaps_.max() for t in tables)), "proven_optimal": False}
    return L1L0LocalCV(paths, full, splits, cell_scores, scoring, solver_info)
