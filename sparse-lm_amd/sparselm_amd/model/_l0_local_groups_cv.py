"""The grouped l0 local search, cross-validated: every fold's (alpha, eta) grid and the grid of all rows from ONE launch per
round (``slm_solve_l0_local_groups`` on up to 16 row sets, csrc/l0_local_group_kernels.hpp).

``l0_local_group_search`` (``model/_l0_local_groups.py``) on every fold's training rows and on all rows, exactly as ``l0_local_cv``
does it for ``l0_local_search``: ONE dataset (of ``[X | 1]`` with an intercept -- the ones column, alone in a last group of its own,
is eliminated per row set), the folds' training masks and the all-rows set in one call per round, every cell of every fold scored
on its held-out rows with numpy; ``L0LocalGroupCV.search`` reads the grid ``{alpha, eta}`` off the scores under both selection
rules of ``model_selection.py``.  A whole cross-validation is 1 + rounds launches, whatever the number of folds.

Limits and caveats are the two parents': 1024 columns, at most 15 splits, ``(splits + 1) x cells x starts <= 8192`` problems per
launch, unweighted held-out scores; nothing is proven optimal and the group descent's screen is a heuristic.  Out of scope: groups
in the cardinality form, an l1 term, a Tikhonov matrix, constraints, seeding the exact search.

Import path: ``sparselm_amd.miqp`` (``l0_local_group_cv``, ``L0LocalGroupCV``).
"""

from __future__ import annotations

import numpy as np

from ._l0_cv import _SCORINGS
from ._l0_local import _IMPROVE, _MAX_PROBLEMS
from ._l0_local_cv import L0LocalCV, _cv_rounds, _fold_splits, _held_out_scores, _warn_capped
from ._l0_local_groups import _WHAT, L0LocalGroupPath, _GroupPlan

__all__ = ["l0_local_group_cv", "L0LocalGroupCV"]


class L0LocalGroupCV(L0LocalCV):
    """What ``l0_local_group_cv`` returns: ``L0LocalCV``'s attributes with ``L0LocalGroupPath`` tables (``paths_`` per fold, ``full_`` of
    all rows: ``group_supports_``, ``n_active_groups_`` and ``trials_`` beside the coefficients).  ``search()`` is ``L0LocalCV``'s, over
    ``{alpha, eta}``."""


def l0_local_group_cv(X, y, *, alphas, groups=None, hierarchy=None, etas=(0.0,), cv=5, big_M=100, fit_intercept=False, sample_weight=None,
                      starts=None, max_rounds=2, scoring="neg_root_mean_squared_error", solver_options=None) -> L0LocalGroupCV:
    """``l0_local_group_search`` on every cross-validation fold's training rows and on all rows, one launch per round on the GPU.

    The arguments of ``l0_local_group_search``, and ``cv`` / ``scoring`` as for ``l0_local_cv``.  One ``ConvergenceWarning`` names
    the (row set, cell) pairs whose kept result ran into a cap.  A fold's coefficients are not byte for byte those of
    ``l0_local_group_search`` on its rows (the Gram of a fold is built from a row mask, centring is by elimination); supports and
    objectives agree where no decision of the rule is close to a tie.  Nothing is proven optimal."""
    if scoring not in _SCORINGS:
        raise ValueError(f"scoring must be one of {list(_SCORINGS)} (got {scoring!r})")
    # everything is validated before a device is touched
    plan = _GroupPlan(X, y, alphas, groups, hierarchy, etas, big_M, fit_intercept, sample_weight, starts, max_rounds, solver_options)
    A, E, al = plan.A, plan.E, plan.al
    splits = _fold_splits(cv, plan.X, plan.y, "l0_local_group_cv")
    R = len(splits) + 1
    if R * A * E * plan.most > _MAX_PROBLEMS:
        raise ValueError(f"{R} row sets x {A * E} cells x up to {plan.most} starts each: more than the {_MAX_PROBLEMS} problems of one launch")
    # (with an intercept the ones column is last, alone in one more group)
    gidx = plan.gidx if plan.gidx is None or not fit_intercept else np.append(plan.gidx, plan.n_groups).astype(np.int32)
    n_groups = plan.n_groups + (1 if fit_intercept else 0)

    def solve(ds, row_weights, n_effs, points):
        if gidx is not None:
            ds.set_groups(gidx, n_groups)  # (setting the same groups again is free; None: the dataset's singleton groups)
        b, i, o, wn, _, stats, info = ds.solve_l0_local_groups(row_weights, n_effs, plan.cell_alpha, plan.cell_eta, need=plan.need,
                                                               intercept=fit_intercept, big_M=plan.big_M, starts=points, swaps=plan.swaps)
        return b, i, o, wn, stats, info

    def improved(new, old):
        return new < old - _IMPROVE * np.maximum(np.abs(old), al[None, :, None])

    coefs, icpts, objectives, infos, history, counts = _cv_rounds(plan.X, plan.y, splits, plan.w, fit_intercept, plan.dev_options.get("device"),
                                                                 solve, plan.first, plan.moves, max_rounds, improved)
    _warn_capped(infos, _WHAT, "alpha")
    take = np.vectorize(lambda d, k: d[k])
    tables = [L0LocalGroupPath(al, plan.et, plan.unpermute(coefs[r]), icpts[r], objectives[r], take(infos[r], "loss").astype(float), len(history),
                               history[:, r], take(infos[r], "swaps").astype(int), take(infos[r], "sweeps").astype(int),
                               take(infos[r], "converged").astype(bool), group_supports=plan.group_supports(coefs[r]),
                               trials=take(infos[r], "trials").astype(int))
              for r in range(R)]
    paths, full = tables[:-1], tables[-1]
    # (the held-out scores read the ORIGINAL column order: the tables' coefficients are mapped back)
    Xo = np.empty_like(plan.X)
    Xo[:, plan.perm] = plan.X
    cell_scores = _held_out_scores(scoring, Xo, plan.y, splits, paths)
    solver_info = {**counts, "winner_max_sweeps": int(max(t.sweeps_.max() for t in tables)),
                   "winner_max_swaps": int(max(t.swaps_.max() for t in tables)), "proven_optimal": False}
    return L0LocalGroupCV(paths, full, splits, cell_scores, scoring, solver_info)
