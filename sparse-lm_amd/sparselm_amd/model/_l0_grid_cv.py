"""Cross-validated exact l0 profiles over a grid of ``eta``: every (fold, eta) table and every (all rows, eta) table from ONE
launch (``slm_solve_l0_profile_grid``, csrc/l0_kernels.hpp in its batched profile mode, with or without its l1 mode).

``L1L0(alpha, eta)`` and ``L2L0(alpha, eta)`` are tuned over both weights.  For one ``eta`` a profile answers every
``alpha``; ``l0_profile_cv`` gives the profiles of every fold for one ridge ``eta``.  ``l1l0_profile_cv`` and
``l2l0_profile_cv`` take the whole list ``etas``: ONE dataset (of ``[X | 1]`` when an intercept is fitted), one Gram per row
set, one launch of ``(splits + 1) x len(etas)`` problems, one read-back.  The result holds one ``L0ProfileCV`` per ``eta``
-- built as ``l0_profile_cv`` builds its own, for ``L1L0`` out of ``L1L0Profile`` tables -- and ``search(alphas)`` reads the
two-parameter grid off them in the order of ``ParameterGrid({"alpha": alphas, "eta": etas})``.

Opt-in: ``GridSearchCV`` / ``LineSearchCV`` keep going fit by fit.  Limits: the narrow search's 64 columns and groups, at
most 15 splits, at most 128 problems in all, no ``wide``, no ``bound``, no ``constraints=``, one ``tikhonov_w`` per call, no
ridge term beside the l1 term; held-out scores are unweighted.

Import path: ``sparselm_amd.miqp`` (``l1l0_profile_cv``, ``l2l0_profile_cv``, ``L0ProfileGridCV``).
"""

from __future__ import annotations

import warnings

import numpy as np
from sklearn.exceptions import ConvergenceWarning
from sklearn.model_selection import check_cv

from ._l0_cv import _SCORINGS, _SELECTIONS, MAX_SPLITS, L0ProfileCV, L0ProfileSearch, _score, _supports
from ._l0_profile import _BIG_M, L0Profile, _ProfileProblem
from ._l1l0_profile import L1L0Profile, _L1ProfileProblem

__all__ = ["l1l0_profile_cv", "l2l0_profile_cv", "L0ProfileGridCV"]

MAX_PROBLEMS = 128  # SLM_L0_GRID_MAX: (splits + 1) x len(etas) problems of one launch


class L0ProfileGridCV:
    """What ``l1l0_profile_cv`` / ``l2l0_profile_cv`` return: ``etas_``, ``cvs_`` (one ``L0ProfileCV`` per ``eta``, so
    ``cvs_[e].regularized_search(alphas)`` is the one-parameter search at ``etas_[e]``), ``splits_``, ``scoring_`` and
    ``solver_info_`` (``problems``: one dict per problem in the engine's order -- row sets outermost, the folds then all rows,
    ``etas`` innermost; ``launches``; ``nodes``; ``proven_optimal``)."""

    def __init__(self, etas, cvs, splits, scoring, solver_info):
        self.etas_ = np.asarray(etas, dtype=np.float64)
        self.cvs_ = list(cvs)
        self.splits_ = splits
        self.scoring_ = scoring
        self.solver_info_ = solver_info

    def search(self, alphas, opt_selection_method="max_score"):
        """``L1L0`` / ``L2L0`` over the grid ``alphas x etas_`` (each ``alpha >= alpha_min``): an ``L0ProfileSearch`` whose
        ``cv_results_["params"]`` are ``{"alpha", "eta"}`` dicts in the order of ``ParameterGrid({"alpha": alphas, "eta":
        etas_})`` -- ``alpha`` outermost -- under either selection rule of ``model_selection.py``; the selected model comes
        from the table of all rows at the chosen ``eta``."""
        from ..model_selection import _format_results, select_best_index_onestd

        if opt_selection_method not in _SELECTIONS:
            raise ValueError(f"opt_selection_method must be one of {list(_SELECTIONS)} (got {opt_selection_method!r})")
        alphas = [a.item() if isinstance(a, np.generic) else a for a in list(alphas)]  # (plain numbers in ``params``)
        if not alphas:
            raise ValueError("no alpha to search")
        etas = [float(e) for e in self.etas_]
        # (every value is checked against every table -- the folds' and the ones a model is taken from -- before anything is scored)
        full_sizes = [[cv.full_.regularized_size(a) for cv in self.cvs_] for a in alphas]
        params, scores, rows = [], [], []
        for i, a in enumerate(alphas):
            for e, cv in enumerate(self.cvs_):
                params.append({"alpha": a, "eta": etas[e]})
                scores.append([cv.size_scores_[f, prof.regularized_size(a)] for f, prof in enumerate(cv.profiles_)])
                rows.append((e, full_sizes[i][e]))
        scores = np.array(scores, dtype=float)
        results = _format_results(params, scores, np.zeros_like(scores))
        if opt_selection_method == "one_std_score":
            best = select_best_index_onestd(results)
        else:
            best = int(results["rank_test_score"].argmin())
        e, size = rows[best]
        return L0ProfileSearch(results, best, self.cvs_[e].full_._row(size))


def _check_etas(name, etas):
    try:
        arr = np.asarray(etas, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: etas must be a sequence of numbers") from None
    if arr.size == 0:
        raise ValueError(f"{name}: etas is empty")
    if not np.all(np.isfinite(arr)) or np.any(arr < 0.0):
        raise ValueError(f"{name}: every eta must be finite and >= 0 (got {arr.tolist()})")
    return arr


def _grid_cv(name, spec, l1, X, y, etas, cv, max_groups, alpha_min, big_M, fit_intercept, sample_weight, scoring, solver_options):
    # everything is validated before a device is touched
    if isinstance(solver_options, dict):
        for key in ("wide", "bound"):
            if key in solver_options:
                raise ValueError(f"{name} takes no solver_options[{key!r}]: a batch holds narrow profile searches with the "
                                 "bound on all columns and nothing else")
    if scoring not in _SCORINGS:
        raise ValueError(f"scoring must be one of {list(_SCORINGS)} (got {scoring!r})")
    etas = _check_etas(name, etas)
    X, y, options, gidx, n_groups, need, T, w = spec._l0_setup(X, y, sample_weight)
    if not np.isfinite(alpha_min):
        raise ValueError("alpha_min must be finite")
    K = n_groups if max_groups is None else int(max_groups)
    if K > n_groups:
        raise ValueError(f"max_groups = {max_groups} is above the number of groups, {n_groups}")
    splitter = check_cv(cv, y, classifier=False)
    n_splits = int(splitter.get_n_splits(X, y))
    if not 1 <= n_splits <= MAX_SPLITS:
        raise ValueError(f"{name} takes 1 .. {MAX_SPLITS} splits (got {n_splits}): the folds and all rows are at most "
                         f"{MAX_SPLITS + 1} row sets of one launch")
    if (n_splits + 1) * len(etas) > MAX_PROBLEMS:
        raise ValueError(f"{name} takes at most {MAX_PROBLEMS} problems in one launch (got ({n_splits} splits + 1) x {len(etas)} etas = "
                         f"{(n_splits + 1) * len(etas)}): split the list of etas")
    splits = [(np.asarray(tr), np.asarray(te)) for tr, te in splitter.split(X, y)]
    n = X.shape[0]
    base = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    row_weights, n_effs = [], []
    for rows in [tr for tr, _ in splits] + [np.arange(n)]:  # the folds' training rows, then all rows
        m = np.zeros(n)
        m[rows] = base[rows]
        total = float(m.sum())
        if not total > 0.0:
            raise ValueError("a training set has no weight")
        row_weights.append(m * (len(rows) / total))
        n_effs.append(len(rows))

    from .. import _engine

    eng = _engine.get_engine(options.get("device"))
    Xd = np.hstack([X, np.ones((n, 1))]) if fit_intercept else X
    # (the ones column: a group of its own behind the others; single columns stay single columns)
    gd = np.append(gidx, n_groups) if fit_intercept and gidx is not None else gidx
    with eng.dataset(Xd, y) as ds:
        ds.set_groups(gd, n_groups + (1 if fit_intercept else 0))
        if need is not None and n_groups > 64:
            need = None  # (the engine refuses the size itself; masks of more than 64 groups have no 64-bit form)
        coefs, icpts, masks, values, infos = ds.solve_l0_profile_grid(
            row_weights, n_effs, etas, eta_kind=1 if l1 else 0, intercept=fit_intercept, alpha_min=float(alpha_min), max_groups=K, T=T,
            big_M=float(big_M), need=need, max_nodes=int(options.get("max_nodes", 0) or 0))
    n_eta, n_sets = len(etas), len(splits) + 1
    set_names = [f"fold {f}" for f in range(len(splits))] + ["all rows"]
    starved = [f"{set_names[b // n_eta]} at eta = {etas[b % n_eta]:g}" for b, info in enumerate(infos) if not info["proven_optimal"]]
    if starved:
        warnings.warn(f"the node budget ran out in {len(starved)} of {len(infos)} problems ({', '.join(starved)}): their tables hold "
                      "the incumbents of every size; raise solver_options['max_nodes']", ConvergenceWarning)

    def table(b, eta):
        parts = (np.asarray(values[b], dtype=float), _supports(masks[b], values[b], n_groups), np.asarray(coefs[b], dtype=float),
                 np.asarray(icpts[b], dtype=float), alpha_min)
        return L1L0Profile(*parts, eta, infos[b]) if l1 else L0Profile(*parts, infos[b])

    cvs = []
    for e, eta in enumerate(etas):
        tables = [table(r * n_eta + e, float(eta)) for r in range(n_sets)]
        profiles, full = tables[:-1], tables[-1]
        size_scores = np.full((len(splits), K + 1), np.nan)
        for f, (_, te) in enumerate(splits):
            for k in np.flatnonzero(np.isfinite(profiles[f].values_)):
                size_scores[f, k] = _score(scoring, y[te] - (X[te] @ profiles[f].coefs_[k] + profiles[f].intercepts_[k]))
        own = [infos[r * n_eta + e] for r in range(n_sets)]
        info_e = {"problems": own, "launches": max(int(i["launches"]) for i in own),
                  "proven_optimal": all(i["proven_optimal"] for i in own), "nodes": int(sum(i["nodes"] for i in own))}
        cvs.append(L0ProfileCV(profiles, full, splits, size_scores, scoring, info_e))
    solver_info = {"problems": list(infos), "launches": max(int(info["launches"]) for info in infos),
                   "proven_optimal": not starved, "nodes": int(sum(info["nodes"] for info in infos))}
    return L0ProfileGridCV(etas, cvs, splits, scoring, solver_info)


def l1l0_profile_cv(X, y, *, etas, cv=5, groups=None, max_groups=None, alpha_min=0.0, big_M=_BIG_M, hierarchy=None,
                    fit_intercept=False, sample_weight=None, scoring="neg_root_mean_squared_error", solver_options=None) -> L0ProfileGridCV:
    """The ``L1L0`` profile (``l1l0_profile``) of every cross-validation fold's training rows and of all rows at every l1
    weight of ``etas``, from one launch on the GPU.

    The arguments of ``l1l0_profile`` with the list ``etas`` for its ``eta``, and ``cv`` / ``scoring`` / ``sample_weight`` as
    ``l0_profile_cv`` takes them.  At most 15 splits and ``(splits + 1) x len(etas) <= 128`` problems.  ``solver_options``:
    ``max_nodes`` (each problem's budget) and ``device``.  One ``ConvergenceWarning`` names the problems whose budget ran out."""
    spec = _L1ProfileProblem(groups=groups, max_groups=max_groups, alpha_min=alpha_min, eta=0.0, big_M=big_M, hierarchy=hierarchy,
                             fit_intercept=fit_intercept, solver_options=solver_options)
    return _grid_cv("l1l0_profile_cv", spec, True, X, y, etas, cv, max_groups, alpha_min, big_M, fit_intercept, sample_weight, scoring,
                    solver_options)


def l2l0_profile_cv(X, y, *, etas, cv=5, groups=None, max_groups=None, alpha_min=0.0, tikhonov_w=None, big_M=_BIG_M, hierarchy=None,
                    fit_intercept=False, sample_weight=None, scoring="neg_root_mean_squared_error", solver_options=None) -> L0ProfileGridCV:
    """The ``L2L0`` profile (``l0_profile`` with a ridge term) of every cross-validation fold's training rows and of all rows
    at every ridge weight of ``etas``, from one launch on the GPU: ``l0_profile_cv(eta=etas[e])`` for every ``e`` at once,
    table for table.  One ``tikhonov_w`` serves all of them.  Limits and ``solver_options`` as for ``l1l0_profile_cv``."""
    spec = _ProfileProblem(groups=groups, max_groups=max_groups, alpha_min=alpha_min, eta=0.0, tikhonov_w=tikhonov_w, big_M=big_M,
                           hierarchy=hierarchy, fit_intercept=fit_intercept, solver_options=solver_options)
    return _grid_cv("l2l0_profile_cv", spec, False, X, y, etas, cv, max_groups, alpha_min, big_M, fit_intercept, sample_weight, scoring,
                    solver_options)
