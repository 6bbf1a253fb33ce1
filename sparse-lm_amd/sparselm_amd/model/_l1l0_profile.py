"""The L1L0 PROFILE: ``L1L0`` at every ``alpha`` from ONE search (``slm_solve_l0_l1_profile`` and its wide twin,
csrc/l0_kernels.hpp with its l1 and profile modes together).

``L1L0`` has two hyper-parameters, ``alpha`` (the price of an active group) and ``eta`` (the l1 weight).  For one FIXED
``eta`` the value of a support,

    f(S) = min 1/2 beta^T G beta - c^T beta + eta ||beta||_1      inside the ``big_M`` box, supp beta in cols(S),

depends on neither ``alpha`` nor the size of S.  So the table ``F_k`` = best ``f`` over admissible supports of exactly k
groups answers ``L1L0(alpha, eta)`` for every ``alpha >= alpha_min`` (``min_k F_k + alpha k``): a grid of
``|alphas| x |etas|`` fits becomes ``|etas|`` searches.  With ``alpha_min = 0`` it also answers the cardinality-bounded
lasso for every bound (``best_subset``).

The lasso sets coefficients to zero by itself, so the table SATURATES: from the size that holds every column the lasso on
all columns uses, every larger size ties with it in value, and its support is then the smallest mask among equals, not a
unique answer.  ``regularized`` and ``best_subset`` break ties to the smaller size, so they never read such a row unless
it is the first of its value.

Limits: 64 columns and 64 groups -- 128 of each with ``solver_options={"wide": True}``, when ``max_groups <= 64`` and the
``max_groups`` largest groups together hold at most 64 columns (a support holds at most 64 columns).  This is the way
``L1L0`` reaches more than 64 columns: the estimator itself has no wide mode.  No ridge term, no ``constraints=``, no
``solver_options["bound"]``, no row-sharded datasets.  One call is one row set at one ``eta``; every fold of a
cross-validation at a list of ``eta`` from one launch is ``l1l0_profile_cv`` (``_l0_grid_cv.py``, narrow problems only).

Import path: ``sparselm_amd.miqp`` (``l1l0_profile``, ``L1L0Profile``).
"""

from __future__ import annotations

import warnings
from numbers import Integral, Real

import numpy as np
from sklearn.exceptions import ConvergenceWarning
from sklearn.utils._param_validation import Interval

from ._l0_profile import _BIG_M, L0Profile
from ._miqp import _NARROW, _ExactL0

__all__ = ["l1l0_profile", "L1L0Profile"]


class _L1ProfileProblem(_ExactL0):
    """The arguments of ``l1l0_profile`` as an estimator, so that validation, group indexing, hierarchy masks, sample-weight
    normalisation and centring are ``_ExactL0``'s own code.  Not exported, never fitted."""

    _parameter_constraints: dict = {"fit_intercept": ["boolean"], "solver_options": [dict, None]}
    _hyper_parameter_constraints: dict = {
        "max_groups": [Interval(type=Integral, left=0, right=None, closed="left"), None],
        "alpha_min": [Interval(type=Real, left=0.0, right=None, closed="left")],
        "eta": [Interval(type=Real, left=0.0, right=None, closed="left")],
        **_ExactL0._hyper_parameter_constraints,
    }

    def __init__(self, groups=None, max_groups=None, alpha_min=0.0, eta=0.0, big_M=_BIG_M, hierarchy=None, fit_intercept=False,
                 solver_options=None):
        self.groups = groups
        self.max_groups = max_groups
        self.alpha_min = alpha_min
        self.eta = eta
        self.big_M = big_M
        self.hierarchy = hierarchy
        self.fit_intercept = fit_intercept
        self.solver_options = solver_options


class L1L0Profile(L0Profile):
    """The table ``l1l0_profile`` returns: an ``L0Profile`` whose ``values_[k]`` is the best LASSO value (weight ``eta_``)
    over admissible supports of exactly k groups.  ``regularized(alpha)`` is ``L1L0(alpha=alpha, eta=eta_)``;
    ``best_subset(K')`` is the lasso under at most ``K'`` active groups; ``alpha_breakpoints()`` is the exact path in
    ``alpha`` at this ``eta_``.  ``solver_info_`` also holds ``descents``, and its ``q_all`` is the proven lower bound on the
    value of all columns that the search cut with.  Rows beyond the size at which the lasso on all columns is reached tie in
    value; their supports are the smallest masks among equals."""

    def __init__(self, values, supports, coefs, intercepts, alpha_min, eta, solver_info):
        super().__init__(values, supports, coefs, intercepts, alpha_min, solver_info)
        self.eta_ = float(eta)


def l1l0_profile(X, y, *, eta, groups=None, max_groups=None, alpha_min=0.0, big_M=_BIG_M, hierarchy=None, fit_intercept=False,
                 sample_weight=None, solver_options=None) -> L1L0Profile:
    """The best support of every size ``0 .. max_groups`` (None: the number of groups) under an l1 term, from one search on
    the GPU.

    ``eta`` is the L1 WEIGHT, as in ``L1L0`` -- not the ridge ``eta`` of ``l0_profile``; there is no ridge term here.
    ``groups``, ``big_M``, ``hierarchy``, ``fit_intercept``, ``sample_weight`` and ``solver_options`` (``max_nodes``,
    ``device``, ``wide``) are the estimators'.  ``alpha_min``: the smallest ``alpha`` that ``regularized`` will be asked; 0
    keeps the full table.  ``eta = 0`` is ``l0_profile`` without a ridge term, bit for bit.  A ``ConvergenceWarning`` is
    raised when the node budget ran out: the table then holds the incumbents."""
    spec = _L1ProfileProblem(groups=groups, max_groups=max_groups, alpha_min=alpha_min, eta=eta, big_M=big_M, hierarchy=hierarchy,
                             fit_intercept=fit_intercept, solver_options=solver_options)
    # everything is validated before a device is touched
    if isinstance(solver_options, dict) and "bound" in solver_options:
        raise ValueError("l1l0_profile takes no solver_options['bound']: the exclusion bound bounds the quadratic value, not a "
                         "lasso's, and the profile search prunes against the table of incumbents per size")
    X, y, options, gidx, n_groups, need, _, w = spec._l0_setup(X, y, sample_weight)
    if not np.isfinite(alpha_min) or not np.isfinite(eta):
        raise ValueError("alpha_min and eta must be finite")
    K = n_groups if max_groups is None else int(max_groups)
    if K > n_groups:
        raise ValueError(f"max_groups = {max_groups} is above the number of groups, {n_groups}")
    wide = bool(options.get("wide")) and (X.shape[1] > _NARROW or n_groups > _NARROW)  # (within the narrow limits: the narrow search)
    with spec._l0_dataset(X, y, w, gidx, n_groups, need, options) as (ds, x_mean, y_mean, need, max_nodes):
        solve = ds.solve_l0_l1_profile_wide if wide else ds.solve_l0_l1_profile
        try:
            coefs, masks, values, info = solve(alpha_min=float(alpha_min), max_groups=K, eta_l1=float(eta), big_M=float(big_M), need=need,
                                               max_nodes=max_nodes)
        except NotImplementedError as exc:
            if options.get("wide") or max(X.shape[1], n_groups) <= _NARROW:
                raise
            raise NotImplementedError(f"{exc}; solver_options={{'wide': True}} takes up to 128 of each") from None
    if not info["proven_optimal"]:
        warnings.warn(f"the node budget ran out after {info['nodes']} nodes: the table holds the incumbents of every size; raise "
                      "solver_options['max_nodes']", ConvergenceWarning)
    filled = np.isfinite(values)
    supports = np.array([[filled[k] and bool((int(masks[k]) >> i) & 1) for i in range(n_groups)] for k in range(K + 1)], dtype=bool)
    supports = supports.reshape(K + 1, n_groups)
    # (row by row with the estimators' own expression, so that an intercept equals the fitted estimator's to the bit)
    intercepts = np.array([float(y_mean - np.dot(x_mean, coefs[k])) if fit_intercept else 0.0 for k in range(K + 1)])
    return L1L0Profile(np.asarray(values, dtype=float), supports, np.asarray(coefs, dtype=float), np.asarray(intercepts, dtype=float),
                       alpha_min, eta, info)
