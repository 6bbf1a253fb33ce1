"""The exact l0 PROFILE: the best support of every size from ONE search (``slm_solve_l0_profile``, csrc/l0_kernels.hpp in its
profile mode).

The value of a support, ``q(S) = min 1/2 beta^T (G + 2 eta W^T W) beta - c^T beta`` inside the ``big_M`` box, depends on
neither ``alpha`` nor ``sparse_bound``.  So the table ``Q_k`` = best ``q`` over admissible supports of exactly k groups --
what classical leaps-and-bounds codes return -- answers, for one ``eta`` / ``tikhonov_w`` / ``big_M`` / hierarchy,

* ``BestSubsetSelection`` / ``RidgedBestSubsetSelection`` for every bound ``K' <= max_groups``: ``min_{k <= K'} Q_k``;
* ``RegularizedL0`` / ``L2L0`` for every ``alpha >= alpha_min``: ``min_k Q_k + alpha k``

(the units of ``_miqp.py``: the reference's objectives divided by ``2n``).  A scan over ``sparse_bound`` or ``alpha`` that
fits one estimator per value walks the same include / exclude tree once per value; ``l0_profile`` walks it once.

With ``alpha_min = 0`` nothing is pruned but what cannot matter to any question, and the search visits about as many nodes
as there are admissible supports of at most ``max_groups`` groups: it is meant for up to ~30 groups, or a small
``max_groups``.  ``alpha_min > 0`` prunes what no ``alpha >= alpha_min`` can use; the table is then no longer the best of
every size and serves ``regularized`` only.  Limits are the estimators': 64 columns and 64 groups -- 128 of each with
``solver_options={"wide": True}``, when ``max_groups <= 64`` and the ``max_groups`` largest groups together hold at most 64
columns (so that every support fits the factor) --, no row-sharded datasets, no ``constraints=``.  ``L1L0`` is not served
HERE: the value of a support there depends on its own l1 weight.  For one fixed l1 weight it depends on nothing else, and
``l1l0_profile`` (``_l1l0_profile.py``) is this table under an l1 term: ``L1L0`` at every ``alpha`` from one search per ``eta``.

Import path: ``sparselm_amd.miqp`` (``l0_profile``, ``L0Profile``); ``sparselm_amd.model`` keeps the names it had.
"""

from __future__ import annotations

import warnings
from numbers import Integral, Real

import numpy as np
from sklearn.exceptions import ConvergenceWarning
from sklearn.utils._param_validation import Interval

from ._miqp import _ExactL0, _TikhonovMixin

__all__ = ["l0_profile", "L0Profile"]

_BIG_M = 100  # the estimators' default (_miqp.py)


class _ProfileProblem(_TikhonovMixin, _ExactL0):
    """The arguments of ``l0_profile`` as an estimator, so that validation, group indexing, hierarchy masks, sample-weight
    normalisation and centring are ``_ExactL0``'s own code.  Not exported, never fitted."""

    _parameter_constraints: dict = {"fit_intercept": ["boolean"], "solver_options": [dict, None]}
    _hyper_parameter_constraints: dict = {
        "max_groups": [Interval(type=Integral, left=0, right=None, closed="left"), None],
        "alpha_min": [Interval(type=Real, left=0.0, right=None, closed="left")],
        "eta": [Interval(type=Real, left=0.0, right=None, closed="left")],
        **_ExactL0._hyper_parameter_constraints,
    }

    def __init__(self, groups=None, max_groups=None, alpha_min=0.0, eta=0.0, tikhonov_w=None, big_M=_BIG_M, hierarchy=None,
                 fit_intercept=False, solver_options=None):
        self.groups = groups
        self.max_groups = max_groups
        self.alpha_min = alpha_min
        self.eta = eta
        self.tikhonov_w = tikhonov_w
        self.big_M = big_M
        self.hierarchy = hierarchy
        self.fit_intercept = fit_intercept
        self.solver_options = solver_options


class L0Profile:
    """The table ``l0_profile`` returns.  With ``K = max_groups`` and p columns:

    ``values_`` (K + 1; ``values_[0] == 0``, ``+inf`` for a size nobody filled -- one the hierarchy admits no support of, or
    one the pruning of ``alpha_min > 0`` never reached), ``supports_`` (K + 1 x n_groups, bool per sorted group label; all
    False on an unfilled row), ``coefs_`` (K + 1 x p), ``intercepts_`` (K + 1), ``alpha_min_``, ``proven_optimal_`` and
    ``solver_info_`` (``nodes``, ``launches``, ``q_all``, ``status``, ``proven_optimal``, ``box_tol``, as the estimators
    report them).  Coefficients are recomputed once per size from the Gram on that support by the code that recomputes an
    estimator's winner, so ``best_subset(K')`` and ``regularized(alpha)`` return the very ``coef_`` of the estimator fitted
    at that value."""

    def __init__(self, values, supports, coefs, intercepts, alpha_min, solver_info):
        self.values_ = values
        self.supports_ = supports
        self.coefs_ = coefs
        self.intercepts_ = intercepts
        self.alpha_min_ = float(alpha_min)
        self.solver_info_ = solver_info
        self.proven_optimal_ = bool(solver_info["proven_optimal"])

    @property
    def max_groups_(self):
        return len(self.values_) - 1

    def _row(self, k):
        return self.coefs_[k].copy(), float(self.intercepts_[k]), self.supports_[k].copy()

    def best_subset_size(self, sparse_bound):
        """The row ``best_subset(sparse_bound)`` reads: ``argmin_{k <= sparse_bound} values_[k]``, ties to the smaller k
        (``l0_profile_best_subset``, csrc/l0_host.hpp)."""
        if self.alpha_min_ > 0.0:
            raise ValueError(f"this table was pruned for regularised use (alpha_min = {self.alpha_min_:g}): its entries need not be the "
                             "best of their size; build it with alpha_min = 0 for best_subset")
        bound = int(np.floor(sparse_bound))
        if bound < 0 or bound > self.max_groups_:
            raise ValueError(f"sparse_bound = {sparse_bound} is outside the table's 0 .. max_groups = {self.max_groups_}")
        return int(np.argmin(self.values_[: bound + 1]))  # (argmin: the first of equal minima)

    def regularized_size(self, alpha):
        """The row ``regularized(alpha)`` reads: ``argmin_k values_[k] + alpha k``, ties to the smaller k
        (``l0_profile_regularized``, csrc/l0_host.hpp)."""
        alpha = float(alpha)
        if not np.isfinite(alpha) or alpha < self.alpha_min_:
            raise ValueError(f"alpha = {alpha:g} is below the table's alpha_min = {self.alpha_min_:g} (or not finite)")
        return int(np.argmin(self.values_ + alpha * np.arange(len(self.values_))))

    def best_subset(self, sparse_bound):
        """``(coef, intercept, active_groups)`` of best subset selection with at most ``sparse_bound`` groups (the row
        ``best_subset_size`` names)."""
        return self._row(self.best_subset_size(sparse_bound))

    def regularized(self, alpha):
        """``(coef, intercept, active_groups)`` of ``RegularizedL0`` / ``L2L0`` at ``alpha >= alpha_min_`` (the row
        ``regularized_size`` names)."""
        return self._row(self.regularized_size(alpha))

    def alpha_breakpoints(self):
        """The exact regularisation path: ``(alphas, sizes)`` with ``alphas`` decreasing and ``len(sizes) == len(alphas) + 1``.
        ``sizes[0]`` is optimal for ``alpha > alphas[0]``, ``sizes[i]`` between ``alphas[i]`` and ``alphas[i - 1]``, ``sizes[-1]``
        below ``alphas[-1]`` -- the vertices of the lower convex envelope of ``values_`` over k, whose slopes are the ``-alpha``
        at which the optimal size changes.  Breakpoints below ``alpha_min_`` are left out (the table does not serve them)."""
        hull = []  # sizes on the envelope, increasing (a monotone-chain lower hull over the finite entries)
        for k in np.flatnonzero(np.isfinite(self.values_)):
            while len(hull) >= 2:
                a, b = hull[-2], hull[-1]
                # b stays only if it lies strictly below the chord from a to k
                if (self.values_[b] - self.values_[a]) * (k - a) < (self.values_[k] - self.values_[a]) * (b - a):
                    break
                hull.pop()
            hull.append(int(k))
        # a size enters only where it lowers the value: the path starts at the empty support and alphas are positive
        sizes, alphas = [hull[0]], []
        for a, b in zip(hull, hull[1:]):
            slope = (self.values_[a] - self.values_[b]) / (b - a)  # the alpha at which sizes a and b tie
            if slope <= 0.0 or slope < self.alpha_min_:
                break
            alphas.append(float(slope))
            sizes.append(b)
        return np.array(alphas), np.array(sizes, dtype=int)


def l0_profile(X, y, *, groups=None, max_groups=None, alpha_min=0.0, eta=0.0, tikhonov_w=None, big_M=_BIG_M, hierarchy=None,
               fit_intercept=False, sample_weight=None, solver_options=None) -> L0Profile:
    """The best support of every size ``0 .. max_groups`` (None: the number of groups) from one search on the GPU.

    ``groups``, ``big_M``, ``hierarchy``, ``fit_intercept``, ``sample_weight`` and ``solver_options`` (``max_nodes``,
    ``device``, ``wide``) are the estimators'; ``eta`` and ``tikhonov_w`` are the ridge term of ``RidgedBestSubsetSelection`` / ``L2L0``
    (``eta = 0``: none).  ``alpha_min``: the smallest ``alpha`` that ``regularized`` will be asked; 0 keeps the full table.
    A ``ConvergenceWarning`` is raised when the node budget ran out: the table then holds the incumbents."""
    spec = _ProfileProblem(groups=groups, max_groups=max_groups, alpha_min=alpha_min, eta=eta, tikhonov_w=tikhonov_w, big_M=big_M,
                           hierarchy=hierarchy, fit_intercept=fit_intercept, solver_options=solver_options)
    # everything is validated before a device is touched
    if isinstance(solver_options, dict) and "bound" in solver_options:
        raise ValueError("l0_profile takes no solver_options['bound']: the profile search prunes against the table of incumbents "
                         "per size, and the exclusion bound is not built into it")
    X, y, options, gidx, n_groups, need, T, w = spec._l0_setup(X, y, sample_weight)
    if not np.isfinite(alpha_min) or not np.isfinite(eta):
        raise ValueError("alpha_min and eta must be finite")
    K = n_groups if max_groups is None else int(max_groups)
    if K > n_groups:
        raise ValueError(f"max_groups = {max_groups} is above the number of groups, {n_groups}")
    wide = bool(options.get("wide")) and (X.shape[1] > 64 or n_groups > 64)  # (within the narrow limits: the narrow search)
    with spec._l0_dataset(X, y, w, gidx, n_groups, need, options) as (ds, x_mean, y_mean, need, max_nodes):
        solve = ds.solve_l0_profile_wide if wide else ds.solve_l0_profile
        coefs, masks, values, info = solve(alpha_min=float(alpha_min), max_groups=K, eta=float(eta), T=T, big_M=float(big_M), need=need, max_nodes=max_nodes)
    if not info["proven_optimal"]:
        warnings.warn(f"the node budget ran out after {info['nodes']} nodes: the table holds the incumbents of every size; raise "
                      "solver_options['max_nodes']", ConvergenceWarning)
    filled = np.isfinite(values)
    supports = np.array([[filled[k] and bool((int(masks[k]) >> i) & 1) for i in range(n_groups)] for k in range(K + 1)], dtype=bool)
    supports = supports.reshape(K + 1, n_groups)
    # (row by row with the estimators' own expression, so that an intercept equals the fitted estimator's to the bit)
    intercepts = np.array([float(y_mean - np.dot(x_mean, coefs[k])) if fit_intercept else 0.0 for k in range(K + 1)])
    return L0Profile(np.asarray(values, dtype=float), supports, np.asarray(coefs, dtype=float), np.asarray(intercepts, dtype=float),
                     alpha_min, info)
