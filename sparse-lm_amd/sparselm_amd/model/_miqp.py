"""Exact l0 estimators under the reference's names: ``BestSubsetSelection``, ``RidgedBestSubsetSelection``,
``RegularizedL0`` and ``L2L0`` (reference src/sparselm/model/_miqp/_best_subset.py:95-124, 215-248 and
_regularized_l0.py:115-144, 502-530 for the constructors and parameter constraints).

The reference writes these as mixed-integer quadratic programs in cvxpy and needs Gurobi or SCIP to solve them.  Here one
launch of a depth-first search over supports on the GPU (``slm_solve_l0``, csrc/l0_kernels.hpp) returns the proven optimum
for up to 64 columns and 64 groups -- with ``solver_options={"wide": True}`` up to 128 of each (``slm_solve_l0_wide``), where a
support may hold at most 64 independent columns.  The reference's objectives divided by ``2n`` (_miqp/_base.py:126-127,
_regularized_l0.py:157-161, ``TikhonovMixin`` _base.py:544-546) are all

    minimise over supports S (sets of GROUPS) and beta, supp beta in cols(S), |beta_j| <= big_M:
        1/2 beta^T (G + 2 eta W^T W) beta - c^T beta + alpha |S|,      G = X^T X / n,  c = X^T y / n
    subject to |S| <= sparse_bound  and  i in S => hierarchy[i] in S

with ``alpha = 0`` for the two best-subset classes (the reference's missing ``1/(2n)`` there does not move the minimiser),
``sparse_bound =`` the number of groups for the two regularised ones, and ``eta = 0`` without a ridge term.

The fifth, ``L1L0`` (an l1 term beside the l0 one: a lasso per support), is served by the same search in its l1 mode
(``slm_solve_l0_l1``); it lives in ``_l1l0.py`` and its import path is ``sparselm_amd.miqp.L1L0`` -- this module's ``__all__``
and ``sparselm_amd.model`` keep the four names above.

``add_constraints`` (``scipy.optimize.LinearConstraint`` / ``Bounds`` objects, as on the Lasso family; the reference's method
of that name, examples/plot_chull.py:157-183 -- there is no ``constraints=`` constructor argument, the constructors stay
the reference's) adds ``lo <= A beta <= hi`` to the problem of the four classes here:
the search then runs in its constrained mode (``slm_solve_l0_constrained``), in which a support's value is a quadratic
programme valued on chip and bounded from below by a dual value (DESIGN 4d "Constrained mode").  A ``Bounds`` interval that
contains 0 narrows the ``big_M`` box of its column; one that excludes 0 forces the column active and becomes a row ``e_j``
of ``A``.  The mode takes up to 64 rows and needs ``G + 2 eta W^T W`` positive definite (``eta > 0``, or a design of full
column rank).  Refused: ``L1L0`` with constraints, constraints with ``wide``, more than 64 rows.  ``l0_profile`` has no
constraints.

``sparselm_amd.miqp.l0_profile`` (``_l0_profile.py``) answers a whole scan over ``sparse_bound`` or ``alpha`` of the four
classes here from one search; it shares ``_ExactL0._l0_setup`` and ``_ExactL0._l0_dataset`` with ``fit``.
"""

from __future__ import annotations

import contextlib
import warnings
from numbers import Real

import numpy as np
from sklearn.base import BaseEstimator, RegressorMixin, _clone_parametrized
from sklearn.exceptions import ConvergenceWarning
from sklearn.utils._param_validation import Interval, validate_parameter_constraints
from sklearn.utils.validation import _check_sample_weight, check_is_fitted, validate_data

from .._utils.validation import check_groups, dense_group_index
from ._constrained import _as_list, check_feasible, stack_constraints

__all__ = ["BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L2L0"]

_KNOWN_OPTIONS = {"max_nodes", "device", "wide", "max_qp_sweeps", "bound"}
_BOUNDS = ("q_all", "exclusion")  # solver_options["bound"]: the plain subtree bound (the default), or the exclusion bound
_NARROW = 64  # L0_PMAX: columns and groups of the narrow search, independent columns of a support in the wide one


def _hierarchy_masks(hierarchy, groups, n_features):
    """``need[i]``: the dense indices (as one integer mask) of the groups the i-th sorted label depends on -- entry i of
    ``hierarchy`` lists LABELS (reference _miqp/_base.py:160-166).  ValueError for a wrong length or an unknown label."""
    labels = np.arange(n_features) if groups is None else np.unique(np.asarray(groups))
    if hierarchy is None:
        return None
    if len(hierarchy) != len(labels):
        raise ValueError(f"hierarchy must have one entry per group: {len(hierarchy)} != {len(labels)}")
    index = {lab.item() if hasattr(lab, "item") else lab: i for i, lab in enumerate(labels)}
    need = []
    for i, subs in enumerate(hierarchy):
        mask = 0
        for lab in subs:
            key = lab.item() if hasattr(lab, "item") else lab
            if key not in index:
                raise ValueError(f"hierarchy[{i}] names {lab!r}, which is not a group label")
            mask |= 1 << index[key]
        need.append(mask)
    return need


def _hierarchy_lists(hierarchy, groups, n_features):
    """``_hierarchy_masks`` in list form, for more groups than a mask has bits (the grouped local search, up to 1024):
    ``need[i]`` is the sorted dense indices of the groups the i-th sorted label depends on.  The same two ``ValueError``s."""
    masks = _hierarchy_masks(hierarchy, groups, n_features)
    if masks is None:
        return None
    return [[g for g in range(len(masks)) if (mask >> g) & 1] for mask in masks]


class _FoldedConstraints:
    """``constraints`` as the constrained search takes them: the rows ``lo <= A b <= hi`` and the per-column box.

    Every object is stacked by ``stack_constraints`` (``self.cs``: validation, the feasibility check, ``split``).  A stacked
    row that comes from a ``Bounds`` entry whose interval contains 0 is FOLDED into the box of its column
    (``box_lo`` / ``box_hi``); every other stacked row -- ``LinearConstraint`` rows, and ``Bounds`` entries that exclude 0
    (the column is forced active) -- is a row of ``A``.  ``route[r]``: ``("row", i)`` the i-th row of ``A``, or
    ``("box", j, lb, ub)``."""

    def __init__(self, constraints, n_features):
        from scipy.optimize import Bounds

        p = int(n_features)
        self.cs = cs = stack_constraints(constraints, p)
        self.box_lo, self.box_hi = np.full(p, -np.inf), np.full(p, np.inf)
        self.route, rows, r = [], [], 0
        for obj, kept in zip(_as_list(constraints), cs.kept):
            for j in kept:
                lb, ub = cs.lo[r], cs.hi[r]
                if isinstance(obj, Bounds) and lb <= 0.0 <= ub:
                    self.box_lo[j], self.box_hi[j] = max(self.box_lo[j], lb), min(self.box_hi[j], ub)
                    self.route.append(("box", int(j), float(lb), float(ub)))
                else:
                    self.route.append(("row", len(rows)))
                    rows.append(r)
                r += 1
        self.A = np.ascontiguousarray(cs.A[rows]).reshape(len(rows), p)
        self.lo, self.hi = cs.lo[rows].copy(), cs.hi[rows].copy()

    def split(self, lam_rows, coef, mu, active_cols):
        """One array of multipliers per constraint object: the engine's for the rows of ``A``; for a folded ``Bounds`` entry
        the box multiplier ``mu_j`` where the coefficient of an active column sits at that entry's own bound
        (> 0: ``ub`` binds, < 0: ``lb`` binds)."""
        lam = np.zeros(self.cs.m)
        for r, how in enumerate(self.route):
            if how[0] == "row":
                lam[r] = lam_rows[how[1]]
            else:
                _, j, lb, ub = how
                if active_cols[j] and ((coef[j] == ub and mu[j] > 0.0) or (coef[j] == lb and mu[j] < 0.0)):
                    lam[r] = mu[j]
        return self.cs.split(lam)


class _ExactL0(RegressorMixin, BaseEstimator):
    """Common part of the four estimators (the reference's ``MIQPl0``, _miqp/_base.py:22-167).

    Fitted attributes: ``coef_``, ``intercept_``, ``active_groups_`` (bool per sorted group label: the counterpart of the
    reference's ``canonicals_.auxiliaries.z0.value``) and ``solver_info_`` with ``objective`` (in the units above),
    ``lower_bound`` (proven; equal to the objective when the search finished), ``proven_optimal``, ``nodes`` (group
    inclusions tried: it may differ between two fits of one problem, because pruning depends on when the wavefronts see
    each other's incumbents -- the result does not), ``status``, ``loss``, ``seed_objective``, ``launches``, ``box_tol``
    (supports that leave the ``big_M`` box are compared by a coordinate descent stopped at this relative change per sweep).
    A column that depends on the other active columns keeps a zero coefficient: an inactive group is all zero, an active
    group need not be all non-zero (a group {a, 2a}, a centred one-hot group).

    ``solver`` is accepted for the reference's signature and ignored; ``ignore_psd_check`` likewise (there is no cvxpy
    check to skip); ``solver_options`` understands ``max_nodes`` (the node budget: when it runs out a
    ``ConvergenceWarning`` is raised and the incumbent kept), ``device``, ``wide`` and ``bound``.  ``bound="exclusion"`` cuts a
    subtree against the value on every column the path has NOT excluded instead of the value on all columns (the default,
    ``"q_all"``): far fewer nodes at a small ``alpha`` or a tight ``sparse_bound``, each a little dearer, the same ``coef_``.
    ``solver_info_`` then holds ``bound`` (``"exclusion"`` with ``bound_margin``, the relative safety margin of the bound; or
    ``"q_all"`` with ``bound_reason`` where the search fell back: a Gram that is not positive definite on all columns, e.g.
    ``n < p`` without a ridge term, or one too ill-conditioned for the margin).  Refused: ``L1L0``, constraints and
    ``l0_profile`` with ``bound``.  ``wide=True`` admits up to 128 columns
    and 128 groups: a problem within the narrow limits still takes the narrow search (the same bits), a wider one the wide
    search, in which a support holds at most 64 independent columns.  Where that cap cut the search and the result is not
    proven all the same, ``solver_info_["status"]`` is ``"capacity"``, ``solver_info_["capacity_cut"]`` the number of groups
    from which includes were refused, and a ``ConvergenceWarning`` names the bound.

    ``constraints`` (None, or the list that ``add_constraints`` built from ``scipy.optimize.LinearConstraint`` / ``Bounds``
    objects) is an attribute, not a constructor argument -- the constructors are the reference's, which attaches constraints
    through ``add_constraints`` too -- so ``get_params`` / ``set_params`` do not know it; ``clone`` carries it over.  The
    constraints act on ``coef_``, never on the intercept.  The fit then also sets ``constraint_multipliers_`` (one array per object; > 0: ``ub`` binds, < 0: ``lb`` binds;
    a ``Bounds`` entry folded into the box reports the box multiplier) and ``solver_info_`` holds ``constrained`` (True),
    ``qp_solves`` (candidates that passed the lower-bound filter and were valued on chip), ``unsettled`` (candidates whose
    sweeps ran out: ``solver_options["max_qp_sweeps"]``, default 20000), ``con_tol`` (rows and duality gap of a valued
    candidate, relative) and ``max_violation`` (of ``coef_``, over every constraint).  ``status`` may be ``"unsettled"``: some
    candidate's lower bound is below the incumbent, which is kept unproven under a ``ConvergenceWarning`` that names the bound.
    A ``ValueError`` says so when no admissible support satisfies the constraints.
    """

    _wide_mode = True  # (L1L0: there is no wide l1 mode)
    _constrained_mode = True  # (L1L0: nor a constrained one)
    _bound_mode = True  # (L1L0: nor an exclusion bound)

    constraints = None  # (set by ``add_constraints`` alone: the constructors stay the reference's)

    def add_constraints(self, constraints):
        """Append linear constraints (a ``LinearConstraint`` / ``Bounds`` or a list of them) to ``self.constraints`` -- the
        semantics of ``ProxRegressor.add_constraints``: a new list is built, the caller's list is never changed.  Returns the
        estimator."""
        old = [] if self.constraints is None else _as_list(self.constraints)
        self.constraints = old + _as_list(constraints)
        return self

    def __sklearn_clone__(self):
        """``constraints`` is no constructor parameter, so ``clone`` (``GridSearchCV``, ``cross_val_score``) would drop it:
        the copy gets a list of its own with the same constraint objects."""
        new = _clone_parametrized(self)
        if self.constraints is not None:
            new.constraints = list(self.constraints)
        return new

    def _l0_constraints(self, n_features, options):
        """``constraints`` validated and folded, before a device is touched; None without constraints."""
        if self.constraints is None:
            return None
        if not self._constrained_mode:
            raise ValueError(f"{self.__class__.__name__} takes no constraints: the constrained search has no l1 term")
        if options.get("wide"):
            raise ValueError("constraints and solver_options['wide'] do not go together: the constrained search takes up to "
                             f"{_NARROW} columns and groups")
        if "bound" in options:
            raise ValueError("constraints and solver_options['bound'] do not go together: the constrained search keeps the bound "
                             "on all columns (its values are quadratic programmes, not q)")
        folded = _FoldedConstraints(self.constraints, n_features)
        check_feasible(folded.cs)
        return folded

    _parameter_constraints: dict = {
        "ignore_psd_check": ["boolean"],
        "fit_intercept": ["boolean"],
        "copy_X": ["boolean"],
        "warm_start": ["boolean"],
        "solver": [str, None],
        "solver_options": [dict, None],
    }
    _hyper_parameter_constraints: dict = {"big_M": [Interval(type=Real, left=0.0, right=None, closed="left")]}

    def _validate_params(self, X, y) -> None:
        constraints = dict(self._parameter_constraints)
        constraints.update(self._hyper_parameter_constraints)
        params = self.get_params(deep=False)
        validate_parameter_constraints(constraints, {k: params[k] for k in constraints}, caller_name=self.__class__.__name__)
        check_groups(self.groups, X.shape[1])

    # what the sub-classes say about the problem
    def _l0_problem(self, n_groups):
        """(alpha, max_groups, eta)"""
        raise NotImplementedError

    def _tikhonov(self, n_features):
        return None

    def _l1_weight(self):
        """The weight of ``||beta||_1`` in the objective (``L1L0``); 0: none, the search without an l1 term."""
        return 0.0

    def _l0_setup(self, X, y, sample_weight):
        """Everything a search needs, validated before a device is touched (shared with ``l0_profile``, _l0_profile.py):
        ``(X, y, options, gidx, n_groups, need, T, w)`` with the hierarchy as masks and the sample weights normalised to sum n."""
        X, y = validate_data(self, X, y, accept_sparse=False, y_numeric=True, multi_output=False)
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        self._validate_params(X, y)
        options = {} if self.solver_options is None else dict(self.solver_options)
        unknown = set(options) - _KNOWN_OPTIONS
        if unknown:
            raise ValueError(f"unknown solver_options {sorted(unknown)}: the exact l0 search takes {sorted(_KNOWN_OPTIONS)}")
        if not isinstance(options.get("wide", False), (bool, np.bool_)):
            raise ValueError("solver_options['wide'] must be a bool")
        if options.get("wide") and not self._wide_mode:
            raise ValueError(f"{self.__class__.__name__} has no wide mode: the l1 search takes up to {_NARROW} columns and groups")
        if "bound" in options:
            if options["bound"] not in _BOUNDS:
                raise ValueError(f"solver_options['bound'] must be one of {list(_BOUNDS)} (got {options['bound']!r})")
            if not self._bound_mode:
                raise ValueError(f"{self.__class__.__name__} has no exclusion bound: solver_options['bound'] serves the search "
                                 "without an l1 term")
        p = X.shape[1]
        gidx, n_groups = dense_group_index(self.groups, p)
        need = _hierarchy_masks(self.hierarchy, self.groups, p)
        T = self._tikhonov(p)
        w = None
        if sample_weight is not None:
            w = _check_sample_weight(sample_weight, X, dtype=X.dtype)
            w = w * (X.shape[0] / np.sum(w))
        return X, y, options, gidx, n_groups, need, T, w

    @contextlib.contextmanager
    def _l0_dataset(self, X, y, w, gidx, n_groups, need, options):
        """The dataset of a search on its device, centred when an intercept is fitted: yields ``(ds, x_mean, y_mean, need,
        max_nodes)``."""
        from .. import _engine

        eng = _engine.get_engine(options.get("device"))
        with eng.dataset(X, y, row_weight=w) as ds:
            x_mean, y_mean = ds.center() if self.fit_intercept else (np.zeros(X.shape[1]), 0.0)
            ds.set_groups(gidx, n_groups)
            if need is not None and n_groups > _NARROW and not options.get("wide"):
                need = None  # (the engine refuses the size itself; masks of more than 64 groups have no 64-bit form)
            yield ds, x_mean, y_mean, need, int(options.get("max_nodes", 0) or 0)

    def fit(self, X, y, sample_weight=None):
        # everything is validated before a device is touched
        X, y, options, gidx, n_groups, need, T, w = self._l0_setup(X, y, sample_weight)
        alpha, max_groups, eta = self._l0_problem(n_groups)
        eta_l1 = float(self._l1_weight())
        # (wide: only a problem beyond the narrow limits takes the wide search -- within them the bits stay what they were)
        wide = bool(options.get("wide")) and (X.shape[1] > _NARROW or n_groups > _NARROW)
        folded = self._l0_constraints(X.shape[1], options)
        xb = options.get("bound") == "exclusion"
        lam = None
        with self._l0_dataset(X, y, w, gidx, n_groups, need, options) as (ds, x_mean, y_mean, need, max_nodes):
            if folded is not None:
                beta, support, lam, info = ds.solve_l0_constrained(
                    folded.A, folded.lo, folded.hi, alpha=alpha, max_groups=max_groups, eta=eta, T=T, big_M=float(self.big_M),
                    need=need, max_nodes=max_nodes, box_lo=folded.box_lo, box_hi=folded.box_hi,
                    max_qp_sweeps=int(options.get("max_qp_sweeps", 0) or 0))
            elif eta_l1 > 0.0:
                beta, support, info = ds.solve_l0_l1(alpha=alpha, eta_l1=eta_l1, big_M=float(self.big_M), need=need, max_nodes=max_nodes)
            elif wide:
                solve = ds.solve_l0_xb_wide if xb else ds.solve_l0_wide
                beta, support, info = solve(alpha=alpha, max_groups=max_groups, eta=eta, T=T, big_M=float(self.big_M), need=need,
                                            max_nodes=max_nodes)
            else:
                try:
                    solve = ds.solve_l0_xb if xb else ds.solve_l0
                    beta, support, info = solve(alpha=alpha, max_groups=max_groups, eta=eta, T=T, big_M=float(self.big_M), need=need,
                                                max_nodes=max_nodes)
                except NotImplementedError as exc:
                    if options.get("wide") or max(X.shape[1], n_groups) <= _NARROW:
                        raise
                    raise NotImplementedError(f"{exc}; solver_options={{'wide': True}} takes up to 128 of each") from None
        if options.get("bound") == "q_all":  # (asked for by name: the default search, and the keys say so)
            info["bound"] = "q_all"
            info["bound_reason"] = "solver_options['bound'] = 'q_all'"
        if info["status"] == "capacity":
            warnings.warn(
                f"a support holds at most {_NARROW} independent columns: includes were refused from {info['capacity_cut']} groups on, "
                f"and the incumbent (objective {info['objective']:.6g}) is above the bound {info['lower_bound']:.6g} on what lies "
                "behind them; it is kept, unproven",
                ConvergenceWarning,
            )
        elif info["status"] == "unsettled":
            warnings.warn(
                f"{info['unsettled']} candidate support(s) ran out of sweeps: the incumbent (objective {info['objective']:.6g}) is "
                f"above the proven lower bound {info['lower_bound']:.6g} on them; it is kept, unproven -- raise "
                "solver_options['max_qp_sweeps']",
                ConvergenceWarning,
            )
        elif not info["proven_optimal"]:
            warnings.warn(
                f"the node budget ran out after {info['nodes']} nodes: the incumbent (objective {info['objective']:.6g}, proven "
                f"lower bound {info['lower_bound']:.6g}) is kept; raise solver_options['max_nodes']",
                ConvergenceWarning,
            )
        self.coef_ = beta
        self.active_groups_ = np.array([(support >> i) & 1 for i in range(n_groups)], dtype=bool)
        self.solver_info_ = info
        self.intercept_ = float(y_mean - np.dot(x_mean, beta)) if self.fit_intercept else 0.0
        if folded is not None:
            # the box multipliers from X: mu = -(H beta - c + A^T lambda), H beta - c the gradient of the smooth part
            Xc, yc = X - x_mean, y - y_mean
            r = Xc @ beta - yc
            g = Xc.T @ (r if w is None else w * r) / X.shape[0]
            if eta > 0.0:
                g = g + 2.0 * eta * (beta if T is None else 0.5 * (T + T.T) @ beta)
            mu = -(g + folded.A.T @ lam)
            gidx_ = np.arange(X.shape[1]) if gidx is None else np.asarray(gidx)
            self.constraint_multipliers_ = folded.split(lam, beta, mu, self.active_groups_[gidx_])
            info["max_violation"] = folded.cs.violation(beta)
        return self

    def predict(self, X):
        check_is_fitted(self)
        X = validate_data(self, X, accept_sparse=False, reset=False)
        return X @ self.coef_ + self.intercept_

    def __sklearn_tags__(self):
        tags = super().__sklearn_tags__()
        tags.target_tags.single_output = True
        return tags


class _TikhonovMixin:
    """``eta ||W beta||^2`` (reference ``TikhonovMixin``, _base.py:522-548); ``W = I`` when ``tikhonov_w`` is None."""

    def _tikhonov(self, n_features):
        if self.tikhonov_w is None:
            return None
        W = np.asarray(self.tikhonov_w, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] != n_features:
            raise ValueError(f"tikhonov_w must have {n_features} columns")
        return W.T @ W


class BestSubsetSelection(_ExactL0):
    """Best subset selection: at most ``sparse_bound`` active groups (reference _best_subset.py:24-139), solved exactly.

    Args as in the reference: ``groups`` (None: every feature its own group), ``sparse_bound``, ``big_M`` (bound on every
    ``|coef_j|``), ``hierarchy`` (entry i lists the group labels the i-th sorted label depends on), ``ignore_psd_check``,
    ``fit_intercept``, ``copy_X``, ``warm_start``, ``solver``, ``solver_options``.
    """

    _hyper_parameter_constraints: dict = {
        "sparse_bound": [Interval(type=Real, left=0, right=None, closed="left")],
        **_ExactL0._hyper_parameter_constraints,
    }

    def __init__(self, groups=None, sparse_bound=100, big_M=100, hierarchy=None, ignore_psd_check=True, fit_intercept=False,
                 copy_X=True, warm_start=False, solver=None, solver_options=None):
        self.groups = groups
        self.sparse_bound = sparse_bound
        self.big_M = big_M
        self.hierarchy = hierarchy
        self.ignore_psd_check = ignore_psd_check
        self.fit_intercept = fit_intercept
        self.copy_X = copy_X
        self.warm_start = warm_start
        self.solver = solver
        self.solver_options = solver_options

    def _l0_problem(self, n_groups):
        return 0.0, int(min(np.floor(self.sparse_bound), n_groups)), 0.0


class RidgedBestSubsetSelection(_TikhonovMixin, BestSubsetSelection):
    """Best subset selection with a ridge / Tikhonov term ``eta ||W beta||^2`` (reference _best_subset.py:142-248)."""

    _hyper_parameter_constraints: dict = {
        "eta": [Interval(type=Real, left=0.0, right=None, closed="left")],
        **BestSubsetSelection._hyper_parameter_constraints,
    }

    def __init__(self, groups=None, sparse_bound=100, eta=1.0, big_M=100, hierarchy=None, tikhonov_w=None,
                 ignore_psd_check=True, fit_intercept=False, copy_X=True, warm_start=False, solver=None, solver_options=None):
        super().__init__(groups=groups, sparse_bound=sparse_bound, big_M=big_M, hierarchy=hierarchy,
                         ignore_psd_check=ignore_psd_check, fit_intercept=fit_intercept, copy_X=copy_X, warm_start=warm_start,
                         solver=solver, solver_options=solver_options)
        self.tikhonov_w = tikhonov_w
        self.eta = eta

    def _l0_problem(self, n_groups):
        return 0.0, int(min(np.floor(self.sparse_bound), n_groups)), float(self.eta)


class RegularizedL0(_ExactL0):
    """``1/(2n)||X beta - y||^2 + alpha |S|`` over active groups S (reference _regularized_l0.py:39-161), solved exactly."""

    _hyper_parameter_constraints: dict = {
        "alpha": [Interval(type=Real, left=0.0, right=None, closed="left")],
        **_ExactL0._hyper_parameter_constraints,
    }

    def __init__(self, groups=None, alpha=1.0, big_M=100, hierarchy=None, ignore_psd_check=True, fit_intercept=False,
                 copy_X=True, warm_start=False, solver=None, solver_options=None):
        self.groups = groups
        self.alpha = alpha
        self.big_M = big_M
        self.hierarchy = hierarchy
        self.ignore_psd_check = ignore_psd_check
        self.fit_intercept = fit_intercept
        self.copy_X = copy_X
        self.warm_start = warm_start
        self.solver = solver
        self.solver_options = solver_options

    def _l0_problem(self, n_groups):
        return float(self.alpha), n_groups, 0.0


class L2L0(_TikhonovMixin, RegularizedL0):
    """``RegularizedL0`` with a ridge / Tikhonov term ``eta ||W beta||^2`` (reference _regularized_l0.py:413-530)."""

    _hyper_parameter_constraints: dict = {
        "eta": [Interval(type=Real, left=0.0, right=None, closed="left")],
        **RegularizedL0._hyper_parameter_constraints,
    }

    def __init__(self, groups=None, alpha=1.0, eta=1.0, big_M=100, hierarchy=None, tikhonov_w=None, ignore_psd_check=True,
                 fit_intercept=False, copy_X=True, warm_start=False, solver=None, solver_options=None):
        super().__init__(groups=groups, alpha=alpha, big_M=big_M, hierarchy=hierarchy, ignore_psd_check=ignore_psd_check,
                         fit_intercept=fit_intercept, copy_X=copy_X, warm_start=warm_start, solver=solver,
                         solver_options=solver_options)
        self.tikhonov_w = tikhonov_w
        self.eta = eta

    def _l0_problem(self, n_groups):
        return float(self.alpha), n_groups, float(self.eta)
