"""The LOCAL PROOF WITH GROUPS AND A HIERARCHY: branch and bound over GROUP nodes, which proves a cell of the grouped l0 local
search's grid OPTIMAL where its tree closes (``slm_solve_l0_local_group_prove``, csrc/l0_local_group_node_kernels.hpp; the tree:
``l0_prove_tree`` with a group map, csrc/l0_host.hpp).

``l0_local_group_search`` returns a closed support and proves nothing; its screen can miss a group.  This is the other half, for
the same objective

    F(beta) = 1/2 beta^T (G + 2 eta I) beta - c^T beta + alpha |cl(S(beta))|,   |beta_j| <= big_M.

Each group's indicator is relaxed to ``z_g`` in [0, 1] with ``|beta_j| <= M z_g`` and the cost ``eta ||beta_g||^2 / z_g + alpha z_g``;
the group penalty that leaves has the conjugate ``max(0, sum_{j in g} h(t_j) - alpha)`` (``h`` as in ``l0_local_bound``).  A NODE
gives every group one state -- FREE, IN (it pays ``alpha`` whether zero or not) or OUT (``beta_g = 0``) -- and for EVERY ``u``,
with ``t = c - G u``,

    L_node(u) = -1/2 u^T G u - sum over FREE g of max(0, sum_{j in g} h(t_j) - alpha) - sum over IN g of (sum_{j in g} h(t_j) - alpha)

is at or below the minimum of ``F`` over the node.  The relaxation ignores the hierarchy (``|cl(S)| >= |S|``); the hierarchy
lives in the branching: the IN child of a group sets it and everything it needs IN, the OUT child sets it and everything that
needs it OUT.  Rounds, pruning and the reported bound are ``l0_local_prove``'s, and with singleton groups and no hierarchy the
result is ``l0_local_prove``'s, field for field.

WHERE THE TREE CLOSES AND WHERE NOT: with a ridge (``eta > 0``) or a box that binds it closes in a few to a few dozen nodes.  At
``eta = 0`` under a loose ``big_M`` the relaxation of a FREE group costs next to nothing, and with a deep hierarchy whose free
groups are cheap the bound cannot see the price of what a group needs: the call ends at ``max_nodes`` with an honest, smaller
proven gap (DESIGN 4d "Local proof with groups").

Not built: a hierarchy-aware relaxation (``z_g <= z_parent``), the cardinality form, the l1 entry, row sets (folds), a Tikhonov
matrix, rerouting ``GridSearchCV``.

Import path: ``sparselm_amd.miqp`` (``l0_local_group_prove``, ``L0LocalGroupProof``).
"""

from __future__ import annotations

import warnings
from numbers import Integral, Real

import numpy as np
from sklearn.exceptions import ConvergenceWarning

from ._l0_local_groups import L0LocalGroupPath, _group_rounds, _GroupPlan
from ._l0_local_prove import _LEAF_BYTES, _MAX_CELLS, _STATUS, L0LocalProof, _bits, _same_grid

__all__ = ["l0_local_group_prove", "L0LocalGroupProof"]

_OPTIONS = {"device"}


class L0LocalGroupProof(L0LocalProof):
    """What ``l0_local_group_prove`` returns: ``L0LocalProof``'s fields per cell of ``alphas_ x etas_`` (``coefs_`` in the caller's
    column order; ``objectives_`` count ``alpha |cl(S)|``; ``proven_optimal_`` True where the tree closed) plus ``group_supports_``
    (A x E x n_groups, bool, in the order of the sorted labels: cl(S) of the incumbent) and ``n_active_groups_``.  In a
    ``certificate_`` the masks ``in_`` and ``out_`` are BY GROUP (leaves x n_groups); ``u`` is in the caller's column order."""

    def __init__(self, *tables, group_supports, certificate=None):
        super().__init__(*tables, certificate)
        self.group_supports_ = np.asarray(group_supports, dtype=bool)
        self.n_active_groups_ = self.group_supports_.sum(axis=-1)


def l0_local_group_prove(X, y, *, alphas, groups=None, hierarchy=None, etas=(0.0,), big_M=100, fit_intercept=False, sample_weight=None,
                         path=None, rel_gap=1e-6, max_nodes=20000, width=32, max_sweeps=None, return_certificate=False,
                         solver_options=None) -> L0LocalGroupProof:
    """Branch and bound over group nodes at every cell of ``alphas x etas``, for up to 1024 grouped columns under a hierarchy,
    on the GPU.

    ``groups``, ``hierarchy`` and the data arguments are ``l0_local_group_search``'s, validated and permuted by the same code.
    ``path``: the incumbents -- None runs ``l0_local_group_search`` on the same dataset handle first; an ``L0LocalGroupPath`` must
    be on this grid, these groups and this hierarchy (else ``ValueError``).  ``rel_gap``, ``max_nodes``, ``width``, ``max_sweeps``,
    ``return_certificate`` and ``solver_options`` (``device``) as for ``l0_local_prove``.  A ``ConvergenceWarning`` is raised when
    cells ended at the node limit; their ``lower_bounds_`` are proven all the same.  The tree closes with a ridge or a box that
    binds; at ``eta = 0`` under a loose box, and with deep hierarchies whose free groups are cheap, it does not."""
    options = {} if solver_options is None else solver_options
    if not isinstance(options, dict):
        raise ValueError("solver_options must be a dict or None")
    unknown = set(options) - _OPTIONS
    if unknown:
        raise ValueError(f"unknown solver_options {sorted(unknown)}: the grouped l0 local proof takes {sorted(_OPTIONS)}")
    if not isinstance(rel_gap, Real) or isinstance(rel_gap, bool) or not 1e-10 <= rel_gap <= 1.0:
        raise ValueError("rel_gap must be a number in [1e-10, 1]")
    for name, value in (("max_nodes", max_nodes), ("width", width)):
        if not isinstance(value, Integral) or isinstance(value, bool) or value < 1:
            raise ValueError(f"{name} must be an integer >= 1")
    if max_sweeps is not None and (not isinstance(max_sweeps, Integral) or isinstance(max_sweeps, bool) or max_sweeps < 1):
        raise ValueError("max_sweeps must be an integer >= 1 or None")
    if path is not None and not isinstance(path, L0LocalGroupPath):
        raise ValueError("path must be an L0LocalGroupPath or None")
    # everything is validated before a device is touched
    plan = _GroupPlan(X, y, alphas, groups, hierarchy, etas, big_M, fit_intercept, sample_weight, None, 2, options or None)
    A, E, p, al, et, n_groups = plan.A, plan.E, plan.p, plan.al, plan.et, len(plan.gstart) - 1
    if A * E > _MAX_CELLS:
        raise ValueError(f"the grid holds {A * E} cells: more than the {_MAX_CELLS} cells of one call")
    if path is not None:
        if not _same_grid(path, al, et) or np.asarray(path.coefs_).shape != (A, E, p):
            raise ValueError("the path and the proof are on different (alpha, eta) grids")
        incumbents = np.ascontiguousarray(np.asarray(path.coefs_, dtype=float)[..., plan.perm])
        if not np.all(np.abs(incumbents) <= plan.big_M):  # (a NaN fails too)
            raise ValueError(f"the path's coefficients must lie inside the box |beta_j| <= big_M = {plan.big_M:g}")
        mine = plan.group_supports(incumbents)
        if np.asarray(path.group_supports_).shape != mine.shape or np.any(np.asarray(path.group_supports_) != mine):
            raise ValueError("the path and the proof are on different groups or hierarchies")
    elif A * E * plan.most > _MAX_CELLS:
        raise ValueError(f"the grid holds {A * E} cells with up to {plan.most} starts each: more than the {_MAX_CELLS} problems of one launch "
                         "of the grouped local search; pass path=")

    with plan.spec._l0_dataset(plan.X, plan.y, plan.w, plan.gidx, plan.n_groups, None, plan.dev_options) as (ds, x_mean, y_mean, _, _):
        if path is None:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", ConvergenceWarning)  # (an incumbent need not be a fixed point)
                incumbents = _group_rounds(ds, plan, 2)[0]
        capacity = min(A * E * int(max_nodes), max(4096, _LEAF_BYTES // (8 * (p + 40)))) if return_certificate else 0
        while True:
            out = ds.solve_l0_local_group_prove(plan.cell_alpha, plan.cell_eta, need=plan.need, big_M=plan.big_M,
                                                incumbents=incumbents.reshape(A * E, p), rel_gap=float(rel_gap), max_nodes=int(max_nodes),
                                                width=int(width), max_sweeps=0 if max_sweeps is None else int(max_sweeps),
                                                leaf_capacity=capacity)
            if not return_certificate or out["leaves"]["count"] <= capacity:
                break
            capacity = out["leaves"]["count"]  # (the tree is deterministic: the second call grows the same one)
    status = np.array(out["status"]).reshape(A, E)
    if status.any():
        a, e = np.argwhere(status != 0)[0]
        warnings.warn(f"the node limit ({int(max_nodes)}) ran out in {int((status != 0).sum())} of {A * E} cells (the first: alpha index {a}, "
                      f"eta index {e}): they are not proven optimal, their lower bounds are proven all the same", ConvergenceWarning)
    permuted = np.array(out["beta"]).reshape(A, E, p)
    coefs = plan.unpermute(permuted)
    intercepts = np.array([[float(y_mean - np.dot(x_mean, permuted[a, e])) if fit_intercept else 0.0 for e in range(E)] for a in range(A)])
    certificate = None
    if return_certificate:
        lv = out["leaves"]
        certificate = {"cell": np.stack(np.divmod(np.asarray(lv["cell"], dtype=int), E), axis=1), "in_": _bits(lv["in_mask"], n_groups),
                       "out_": _bits(lv["out_mask"], n_groups), "u": plan.unpermute(np.array(lv["u"])), "lower": np.array(lv["lower"])}
    names = np.array(_STATUS, dtype=object)[status]
    return L0LocalGroupProof(al, et, coefs, intercepts, np.array(out["objective"]).reshape(A, E), np.array(out["lower_bound"]).reshape(A, E),
                             np.array(out["nodes"]).reshape(A, E), np.array(out["rounds"]).reshape(A, E), names,
                             group_supports=np.array(out["group_support"]).reshape(A, E, -1) != 0, certificate=certificate)
