"""The LOCAL PROOF: branch and bound on the local bound, which proves a cell of the l0 local search's grid OPTIMAL where its tree
closes (``slm_solve_l0_local_prove``, csrc/l0_local_node_kernels.hpp; the tree: ``l0_prove_tree``, csrc/l0_host.hpp).

``l0_local_search`` returns a support and proves nothing; ``l0_local_bound`` returns a proven number for the root alone, which
at ``eta = 0`` under a loose ``big_M`` lies far below the optimum.  This is where the two meet (the L0BnB scheme of Hazimeh,
Mazumder and Saab).  A NODE fixes some columns IN (they pay ``alpha`` whether their coefficient is zero or not) and some OUT
(``beta_j = 0``); the bound's relaxation on a node is the same separable convex problem with three kinds of coordinate, and for
EVERY vector ``u``, with ``t = c - G u``,

    L_node(u) = -1/2 u^T G u - sum over FREE of max(0, h(t_j) - alpha) - sum over IN of (h(t_j) - alpha)
             <=  min { F(beta) : |beta_j| <= big_M, beta_OUT = 0, IN columns pay alpha whether zero or not }

(``h`` as in ``l0_local_bound``).  A best-first tree over such nodes is pruned against the incumbent of the local search: a
round pops the ``width`` open nodes of lowest bound of every cell, splits each on the FREE column whose relaxed indicator
``z_j = min(|u_j| / tauc, 1)`` is closest to 1/2 (ties: the lowest index; where every ``z_j`` is 0 or 1, the largest ``|u_j|``,
then the largest ``|t_j|``), and bounds the children of ALL cells in ONE launch, one wavefront per node.  A node whose own point
``u`` beats the incumbent replaces it.  A node is dropped when ``best - lower <= rel_gap max(|best|, alpha)``; a cell whose open
list is empty is PROVEN OPTIMAL to ``rel_gap``, and a cell that reaches ``max_nodes`` reports ``min(best, lowest open bound)``,
which is proven all the same.

WHERE THE TREE CLOSES AND WHERE NOT: it closes with a ridge (``eta > 0``) or a box that binds, where the root bound is already
close and a few dozen to a few hundred nodes settle the rest.  At ``eta = 0`` with ``p > n`` it does not: the relaxation of a
node is then next to free in every FREE column, the bound rises only with depth, and the tree is the full enumeration; the
call ends at ``max_nodes`` with an honest, smaller proven gap (DESIGN 4d "Local proof" has the measured counts).

Not built: the cardinality form, the l1 entry, row sets (folds), a Tikhonov matrix, strengthening
``eta = 0`` by extracting a diagonal from G, feeding the bound into the exact search over supports.  (Groups and a hierarchy:
``l0_local_group_prove``, ``model/_l0_local_group_prove.py``.)

Import path: ``sparselm_amd.miqp`` (``l0_local_prove``, ``L0LocalProof``).
"""

from __future__ import annotations

import warnings
from numbers import Integral, Real

import numpy as np
from sklearn.exceptions import ConvergenceWarning

from ._l0_local import _PMAX, L0LocalPath, _first_starts, _grid, _LocalProblem, _round_moves, _search_rounds

__all__ = ["l0_local_prove", "L0LocalProof"]

_MAX_CELLS = 8192  # SLM_L0_LOCAL_MAX_PROBLEMS: the cells of one call
_OPTIONS = {"device"}
_STATUS = ("optimal", "node_limit")
_LEAF_BYTES = 1 << 28  # what a certificate's arrays may take at the first call: a tree with more leaves than fit is grown a second time


class L0LocalProof:
    """What ``l0_local_prove`` returns, per cell of the grid ``alphas_ x etas_``.

    ``coefs_`` (A x E x p), ``intercepts_``, ``objectives_`` (the incumbent, in the units of ``L0LocalPath.objectives_``),
    ``lower_bounds_`` (proven: at or below the cell's optimum), ``gaps_`` (``(objective - lower bound) / max(|objective|,
    alpha)``, never negative), ``proven_optimal_`` (True: the tree closed, the objective is optimal to ``rel_gap``), ``nodes_``
    (bound evaluations), ``rounds_`` (launches the cell took part in), ``status_`` (``"optimal"`` or ``"node_limit"``) and, when
    asked for, ``certificate_``: a dict with every dropped node's ``cell`` (``(alpha index, eta index)`` rows), ``in_`` and
    ``out_`` (bool, leaves x p), ``u`` and ``lower`` -- enough to check the proof with nothing but numpy (else None)."""

    def __init__(self, alphas, etas, coefs, intercepts, objectives, lower_bounds, nodes, rounds, status, certificate=None):
        self.alphas_ = np.asarray(alphas, dtype=float)
        self.etas_ = np.asarray(etas, dtype=float)
        self.coefs_ = np.asarray(coefs, dtype=float)
        self.intercepts_ = np.asarray(intercepts, dtype=float)
        self.objectives_ = np.asarray(objectives, dtype=float)
        self.lower_bounds_ = np.asarray(lower_bounds, dtype=float)
        self.gaps_ = np.maximum(self.objectives_ - self.lower_bounds_, 0.0) / np.maximum(np.abs(self.objectives_), self.alphas_[:, None])
        self.nodes_ = np.asarray(nodes, dtype=int)
        self.rounds_ = np.asarray(rounds, dtype=int)
        self.status_ = np.asarray(status, dtype=object)
        self.proven_optimal_ = self.status_ == "optimal"
        self.certificate_ = certificate


def _same_grid(path, al, et):
    pa, pe = np.asarray(path.alphas_, dtype=float), np.asarray(path.etas_, dtype=float)
    return pa.shape == al.shape and pe.shape == et.shape and not np.any(pa != al) and not np.any(pe != et)


def _bits(words, p):
    """[leaves, 16] words of 64 bits -> [leaves, p] bool: bit ``j & 63`` of word ``j >> 6`` is column ``j``."""
    w = np.ascontiguousarray(words, dtype="<u8")
    return np.unpackbits(w.view(np.uint8).reshape(len(w), -1), axis=1, bitorder="little")[:, :p].astype(bool)


def l0_local_prove(X, y, *, alphas, etas=(0.0,), big_M=100, fit_intercept=False, sample_weight=None, path=None, rel_gap=1e-6,
                   max_nodes=20000, width=32, max_sweeps=None, return_certificate=False, solver_options=None) -> L0LocalProof:
    """Branch and bound on the local bound at every cell of ``alphas x etas``, for up to 1024 columns, on the GPU.

    The arguments are ``l0_local_search``'s, and validation, centring and weights are the same code, so all three of the family
    see the same ``G``, ``c`` and objective units.  ``path``: the incumbents -- None runs ``l0_local_search`` on the same dataset
    handle first; an ``L0LocalPath`` must be on this grid (else ``ValueError``).  ``rel_gap`` in [1e-10, 1]: a node is dropped
    when it cannot improve the incumbent by more than ``rel_gap max(|best|, alpha)``, which is what "optimal" means here.
    ``max_nodes``: bound evaluations per cell; ``width``: nodes a cell splits per round (all children of all cells of a round
    are one launch of at most 8192 nodes).  ``max_sweeps``: the cap on a node's sweeps (None: 10000).  ``return_certificate``:
    every dropped node's masks and ``u`` come back, for an independent check (the arrays are sized for ``cells x max_nodes`` leaves, up to
    256 MB; only a tree with more leaves than fit there runs a second time, at twice the cost).  ``solver_options``: ``device``.  A
    ``ConvergenceWarning`` is raised when cells ended at the node limit; their ``lower_bounds_`` are proven all the same.  The
    tree closes with a ridge or a box that binds; at ``eta = 0`` with ``p > n`` it does not."""
    options = {} if solver_options is None else solver_options
    if not isinstance(options, dict):
        raise ValueError("solver_options must be a dict or None")
    unknown = set(options) - _OPTIONS
    if unknown:
        raise ValueError(f"unknown solver_options {sorted(unknown)}: the l0 local proof takes {sorted(_OPTIONS)}")
    if not isinstance(rel_gap, Real) or isinstance(rel_gap, bool) or not 1e-10 <= rel_gap <= 1.0:
        raise ValueError("rel_gap must be a number in [1e-10, 1]")
    for name, value in (("max_nodes", max_nodes), ("width", width)):
        if not isinstance(value, Integral) or isinstance(value, bool) or value < 1:
            raise ValueError(f"{name} must be an integer >= 1")
    if max_sweeps is not None and (not isinstance(max_sweeps, Integral) or isinstance(max_sweeps, bool) or max_sweeps < 1):
        raise ValueError("max_sweeps must be an integer >= 1 or None")
    if path is not None and not isinstance(path, L0LocalPath):
        raise ValueError("path must be an L0LocalPath or None")
    spec = _LocalProblem(big_M=big_M, fit_intercept=fit_intercept, solver_options=options or None)
    # everything is validated before a device is touched
    X, y, dev_options, gidx, n_groups, need, _, w = spec._l0_setup(X, y, sample_weight)
    al, et = _grid(alphas, "alphas"), _grid(etas, "etas")
    A, E, p = len(al), len(et), X.shape[1]
    if p > _PMAX:
        raise NotImplementedError(f"the l0 local proof takes up to {_PMAX} columns (got {p})")
    if A * E > _MAX_CELLS:
        raise ValueError(f"the grid holds {A * E} cells: more than the {_MAX_CELLS} cells of one call")
    big_M = float(big_M)
    if path is not None:
        if not _same_grid(path, al, et) or np.asarray(path.coefs_).shape != (A, E, p):
            raise ValueError("the path and the proof are on different (alpha, eta) grids")
        incumbents = np.ascontiguousarray(path.coefs_, dtype=float)
        if not np.all(np.abs(incumbents) <= big_M):  # (a NaN fails too)
            raise ValueError(f"the path's coefficients must lie inside the box |beta_j| <= big_M = {big_M:g}")
    moves = _round_moves(A, E, 2)
    if path is None and A * E * max(1, len(moves)) > _MAX_CELLS:
        raise ValueError(f"the grid holds {A * E} cells with up to {max(1, len(moves))} starts each: more than the {_MAX_CELLS} problems of "
                         "one launch of the local search; pass path=")
    cell_alpha, cell_eta = np.repeat(al, E), np.tile(et, A)

    with spec._l0_dataset(X, y, w, gidx, n_groups, need, dev_options) as (ds, x_mean, y_mean, _, _):
        if path is None:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", ConvergenceWarning)  # (an incumbent need not be a fixed point)
                incumbents = _search_rounds(ds, al, et, big_M, _first_starts(None, A, E, p, big_M), moves, 2, True)[0]
        # (every bound evaluation leaves at most one leaf, so cells x max_nodes leaves always suffice; where that many rows of p doubles
        #  pass _LEAF_BYTES the arrays start smaller, and only a tree that outgrows them is grown again -- it is deterministic)
        capacity = min(A * E * int(max_nodes), max(4096, _LEAF_BYTES // (8 * (p + 40)))) if return_certificate else 0
        while True:
            out = ds.solve_l0_local_prove(cell_alpha, cell_eta, big_M=big_M, incumbents=incumbents.reshape(A * E, p), rel_gap=float(rel_gap),
                                          max_nodes=int(max_nodes), width=int(width), max_sweeps=0 if max_sweeps is None else int(max_sweeps),
                                          leaf_capacity=capacity)
            if not return_certificate or out["leaves"]["count"] <= capacity:
                break
            capacity = out["leaves"]["count"]  # (the tree is deterministic: the second call grows the same one)
    status = np.array(out["status"]).reshape(A, E)
    if status.any():
        a, e = np.argwhere(status != 0)[0]
        warnings.warn(f"the node limit ({int(max_nodes)}) ran out in {int((status != 0).sum())} of {A * E} cells (the first: alpha index {a}, "
                      f"eta index {e}): they are not proven optimal, their lower bounds are proven all the same", ConvergenceWarning)
    coefs = np.array(out["beta"]).reshape(A, E, p)
    intercepts = np.array([[float(y_mean - np.dot(x_mean, coefs[a, e])) if fit_intercept else 0.0 for e in range(E)] for a in range(A)])
    certificate = None
    if return_certificate:
        lv = out["leaves"]
        certificate = {"cell": np.stack(np.divmod(np.asarray(lv["cell"], dtype=int), E), axis=1), "in_": _bits(lv["in_mask"], p),
                       "out_": _bits(lv["out_mask"], p), "u": np.array(lv["u"]), "lower": np.array(lv["lower"])}
    names = np.array(_STATUS, dtype=object)[status]
    return L0LocalProof(al, et, coefs, intercepts, np.array(out["objective"]).reshape(A, E), np.array(out["lower_bound"]).reshape(A, E),
                        np.array(out["nodes"]).reshape(A, E), np.array(out["rounds"]).reshape(A, E), names, certificate)
