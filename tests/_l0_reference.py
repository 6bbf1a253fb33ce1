"""Brute-force reference for the exact l0 estimators: every admissible support, solved straight from X in numpy.

The problem (sparselm_amd/model/_miqp.py; the reference's objectives divided by 2n):

    minimise over supports S (sets of groups) and beta, supp beta in cols(S), |beta_j| <= big_M:
        1/(2n) ||X beta - y||^2 - 1/(2n) ||y||^2 + eta ||W beta||^2 + alpha |S|
    subject to |S| <= K  and  i in S => hierarchy[i] in S

Per support: ``numpy.linalg.lstsq`` on the columns of the support; where that solution leaves the box,
``scipy.optimize.lsq_linear`` (BVLS, an exact active-set method) inside it -- an unconstrained minimiser inside the box is
the boxed one, so the second call is only made where it can differ.  The ridge term goes in by row augmentation
(``sqrt(2 n eta) W`` under X, zeros under y).  Hierarchy and cardinality by filtering.  Nothing here forms a Gram matrix
to solve with: the engine's route (Cholesky on X^T X / n) is what is being checked.

``brute_force`` also returns the relative gap between the best and the second-best support and the condition number of
the winner's Gram block: the comparison tests assert on those first, so that "the same support" and "the same
coefficients to 1e-9" are well-posed questions.

For problems too wide to enumerate in full, ``brute_force(..., max_size=S)`` stops at supports of S groups and returns
``closed``: whether the reference's own numbers prove that no larger support can win.  ``search_rank`` restates the
engine's documented search order (csrc/l0_kernels.hpp) from X, so that a test can assert that its winner lies where it is
meant to lie in the search tree; it is used for premises only.
"""

from __future__ import annotations

import itertools

import numpy as np
from scipy.optimize import lsq_linear


def group_columns(groups, p):
    """(sorted labels, list of column index arrays, one per sorted label)"""
    labels = np.arange(p) if groups is None else np.asarray(groups)
    uniq = np.unique(labels)
    return uniq, [np.flatnonzero(labels == u) for u in uniq]


def augmented(X, y, eta=0.0, W=None):
    """(Xa, ya): 1/(2n)||Xa b - ya||^2 = 1/(2n)||X b - y||^2 + eta ||W b||^2 (n the rows of X)."""
    X = np.asarray(X, dtype=float)
    y = np.asarray(y, dtype=float)
    n, p = X.shape
    if eta == 0.0:
        return X, y
    W = np.eye(p) if W is None else np.asarray(W, dtype=float)
    return np.vstack([X, np.sqrt(2.0 * n * eta) * W]), np.concatenate([y, np.zeros(W.shape[0])])


def solve_support(Xa, ya, cols, big_M=np.inf):
    """The minimiser of ||Xa[:, cols] b - ya||^2 inside the box, and that squared norm."""
    if len(cols) == 0:
        return np.zeros(0), float(ya @ ya)
    A = Xa[:, cols]
    b = np.linalg.lstsq(A, ya, rcond=None)[0]
    if np.max(np.abs(b)) > big_M:
        b = lsq_linear(A, ya, bounds=(-big_M, big_M), method="bvls", tol=1e-15, max_iter=10 * len(cols) + 100).x
    r = A @ b - ya
    return b, float(r @ r)


def objective_of(X, y, coef, n_active, alpha=0.0, eta=0.0, W=None):
    """The objective above for given coefficients (straight from X)."""
    Xa, ya = augmented(X, y, eta, W)
    n = np.asarray(X).shape[0]
    r = Xa @ coef - ya
    return float((r @ r - ya @ ya) / (2.0 * n) + alpha * n_active)


def search_rank(X, y, groups=None, eta=0.0, W=None):
    """The position of every group (by sorted label) in the engine's search order, as csrc/l0_kernels.hpp documents it:
    groups by descending ``||c_g||^2 / tr G_gg`` with ``G = X^T X / n`` and ``c = X^T y / n``, ties to the lower sorted
    label; a group whose trace is zero scores zero.  The documented denominator is the trace of the data's Gram block: the
    ridge term ``2 eta W^T W`` that the search adds to it does not enter the order, so ``eta`` and ``W`` are accepted (a
    call can pass a problem's arguments whole) and leave the result unchanged."""
    del eta, W
    X = np.asarray(X, dtype=float)
    y = np.asarray(y, dtype=float)
    n, p = X.shape
    _, gcols = group_columns(groups, p)
    c = X.T @ y / n
    diag = np.einsum("ij,ij->j", X, X) / n
    score = np.zeros(len(gcols))
    for g, cols in enumerate(gcols):
        den = float(np.sum(diag[cols]))
        score[g] = float(np.sum(c[cols] ** 2)) / den if den > 0.0 else 0.0
    order = np.argsort(-score, kind="stable")  # (stable: ties keep the lower sorted label first)
    rank = np.empty(len(gcols), dtype=int)
    rank[order] = np.arange(len(gcols))
    return rank


def brute_force(X, y, groups=None, K=None, alpha=0.0, eta=0.0, W=None, big_M=np.inf, hierarchy=None, max_size=None):
    """The optimum over all admissible supports.  Returns a dict: ``active`` (bool per sorted label), ``coef``,
    ``objective``, ``gap`` (relative, to the second-best support), ``kappa`` (condition number of the winner's block of
    Xa^T Xa), ``n_supports``, ``closed``.

    ``max_size=S`` enumerates supports of at most S groups only.  ``closed`` then says whether that was enough:
    ``q_all_ref + alpha (S + 1) > objective``, with ``q_all_ref`` the unboxed ``lstsq`` value on ALL columns.  The quadratic
    part is monotone in the support (and the box can only raise it), so every support of more than S groups costs at
    least the left-hand side and cannot win -- nor can it be the second best, unless the gap is that wide, so ``gap`` is
    then capped by the distance to that bound.  Without ``max_size``, or when S reaches the bound K, everything admissible
    was enumerated and ``closed`` is True."""
    X = np.asarray(X, dtype=float)
    y = np.asarray(y, dtype=float)
    n, p = X.shape
    uniq, gcols = group_columns(groups, p)
    G = len(uniq)
    K = G if K is None else int(min(K, G))
    S_max = K if max_size is None else int(min(max_size, K))
    index = {u.item(): i for i, u in enumerate(uniq)}
    need = [set() for _ in range(G)]
    if hierarchy is not None:
        assert len(hierarchy) == G
        need = [{index[np.asarray(lab).item()] for lab in subs} for subs in hierarchy]
    Xa, ya = augmented(X, y, eta, W)
    yy = float(ya @ ya)
    best = (np.inf, None, None)
    second = np.inf
    count = 0
    for size in range(S_max + 1):
        for S in itertools.combinations(range(G), size):
            chosen = set(S)
            if any(not need[i] <= chosen for i in S):
                continue
            count += 1
            cols = np.concatenate([gcols[i] for i in S]).astype(int) if S else np.zeros(0, dtype=int)
            b, rss = solve_support(Xa, ya, cols, big_M)
            obj = (rss - yy) / (2.0 * n) + alpha * size
            if obj < best[0]:
                second = best[0]
                best = (obj, S, (cols, b))
            elif obj < second:
                second = obj
    obj, S, (cols, b) = best
    coef = np.zeros(p)
    coef[cols] = b
    active = np.zeros(G, dtype=bool)
    active[list(S)] = True
    scale = abs(obj) if obj != 0.0 else yy / (2.0 * n)
    closed = True
    if S_max < K:
        r_all = Xa @ np.linalg.lstsq(Xa, ya, rcond=None)[0] - ya
        floor = (float(r_all @ r_all) - yy) / (2.0 * n) + alpha * (S_max + 1)  # no support of more than S_max groups is below this
        closed = bool(floor > obj)
        second = min(second, floor)
    kappa = 1.0
    if len(cols):
        sv = np.linalg.svd(Xa[:, cols], compute_uv=False)
        kappa = float((sv[0] / sv[-1]) ** 2) if sv[-1] > 0 else np.inf
    return {"active": active, "coef": coef, "objective": float(obj), "gap": float((second - obj) / scale) if np.isfinite(second) else np.inf,
            "kappa": kappa, "n_supports": count, "closed": closed}


def forward_stepwise(X, y, K):
    """Greedy forward selection of K single columns by residual sum of squares: (columns, rss)."""
    X = np.asarray(X, dtype=float)
    chosen = []
    rss = float(y @ y)
    for _ in range(K):
        cand = [(solve_support(X, y, np.array(chosen + [j]))[1], j) for j in range(X.shape[1]) if j not in chosen]
        rss, j = min(cand)
        chosen.append(j)
    return sorted(chosen), rss
