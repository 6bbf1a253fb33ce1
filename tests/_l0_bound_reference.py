"""A sequential restatement of the exact l0 search with the exclusion bound, for problems too wide for ``brute_force``.

The search of csrc/l0_kernels.hpp in numpy, one node at a time: groups in the documented search order (``search_rank``),
depth first, include before exclude; a node's value comes from X by ``lstsq`` (``solve_support`` of ``_l0_reference``: the
box by BVLS where it binds); the hierarchy and the cardinality bound by the kernel's rules.  The subtree below a node of
``cnt`` groups with the groups E excluded is cut when

    q(all \\ E) + alpha (cnt + 1) >= incumbent,

with ``q(all \\ E)`` computed DIRECTLY -- a solve on the Gram block of every column outside E -- and not through ``P = H^-1`` as
the engine does it: the two routes to the same number are what the GPU tests compare.  The incumbent starts from a greedy
forward selection, as the engine's does.  Returns the optimum and ``nodes``, the include attempts that passed the hierarchy
(the engine's count; pruning depends on when an incumbent is met, so the two counts agree in size, not digit for digit).
"""

from __future__ import annotations

import numpy as np
from scipy.linalg import cho_factor, cho_solve

from _l0_reference import augmented, group_columns, search_rank, solve_support


def bounded_search(X, y, groups=None, K=None, alpha=0.0, eta=0.0, W=None, big_M=np.inf, hierarchy=None, bound="exclusion",
                   max_nodes=10**7):
    """dict: ``active`` (bool per sorted label), ``coef``, ``objective``, ``nodes``, ``finished``.  ``bound="q_all"`` is the
    plain search (the value on all columns, whatever was excluded) for node counts to compare with."""
    X = np.asarray(X, dtype=float)
    y = np.asarray(y, dtype=float)
    n, p = X.shape
    uniq, gcols = group_columns(groups, p)
    G = len(uniq)
    K = G if K is None else int(min(K, G))
    index = {u.item(): i for i, u in enumerate(uniq)}
    need = [set() for _ in range(G)]
    if hierarchy is not None:
        assert len(hierarchy) == G
        need = [{index[np.asarray(lab).item()] for lab in subs} - {i} for i, subs in enumerate(hierarchy)]
    Xa, ya = augmented(X, y, eta, W)
    yy = float(ya @ ya)
    order = np.argsort(search_rank(X, y, groups=groups), kind="stable")  # order[k]: the group at search position k

    def value(S):  # the objective of the support S (a list of groups), and its coefficients
        cols = np.concatenate([gcols[i] for i in S]).astype(int) if S else np.zeros(0, dtype=int)
        b, rss = solve_support(Xa, ya, cols, big_M)
        return (rss - yy) / (2.0 * n) + alpha * len(S), cols, b

    Ga, ca = Xa.T @ Xa / n, Xa.T @ ya / n

    def q_rest(excluded):  # q on every column outside the excluded groups, unboxed: -1/2 c_R^T (G_RR)^-1 c_R, lstsq where G_RR is singular
        cols = [gcols[i] for i in range(G) if i not in excluded]
        if not cols:
            return 0.0
        R = np.concatenate(cols).astype(int)
        try:
            q = -0.5 * float(ca[R] @ cho_solve(cho_factor(Ga[np.ix_(R, R)]), ca[R]))
        except np.linalg.LinAlgError:
            r = Xa[:, R] @ np.linalg.lstsq(Xa[:, R], ya, rcond=None)[0] - ya
            q = (float(r @ r) - yy) / (2.0 * n)
        return q - 1e-9 * abs(q)

    q_all = q_rest(set())
    best = {"obj": 0.0, "S": [], "cols": np.zeros(0, dtype=int), "b": np.zeros(0)}

    def offer(S):
        if any(not need[i] <= set(S) for i in S):
            return
        obj, cols, b = value(S)
        if obj < best["obj"]:
            best.update(obj=obj, S=list(S), cols=cols, b=b)

    # the greedy seed: forward selection over the groups whose needs are met
    cur = []
    for _ in range(K):
        cand = [(value(cur + [g])[0], g) for g in range(G) if g not in cur and need[g] <= set(cur)]
        if not cand:
            break
        cur = cur + [min(cand)[1]]
        offer(cur)
    state = {"nodes": 0, "finished": True}

    def walk(depth, included, excluded):
        cnt = len(included)
        if depth >= G or cnt >= K:
            return
        floor = q_rest(excluded) if bound == "exclusion" else q_all
        if not floor + alpha * (cnt + 1) < best["obj"]:
            return
        if state["nodes"] >= max_nodes:
            state["finished"] = False
            return
        g = int(order[depth])
        if not (need[g] & excluded):  # the hierarchy: it needs a group that was excluded
            state["nodes"] += 1
            offer(included + [g])
            walk(depth + 1, included + [g], excluded)
        if not any(g in need[i] for i in included):  # an included group needs this one: no exclude branch
            walk(depth + 1, included, excluded | {g})

    walk(0, [], set())
    coef = np.zeros(p)
    coef[best["cols"]] = best["b"]
    active = np.zeros(G, dtype=bool)
    active[best["S"]] = True
    return {"active": active, "coef": coef, "objective": float(best["obj"]), "nodes": state["nodes"], "finished": state["finished"]}
