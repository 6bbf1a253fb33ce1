"""Brute-force reference for the L1L0 PROFILE (``sparselm_amd.miqp.l1l0_profile``): for every size k the best and the
second-best admissible support of EXACTLY k groups under an l1 term, every support solved straight from X by
``solve_support_l1`` of tests/_l1l0_reference.py (a lasso per support, then an exact solve on its sign pattern -- no Gram
matrix), with the KKT residual of every solution asserted as ``brute_force_l1`` asserts it.

``profile_table_l1`` returns what ``_l0_profile_reference.profile_table`` returns, per size k = 0 .. K: ``values`` (the lasso
value of the best support, without an ``alpha |S|`` term; ``+inf`` where the hierarchy admits no support of that size),
``seconds``, ``gaps`` (relative; ``inf`` where a size has one support only), ``actives`` (bool per sorted group label),
``coefs``, ``kappas`` (condition number of the winner's NON-ZERO columns, as ``brute_force_l1`` reports it), ``n_supports`` and
``kkt`` (the largest residual met).

Under an l1 term the table saturates: once a size holds every column the lasso on all columns uses, every larger size ties
with it, its gap is 0 and its support is not unique.  The tests compare such rows by value only.
"""

from __future__ import annotations

import itertools

import numpy as np

from _l0_reference import group_columns
from _l1l0_reference import KKT_RTOL, solve_support_l1


def profile_table_l1(X, y, groups=None, K=None, eta=0.0, big_M=np.inf, hierarchy=None):
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
        need = [{index[np.asarray(lab).item()] for lab in subs} for subs in hierarchy]
    c_inf = float(np.max(np.abs(X.T @ y / n)))
    yy = float(y @ y)
    values, seconds = np.full(K + 1, np.inf), np.full(K + 1, np.inf)
    actives, coefs, kappas = np.zeros((K + 1, G), dtype=bool), np.zeros((K + 1, p)), np.ones(K + 1)
    count = 0
    worst_kkt = 0.0
    for size in range(K + 1):
        best = None
        for S in itertools.combinations(range(G), size):
            chosen = set(S)
            if any(not need[i] <= chosen for i in S):
                continue
            count += 1
            cols = np.concatenate([gcols[i] for i in S]).astype(int) if S else np.zeros(0, dtype=int)
            b, value, kkt = solve_support_l1(X, y, cols, eta, big_M)
            assert kkt <= KKT_RTOL * c_inf, f"support {S}: KKT residual {kkt:.3e} > {KKT_RTOL:g} * {c_inf:.3e}"
            worst_kkt = max(worst_kkt, kkt)
            if value < values[size]:
                seconds[size] = values[size]
                values[size] = value
                best = (S, cols, b)
            elif value < seconds[size]:
                seconds[size] = value
        if best is None:
            continue
        S, cols, b = best
        actives[size, list(S)] = True
        coefs[size, cols] = b
        nz = np.flatnonzero(coefs[size])
        if len(nz):
            sv = np.linalg.svd(X[:, nz], compute_uv=False)
            kappas[size] = float((sv[0] / sv[-1]) ** 2) if sv[-1] > 0 else np.inf
    scale = np.where(values != 0.0, np.abs(values), yy / (2.0 * n))
    with np.errstate(invalid="ignore"):
        gaps = np.where(np.isfinite(seconds), (seconds - values) / scale, np.inf)
    return {"values": values, "seconds": seconds, "gaps": gaps, "actives": actives, "coefs": coefs, "kappas": kappas,
            "n_supports": count, "kkt": worst_kkt}
