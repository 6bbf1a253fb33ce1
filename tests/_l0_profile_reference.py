"""Brute-force reference for the exact l0 PROFILE (``sparselm_amd.miqp.l0_profile``): for every size k the best and the
second-best admissible support of EXACTLY k groups, every support solved straight from X by the functions of
tests/_l0_reference.py (``lstsq``, BVLS inside the box, the ridge term by row augmentation -- no Gram matrix).

``profile_table`` returns, per size k = 0 .. K: ``values`` (the objective of _l0_reference without its ``alpha |S|`` term;
``+inf`` where the hierarchy admits no support of that size), ``seconds`` (the runner-up of that size), ``gaps`` (relative,
as ``brute_force`` reports its gap; ``inf`` where a size has one support only), ``actives`` (bool per sorted group label),
``coefs``, ``kappas`` (condition number of the winner's block) and ``n_supports``.  The comparison tests assert on gaps and
kappas first, so that "the same support" and "the same coefficients to 1e-9" are well-posed questions at every size.

``best_subset_of`` and ``regularized_of`` read the two answers off the table (ties to the smaller size); ``envelope_sizes``
gives the sizes on the lower convex envelope of the values, i.e. the sizes some ``alpha > 0`` makes optimal.
"""

from __future__ import annotations

import itertools

import numpy as np

from _l0_reference import augmented, group_columns, solve_support


def profile_table(X, y, groups=None, K=None, eta=0.0, W=None, big_M=np.inf, hierarchy=None):
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
    Xa, ya = augmented(X, y, eta, W)
    yy = float(ya @ ya)
    values, seconds = np.full(K + 1, np.inf), np.full(K + 1, np.inf)
    actives, coefs, kappas = np.zeros((K + 1, G), dtype=bool), np.zeros((K + 1, p)), np.ones(K + 1)
    count = 0
    for size in range(K + 1):
        best = None
        for S in itertools.combinations(range(G), size):
            chosen = set(S)
            if any(not need[i] <= chosen for i in S):
                continue
            count += 1
            cols = np.concatenate([gcols[i] for i in S]).astype(int) if S else np.zeros(0, dtype=int)
            b, rss = solve_support(Xa, ya, cols, big_M)
            obj = (rss - yy) / (2.0 * n)
            if obj < values[size]:
                seconds[size] = values[size]
                values[size] = obj
                best = (S, cols, b)
            elif obj < seconds[size]:
                seconds[size] = obj
        if best is None:
            continue
        S, cols, b = best
        actives[size, list(S)] = True
        coefs[size, cols] = b
        if len(cols):
            sv = np.linalg.svd(Xa[:, cols], compute_uv=False)
            kappas[size] = float((sv[0] / sv[-1]) ** 2) if sv[-1] > 0 else np.inf
    scale = np.where(values != 0.0, np.abs(values), yy / (2.0 * n))
    with np.errstate(invalid="ignore"):
        gaps = np.where(np.isfinite(seconds), (seconds - values) / scale, np.inf)
    return {"values": values, "seconds": seconds, "gaps": gaps, "actives": actives, "coefs": coefs, "kappas": kappas,
            "n_supports": count}


def best_subset_of(table, bound):
    """The size of the best support of at most ``bound`` groups (ties to the smaller size)."""
    return int(np.argmin(table["values"][: bound + 1]))


def regularized_of(table, alpha):
    """The size minimising ``values[k] + alpha k`` (ties to the smaller size)."""
    v = table["values"]
    return int(np.argmin(v + alpha * np.arange(len(v))))


def envelope_sizes(values):
    """The sizes on the lower convex envelope of (k, values[k]) from size 0 down to the overall minimum: a size is on it iff
    some alpha > 0 makes it the unique minimiser of values[k] + alpha k.  By definition, not by a hull algorithm: size k is
    kept iff no pair a < k < b has the chord from a to b at or below values[k], and no smaller size is at or below it."""
    v = np.asarray(values, dtype=float)
    finite = [int(k) for k in np.flatnonzero(np.isfinite(v))]
    out = []
    for k in finite:
        if any(v[a] <= v[k] for a in finite if a < k):
            continue  # a smaller size is as good: never optimal at a positive alpha
        under = any(v[a] + (v[b] - v[a]) * (k - a) / (b - a) <= v[k] for a in finite for b in finite if a < k < b)
        if not under:
            out.append(k)
    return out
