"""The inputs of the local-subsets GPU tests (tests/test_l0_local_subsets_gpu.py) and, per (row set, cell), the numpy
restatement (tests/_l0_local_subsets_reference.py) run on the rows directly -- rows weighted and centred in numpy, no Gram of a
complement, no elimination.  The seeds were picked on the CPU so that the restatement's own decision margins stay at or above
1e-6 (tests/test_l0_local_subsets_cpu.py recomputes that premise for every case).

A case: ``X``, ``y``, ``sizes``, ``etas`` (one per cell), ``big_M``, ``starts`` (None or cells x S x p, shared by the row sets),
``swaps``, ``weights`` (one array of n row weights per row set, or [None]), ``intercept``.  What each is there for:

  one_column      p = 1; k = 1 and k above p
  p63 p64 p65     the slot boundary in the shrink arg-min and the grow arg-max; k = 1; a start of 10 columns with one in the LAST
                  column (at p = 65 alone in the second slot: the surplus sits in another slot than what stays) that is shrunk
                  for k < 10 and grown for k = 12
  p130            three slots, ld = 144 != p; eta > 0 in one cell
  p1024           one true column per 64-block, all sixteen slots live in every scan; n = 120 < p with eta > 0 in one cell
  dead_column     k >= p with an all-zero column: the grow stops at the live ones
  box             a binding box
  ridge_wide      eta > 0 with n = 20 < p = 40, a size above n
  greedy          swaps = 0 on the hard law
  hard_swaps      the hard law, accepted swaps in every problem
  second_start    the hard law where the zero start misses the optimum: a second start wins
  sixteen_sets    16 row sets with weights that are not masks, an intercept
  intercept       four row sets (three folds' rows and all rows), an intercept, weights
"""

import functools

import numpy as np

from _l0_local_reference import gram, hard_law
from _l0_local_subsets_reference import best_subset, solve_cells

NAMES = ("one_column", "p63", "p64", "p65", "p130", "p1024", "dead_column", "box", "ridge_wide", "greedy", "hard_swaps", "second_start",
         "sixteen_sets", "intercept")


def _draw(n, p, k, seed, rho=0.5, noise=0.5, spread=False):
    """n x p AR(1) columns, k true columns with coefficients +-1 (``spread``: one in every block of 64 columns)."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, p))
    X = Z.copy()
    for j in range(1, p):
        X[:, j] = rho * X[:, j - 1] + np.sqrt(1.0 - rho * rho) * Z[:, j]
    beta = np.zeros(p)
    cols = 64 * np.arange(k) + rng.integers(0, 64, k) if spread else rng.choice(p, min(k, p), replace=False)
    beta[cols] = (-1.0) ** np.arange(len(cols))
    return X, X @ beta + noise * rng.standard_normal(n)


def _ten_column_start(p, cells, seed):
    """Per cell: the zero start and a start of 10 columns, the last column among them."""
    rng = np.random.default_rng(seed)
    start = np.zeros(p)
    start[np.r_[rng.choice(p - 1, 9, replace=False), p - 1]] = rng.uniform(0.2, 0.8, 10) * rng.choice([-1.0, 1.0], 10)
    return np.broadcast_to(np.stack([np.zeros(p), start]), (cells, 2, p)).copy()


@functools.lru_cache(maxsize=None)
def case(name):
    out = {"big_M": 100.0, "starts": None, "swaps": True, "weights": [None], "intercept": False}
    if name == "one_column":
        X, y = _draw(20, 1, 1, 0)
        out.update(sizes=[1, 3], etas=[0.0, 0.1])
    elif name in ("p63", "p64", "p65"):
        p = int(name[1:])
        X, y = _draw(40, p, 5, p)
        out.update(sizes=[1, 3, 6, 12], etas=[0.0, 0.0, 0.01, 0.0], starts=_ten_column_start(p, 4, p))
    elif name == "p130":
        X, y = _draw(60, 130, 7, 130)
        start = _ten_column_start(130, 3, 130)
        start[:, 1, [5, 70]] = 0.3  # (twelve columns over the three slots)
        out.update(sizes=[2, 5, 9], etas=[0.0, 0.02, 0.0], starts=start)
    elif name == "p1024":
        X, y = _draw(120, 1024, 16, 1024, spread=True)
        out.update(sizes=[4, 16, 20], etas=[0.0, 0.0, 0.05])
    elif name == "dead_column":
        X, y = _draw(30, 12, 4, 12)
        X[:, 5] = 0.0
        out.update(sizes=[12, 40], etas=[0.0, 0.0])
    elif name == "box":
        X, y = _draw(40, 20, 5, 20)
        out.update(sizes=[2, 4, 7], etas=[0.0, 0.0, 0.0], big_M=0.4)
    elif name == "ridge_wide":
        X, y = _draw(20, 40, 5, 40)
        out.update(sizes=[5, 25], etas=[0.05, 0.05])
    elif name == "greedy":
        X, y = hard_law(4)
        out.update(sizes=[2, 3, 5], etas=[0.0, 0.0, 0.0], swaps=False)
    elif name == "hard_swaps":
        X, y = hard_law(20)
        out.update(sizes=[2, 4, 5], etas=[0.0, 0.0, 0.0])
    elif name == "second_start":
        X, y = hard_law(SECOND_START[0])
        out.update(sizes=list(SECOND_START[1]), etas=[0.0] * len(SECOND_START[1]))
        G, c, _, _, _ = gram(X, y)
        starts = np.zeros((len(SECOND_START[1]), 2, 14))
        for e, k in enumerate(SECOND_START[1]):
            starts[e, 1] = _optimum(G, c, k)
        out.update(starts=starts)
    elif name == "sixteen_sets":
        X, y = _draw(50, 6, 3, 6)
        X, y = X + 1.5, y - 2.0
        rng = np.random.default_rng(16)
        out.update(sizes=[1, 3], etas=[0.0, 0.0], weights=[rng.uniform(0.2, 2.0, 50) for _ in range(16)], intercept=True)
    elif name == "intercept":
        X, y = _draw(60, 18, 4, 18)
        X, y = X + 3.0, y + 5.0
        w = np.random.default_rng(2).uniform(0.2, 2.0, 60)
        weights = []
        for lo in (0, 20, 40, None):
            m = w.copy()
            if lo is not None:
                m[lo:lo + 20] = 0.0
            weights.append(m)
        out.update(sizes=[2, 4, 6], etas=[0.0, 0.01, 0.0], weights=weights, intercept=True)
    else:
        raise KeyError(name)
    for a in (X, y):
        a.setflags(write=False)
    out.update(X=X, y=y)
    return out


SECOND_START = (2, (3, 4))  # (hard-law seed, sizes): the full rule from zero stays above the optimum there


def _optimum(G, c, k):
    """The coefficients of the best subset of exactly the size the enumeration finds for <= k."""
    from itertools import combinations

    best, at = 0.0, None
    for m in range(1, k + 1):
        for S in combinations(range(len(c)), m):
            S = list(S)
            b = np.linalg.solve(G[np.ix_(S, S)], c[S])
            if -0.5 * c[S] @ b < best:
                best, at = -0.5 * c[S] @ b, (S, b)
    beta = np.zeros(len(c))
    beta[at[0]] = at[1]
    assert abs(best - best_subset(G, c, k)) <= 1e-12 * abs(best)
    return beta


def row_sets(c):
    """``(row_weights, n_effs)`` as the engine takes them: each set's weights scaled to sum to the rows that carry weight."""
    n = c["X"].shape[0]
    weights, n_effs = [], []
    for w in c["weights"]:
        if w is None:
            weights.append(None)
            n_effs.append(0)
            continue
        rows = int(np.count_nonzero(w))
        weights.append(w * (rows / w.sum()))
        n_effs.append(rows)
    return weights, n_effs, n


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per row set, per cell: the dict of ``_l0_local_subsets_reference.solve_cells`` on the weighted rows, with ``intercept``."""
    c = case(name)
    out = []
    for w in c["weights"]:
        rows = np.arange(c["X"].shape[0]) if w is None else np.flatnonzero(w)
        sw = None if w is None else w[rows]
        G, cv, yy, x_mean, y_mean = gram(c["X"][rows], c["y"][rows], sw, c["intercept"])
        cells = solve_cells(G, cv, yy, c["sizes"], c["etas"], c["big_M"], c["starts"], c["swaps"])
        for cell in cells:
            cell["c"], cell["yy"] = cv, yy
            cell["intercept"] = float(y_mean - x_mean @ cell["beta"])
        out.append(cells)
    return out
