"""The node batches that tests/test_l0_local_group_prove_cpu.py (the host twin) and tests/test_l0_local_group_prove_gpu.py (the
kernel) both run through the numpy restatement of the group node rule: the widths at which the kernel changes path (2, 63, 64,
65, 130, 1024 columns; groups that straddle lanes 63 / 64; one group of 70 columns; a rank-deficient 12 x 20 design in groups of
four with a zero column) and the node states (all FREE, all IN, all OUT, closed mixtures under a chain, IN on a failed pivot,
one sweep).  A case: ``X``, ``y``, ``gstart``, ``need`` (direct lists or None), ``alphas``, ``etas``, ``big_M``, ``max_sweeps``,
``gap_tol`` and ``nodes``: [(cell, gin, gout, parent lower, start or None)]."""

import functools

import numpy as np

from _l0_local_groups_reference import close_hierarchy
from _l0_local_group_prove_reference import node_rule


def _draw(seed, n, p, rho=0.6):
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, p))
    X = Z.copy()
    for j in range(1, p):
        X[:, j] = rho * X[:, j - 1] + np.sqrt(1.0 - rho * rho) * Z[:, j]
    beta = np.zeros(p)
    beta[rng.choice(p, max(1, p // 8), replace=False)] = rng.choice([-1.0, 1.0], max(1, p // 8))
    y = X @ beta + 0.5 * rng.standard_normal(n)
    return X, y


def _chain(ng):
    return [[]] + [[g - 1] for g in range(1, ng)]


def _nodes(ng, p, n_cells, rng, chained, big_M):
    """All FREE, all IN, all OUT, then closed mixtures: under a chain IN is a prefix and OUT a suffix."""
    none, every = np.zeros(ng, dtype=bool), np.ones(ng, dtype=bool)
    nodes = [(0, none, none, -np.inf, None), (n_cells - 1, every, none, -0.5, None), (0, none, every, -np.inf, None)]
    for k in range(3):
        gin, gout = none.copy(), none.copy()
        if chained:
            gin[: rng.integers(0, ng // 2 + 1)] = True
            gout[ng - rng.integers(0, ng // 2 + 1):] = True
        else:
            state = rng.integers(0, 3, ng)
            gin, gout = state == 1, state == 2
        start = rng.uniform(-1.5, 1.5, p) * (rng.random(p) < 0.5) if k else None  # (some beyond a small box: clipped)
        nodes.append((k % n_cells, gin, gout & ~gin, -np.inf if k else -1e-3, start))
    return nodes


@functools.lru_cache(maxsize=None)
def cases():
    out = {}

    def add(name, seed, n, p, gstart, chained, alphas, etas, big_M, max_sweeps, few=False):
        X, y = _draw(seed, n, p)
        gstart = np.asarray(gstart, dtype=int)
        ng = len(gstart) - 1
        rng = np.random.default_rng(100 + seed)
        nodes = _nodes(ng, p, len(alphas), rng, chained, big_M)
        out[name] = dict(X=X, y=y, gstart=gstart, need=_chain(ng) if chained else None, alphas=np.array(alphas, dtype=float),
                         etas=np.array(etas, dtype=float), big_M=big_M, max_sweeps=max_sweeps, gap_tol=1e-8, nodes=nodes[:3] if few else nodes)

    add("p2_one_group", 1, 20, 2, [0, 2], False, [0.05, 0.3], [0.02, 0.0], 100.0, 200)
    add("p63_threes", 2, 80, 63, np.arange(0, 64, 3), True, [0.02, 0.2], [0.05, 0.0], 100.0, 12)
    add("p64_fours_tight_box", 3, 80, 64, np.arange(0, 65, 4), False, [0.02, 0.2], [0.05, 1.0], 0.7, 12)
    add("p65_straddle", 4, 80, 65, list(range(0, 61, 5)) + [65], True, [0.02, 0.2], [0.0, 0.05], 100.0, 12)  # the last group: columns 60 .. 64
    add("p70_one_group", 5, 90, 70, [0, 70], False, [0.5, 3.0], [0.05, 0.0], 100.0, 10)
    add("p130_sevens", 6, 100, 130, list(range(0, 127, 7)) + [130], False, [0.05, 0.4], [0.02, 0.0], 100.0, 6)  # columns 63 .. 69 are one group
    add("p1024_fours_one_sweep", 7, 64, 1024, np.arange(0, 1025, 4), False, [0.3], [0.1], 100.0, 1, few=True)
    # rank-deficient: 12 rows, 20 columns in groups of four, column 7 zero (a failed pivot inside an IN group and inside a FREE one)
    X, y = _draw(8, 12, 20)
    X[:, 7] = 0.0
    ng, none, every = 5, np.zeros(5, dtype=bool), np.ones(5, dtype=bool)
    one = none.copy()
    one[1] = True
    out["rank_deficient_fours"] = dict(
        X=X, y=y, gstart=np.arange(0, 21, 4), need=None, alphas=np.array([0.01, 0.2]), etas=np.array([0.0, 0.05]), big_M=100.0, max_sweeps=40,
        gap_tol=1e-8, nodes=[(0, none, none, -np.inf, None), (1, every, none, -np.inf, None), (0, one, none, -np.inf, None),
                             (1, one, ~one, -np.inf, None), (0, none, one, -0.2, np.full(20, 0.3)), (1, none, none, -np.inf, None)])
    out["one_sweep"] = dict(out["p63_threes"], max_sweeps=1)
    return out


def run_rule(G, c, k):
    """The restatement on every node of a case (one lockstep batch): a list of dicts per node, ``lower`` with the parent's bound
    folded in and ``own_lower`` without."""
    ng = len(k["gstart"]) - 1
    closed = close_hierarchy(ng, k["need"])
    cell = [n[0] for n in k["nodes"]]
    p = len(c)
    starts = np.stack([np.zeros(p) if n[4] is None else n[4] for n in k["nodes"]])
    r = node_rule(G, c, k["big_M"], k["gstart"], closed, k["alphas"][cell], k["etas"][cell], np.stack([n[1] for n in k["nodes"]]),
                  np.stack([n[2] for n in k["nodes"]]), starts, max_sweeps=k["max_sweeps"], gap_tol=k["gap_tol"])
    return [dict(u=r["u"][i], own_lower=float(r["lower"][i]), lower=max(float(r["lower"][i]), n[3]), primal=float(r["primal"][i]),
                 upper=float(r["upper"][i]), sweeps=int(r["sweeps"][i]), status=int(r["status"][i])) for i, n in enumerate(k["nodes"])]
