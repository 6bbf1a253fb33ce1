"""The node batches of tests/test_l0_local_prove_gpu.py's comparison with the rule (tests/_l0_local_prove_reference.node_rule),
shared with tests/test_l0_local_prove_cpu.py, which runs the host twin on the same nodes.  The shapes are those at which the
kernel can go wrong: one column, the slot edges (63, 64, 65, 130), all sixteen slots (1024 columns on 40 rows), a rank-deficient
12 x 20 design with a zero column.  Every batch holds the five nodes that matter -- all FREE, all OUT, all IN, IN on the last
column and OUT on the first (at 12 x 20: IN on the zero column, which fails the pivot test), and states that differ across a
slot edge (bits 63 and 64, where there are that many columns) -- and random masks beside them, at eta in {0, 0.02, 1} and big_M
in {0.6, 100}; one batch runs a single sweep, and every batch but the first mixes the nodes of several cells."""

import functools

import numpy as np
from _l0_local_bound_cases import draw, var

SWEEPS = 40  # the cap of the cases: a node at eta = 0 under a loose box may end there, and is compared all the same
ETAS = (0.0, 0.02, 1.0)


def _nodes(p, n_cells, seed, extra=4, special=None):
    """[(cell, in_, out_, parent_lower, start or None)]: the named nodes, then ``extra`` random ones."""
    rng = np.random.default_rng(seed)
    none, every = np.zeros(p, dtype=bool), np.ones(p, dtype=bool)
    one_in, one_out = none.copy(), none.copy()
    one_in[p - 1 if special is None else special] = True
    one_out[0] = p > 1
    edge_in, edge_out = none.copy(), none.copy()
    if p > 64:
        edge_in[63], edge_out[64] = True, True
    else:
        edge_in[p - 1] = True
    nodes = [(none, none), (none, every), (every, none), (one_in, one_out), (edge_in, edge_out)]
    if p > 64:
        nodes.append((edge_out, edge_in))  # the edge the other way round
    for _ in range(extra):
        s = rng.choice(3, size=p, p=[0.6, 0.2, 0.2])
        nodes.append((s == 1, s == 2))
    out = []
    for i, (in_, out_) in enumerate(nodes):
        start = None if i % 3 == 0 else 0.8 * rng.uniform(-1.0, 1.0, p) * (rng.random(p) < 0.3)
        parent = -np.inf if i % 2 == 0 else -0.05 * (i + 1)  # (an odd node's parent bound is sometimes the better one)
        out.append((i % n_cells, in_.copy(), out_.copy(), parent, start))
    return out


def _cases():
    out = {}

    def add(name, X, y, cells, nodes, big_M=100.0, max_sweeps=SWEEPS, gap_tol=1e-8):
        cells = np.asarray(cells, dtype=float).reshape(-1, 2)
        X.setflags(write=False)
        y.setflags(write=False)
        out[name] = dict(X=X, y=y, alphas=cells[:, 0] * var(y), etas=cells[:, 1].copy(), big_M=big_M, nodes=nodes, max_sweeps=max_sweeps,
                         gap_tol=gap_tol)

    grid = [(0.01, 0.0), (0.05, 0.02), (0.02, 1.0)]
    X, y = draw(20, 1, 1, 0)
    add("p1", X, y, grid[:1], _nodes(1, 1, 1))
    add("p1_box", X, y, grid, _nodes(1, 3, 2), big_M=0.6)
    for p in (63, 64, 65, 130):
        X, y = draw(80, p, 6, p)
        add(f"slots{p}", X, y, grid, _nodes(p, 3, p))
        add(f"slots{p}_box", X, y, grid, _nodes(p, 3, p + 1), big_M=0.6)
    X, y = draw(80, 65, 6, 65)
    add("slots65_one_sweep", X, y, grid, _nodes(65, 3, 7), max_sweeps=1)
    X, y = draw(40, 1024, 16, 3, rho=0.0, noise=0.3, spread=True)
    add("p1024", X, y, [(0.02, 1.0), (0.002, 0.02)], _nodes(1024, 2, 9, extra=2), max_sweeps=3)
    rng = np.random.default_rng(5)
    X = rng.standard_normal((12, 20))
    X[:, 7] = 0.0
    y = X[:, 0] - X[:, 3] + X[:, 11] + 0.2 * rng.standard_normal(12)
    add("rank_deficient", X, y, grid, _nodes(20, 3, 11, special=7))
    add("rank_deficient_box", X, y, grid, _nodes(20, 3, 12, special=7), big_M=0.6)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return _cases()


def run_rule(G, c, k):
    """The rule on every node of case ``k`` with the Gram ``(G, c)``: a list of ``node_rule``'s dicts, ``lower`` with the parent's
    bound folded in (``own_lower``: without)."""
    from _l0_local_prove_reference import node_rule

    runs = []
    for cell, in_, out_, parent, start in k["nodes"]:
        r = node_rule(G, c, float(k["alphas"][cell]), float(k["etas"][cell]), k["big_M"], in_, out_, start=start, max_sweeps=k["max_sweeps"],
                      gap_tol=k["gap_tol"])
        r["own_lower"] = r["lower"]
        r["lower"] = max(r["lower"], parent)
        runs.append(r)
    return runs


@functools.lru_cache(maxsize=None)
def reference(name):
    """``(G, c, the rule's dicts)`` of case ``name`` on the numpy Gram: computed once per process and left unchanged."""
    from _l0_local_reference import gram

    k = cases()[name]
    G, c, _, _, _ = gram(k["X"], k["y"])
    G.setflags(write=False)
    c.setflags(write=False)
    return G, c, run_rule(G, c, k)
