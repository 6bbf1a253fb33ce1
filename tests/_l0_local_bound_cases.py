"""The problems of tests/test_l0_local_bound_gpu.py's comparison with the rule (tests/_l0_local_bound_reference.rule), shared with
tests/test_l0_local_bound_cpu.py, which runs the host twin on the same cells.  The shapes are those at which the kernel can go
wrong: one column, the slot edges (63, 64, 65, 130), all sixteen slots (1024 columns on 40 rows), a rank-deficient 12 x 20 design
with a zero column (a column the descent never touches is still counted in the sum), a box that binds, eta = 0, alpha = 0, a
start outside the box, and a single sweep."""

import functools

import numpy as np

SWEEPS = 200  # the cap of the cases: a cell at eta = 0 under a loose box may end there, and is compared all the same


def draw(n, p, k, seed, rho=0.5, noise=0.5, spread=False):
    """n x p AR(1) columns, k true columns (at most p) with coefficients +-1 (``spread``: one in every block of 64 columns): the
    law of the local search's own GPU cases, stated here so that this helper imports no test module."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, p))
    X = Z.copy()
    for j in range(1, p):
        X[:, j] = rho * X[:, j - 1] + np.sqrt(1.0 - rho * rho) * Z[:, j]
    beta = np.zeros(p)
    cols = 64 * np.arange(k) + rng.integers(0, 64, k) if spread else rng.choice(p, min(k, p), replace=False)
    beta[cols] = (-1.0) ** np.arange(len(cols))
    y = X @ beta + noise * rng.standard_normal(n)
    return X, y


def var(y):
    return float(np.var(y))


def _cases():
    out = {}

    def add(name, X, y, cells, big_M=100.0, starts=None, max_sweeps=SWEEPS, gap_tol=1e-9):
        cells = np.asarray(cells, dtype=float).reshape(-1, 2)
        X.setflags(write=False)
        y.setflags(write=False)
        out[name] = dict(X=X, y=y, alphas=cells[:, 0] * var(y), etas=cells[:, 1].copy(), big_M=big_M, starts=starts, max_sweeps=max_sweeps,
                         gap_tol=gap_tol)

    grid = [(0.01, 0.0), (0.05, 0.02), (0.3, 0.5), (0.0, 0.1), (0.02, 1.0)]
    X, y = draw(20, 1, 1, 0)
    add("p1", X, y, grid)
    add("p1_box", X, y, grid, big_M=0.3)
    for p in (63, 64, 65, 130):
        X, y = draw(80, p, 6, p)
        add(f"slots{p}", X, y, grid)
        add(f"slots{p}_box", X, y, grid, big_M=0.6)
    rng = np.random.default_rng(5)
    X, y = draw(80, 65, 6, 65)
    add("slots65_start_outside_the_box", X, y, grid, big_M=0.6, starts=3.0 * rng.uniform(-1.0, 1.0, (len(grid), 65)))
    add("slots65_one_sweep", X, y, grid, max_sweeps=1)
    X, y = draw(40, 1024, 16, 3, rho=0.0, noise=0.3, spread=True)
    add("p1024", X, y, [(0.02, 0.5), (0.002, 1.0)])
    start = np.zeros((1, 1024))
    start[0, 5::64] = 0.5  # sixteen wrong columns, one per slot
    add("p1024_wrong_start", X, y, [(0.02, 0.5)], starts=start)
    X = rng.standard_normal((12, 20))
    X[:, 7] = 0.0
    y = X[:, 0] - X[:, 3] + X[:, 11] + 0.2 * rng.standard_normal(12)
    add("rank_deficient", X, y, [(0.02, 0.0), (0.02, 0.1), (0.0, 0.05)])
    add("rank_deficient_box", X, y, [(0.02, 0.0), (0.02, 0.1), (0.0, 0.05)], big_M=0.5)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return _cases()


@functools.lru_cache(maxsize=None)
def reference(name):
    """``(G, c, the rule's dicts)`` of case ``name`` on the numpy Gram: computed once per process and left unchanged."""
    from _l0_local_reference import gram

    k = cases()[name]
    G, c, _, _, _ = gram(k["X"], k["y"])
    G.setflags(write=False)
    c.setflags(write=False)
    return G, c, run_rule(G, c, k)


def run_rule(G, c, k):
    """The rule on every cell of case ``k`` with the Gram ``(G, c)``: a list of the rule's dicts."""
    from _l0_local_bound_reference import rule

    return [rule(G, c, float(k["alphas"][e]), float(k["etas"][e]), k["big_M"], start=None if k["starts"] is None else k["starts"][e],
                 max_sweeps=k["max_sweeps"], gap_tol=k["gap_tol"]) for e in range(len(k["alphas"]))]
