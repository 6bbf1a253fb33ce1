"""The problems of tests/test_l1l0_local_gpu.py, and the numpy restatement's answer to each (computed once per process and
left unchanged): tests/test_l1l0_local_cpu.py recomputes every premise without a device, the GPU tests compare against the same
cells.  The shapes are those at which the kernel can go wrong: one column, the slot boundary (63, 64, 65, 130), all sixteen slots
(1024, from zero and from a wrong start), eta = 0 with fewer rows than columns, a binding box, a lam above max |c|, alpha = 0,
a second start that wins, the descent alone, and the hard law with swaps."""

import functools

import numpy as np
from _l0_local_reference import gram, hard_law
from _l1l0_local_reference import solve_cells
from test_l0_local_gpu import draw

MARGIN_MIN = 1e-6


def var(y):
    return float(np.var(y))


def _wrong_start_1024():
    start = np.zeros((1, 1, 1024))
    start[0, 0, 5::64] = 0.5  # sixteen wrong columns, one per slot
    return start


def _second_start():
    """The hard law at seed 0: the search from zero misses what a start on the brute-force optimum's support reaches."""
    X, y = hard_law(0, n=30, p=10, k=3)
    return X, y, 0.05 * var(y), 0.02


@functools.lru_cache(maxsize=None)
def second_start_optimum():
    from _l1l0_local_reference import brute_force

    X, y, alpha, lam = _second_start()
    G, c, _, _, _ = gram(X, y)
    return brute_force(G, c, alpha, lam, 100.0)


def _cases():
    out = {}

    def add(name, X, y, cells, big_M=100.0, starts=None, swaps=True):
        cells = np.asarray(cells, dtype=float).reshape(-1, 3)
        out[name] = dict(X=X, y=y, alphas=cells[:, 0] * var(y), l1s=cells[:, 1].copy(), ridges=cells[:, 2].copy(), big_M=big_M, starts=starts,
                         swaps=swaps)

    X, y = draw(20, 1, 1, 0)
    add("p1", X, y, [(0.01, 0.05, 0.0), (10.0, 0.05, 0.0), (0.0, 0.05, 0.0)])
    for p in (63, 64, 65, 130):
        X, y = draw(80, p, 6, p)
        add(f"slots{p}", X, y, [(0.01, 0.05, 0.0), (0.05, 0.2, 0.02), (0.3, 0.02, 0.0), (0.0, 0.3, 0.0)])
    X, y = draw(200, 1024, 16, 3, rho=0.0, noise=0.3, spread=True)
    add("p1024_zero", X, y, [(0.015, 0.05, 0.0)])
    add("p1024_wrong_start", X, y, [(0.015, 0.05, 0.0)], starts=_wrong_start_1024())
    X, y = draw(40, 130, 5, 7)
    add("rows_below_columns", X, y, [(0.02, 0.1, 0.0), (0.0, 0.2, 0.0)])
    X, y = draw(80, 20, 4, 5)
    add("box", X, y, [(0.01, 0.05, 0.0)], big_M=0.6)
    X, y = draw(40, 12, 4, 5)
    cmax = float(np.max(np.abs(gram(X, y)[1])))
    add("lam_above_max_c", X, y, [(0.0, 1.01 * cmax, 0.0), (0.01, 1.01 * cmax, 0.0)])
    add("alpha_zero", X, y, [(0.0, 0.1, 0.0), (0.0, 0.4, 0.05)])
    X, y, alpha, lam = _second_start()
    starts = np.stack([np.zeros(10), second_start_optimum()[1]])[None]
    add("second_start", X, y, [(alpha / var(y), lam, 0.0)], starts=starts)
    add("second_start_reversed", X, y, [(alpha / var(y), lam, 0.0)], starts=starts[:, ::-1].copy())
    X, y = hard_law(5, n=30, p=10, k=3)
    add("hard_law_swaps", X, y, [(0.05, 0.02, 0.0), (0.01, 0.1, 0.0), (0.2, 0.02, 0.0)])
    X11, y11 = hard_law(11, n=30, p=10, k=3)
    add("hard_law_two_swaps", X11, y11, [(0.01, 0.02, 0.0), (0.01, 0.1, 0.0)])
    add("hard_law_descent", X, y, [(0.05, 0.02, 0.0), (0.01, 0.1, 0.0), (0.2, 0.02, 0.0)], swaps=False)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return _cases()


@functools.lru_cache(maxsize=None)
def reference(name):
    """The restatement's cells of case ``name`` (tests/_l1l0_local_reference.solve_cells)."""
    k = cases()[name]
    return solve_cells(k["X"], k["y"], k["alphas"], k["l1s"], k["ridges"], big_M=k["big_M"], starts=k["starts"], swaps=k["swaps"])


def premise(name):
    """``(ok, text)``: every cell of the case has status 0 and margin and lead >= 1e-6."""
    cells = reference(name)
    text = "; ".join(f"margin {c['margin']:.3e} lead {c['lead']:.3e} status {c['status']} swaps {c['swaps']} nnz {np.count_nonzero(c['beta'])}"
                     for c in cells)
    return all(c["status"] == 0 and c["margin"] >= MARGIN_MIN and c["lead"] >= MARGIN_MIN for c in cells), text
