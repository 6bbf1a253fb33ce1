"""The inputs that tests/test_l0_local_cv_gpu.py compares on, and their reference: per (row set, cell) the numpy restatement
(tests/_l0_local_reference.solve_cells) run on ``X[rows], y[rows]`` DIRECTLY -- rows selected and centred in numpy, no Gram of a
complement, no elimination.  tests/test_l0_local_cv_cpu.py recomputes the premise of every case (status 0, every decision margin
and lead >= 1e-6) and what each case is there to cover, so that a change of inputs cannot silently void the GPU comparisons.

Row sets: the training rows of ``KFold(k)`` without shuffle, then all rows.  ``alphas`` are relative to ``var y`` of all rows."""

import functools

import numpy as np
from sklearn.model_selection import KFold

from _l0_local_reference import gram, hard_law, solve_cells
from test_l0_local_gpu import draw


def _hard(seed):
    X, y = hard_law(seed, n=45)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


# name: (data, shift of X with an intercept, folds, alphas / var y, etas)
CASES = {
    "two_slots": (lambda: draw(60, 65, 6, 65), 1.0, 3, (0.01, 0.05, 0.3), (0.0, 0.02, 0.0)),
    "sixteen_row_sets": (lambda: draw(48, 6, 3, 11), 0.0, 15, (0.003, 0.03), (0.0, 0.0)),
    "three_slots": (lambda: draw(45, 130, 6, 130), 0.0, 5, (0.02, 0.1), (0.01, 0.0)),
    "sixteen_slots": (lambda: draw(200, 1024, 16, 3, rho=0.0, noise=0.3, spread=True), 0.5, 2, (0.015,), (0.0,)),
    "hard_3": (lambda: _hard(3), 0.0, 3, (0.02, 0.05, 0.1), (0.0, 0.0, 0.0)),
    "hard_7": (lambda: _hard(7), 0.0, 3, (0.02, 0.05, 0.1), (0.0, 0.0, 0.0)),
}
# (case, intercept) pairs the GPU tests run; the 1024-column case and the hard law with an intercept only
RUNS = [("two_slots", False), ("two_slots", True), ("sixteen_row_sets", False), ("sixteen_row_sets", True), ("three_slots", False),
        ("three_slots", True), ("sixteen_slots", True), ("hard_3", True), ("hard_7", True)]


@functools.lru_cache(maxsize=None)
def case(name, intercept):
    """``(X, y, row sets, alphas, etas)``: ``X`` shifted when an intercept is fitted; row sets as index arrays, the folds' training
    rows then all rows."""
    data, shift, folds, rel, etas = CASES[name]
    X, y = data()
    if intercept and shift:
        X = X + shift
        X.setflags(write=False)
    n = X.shape[0]
    rows = [tr for tr, _ in KFold(folds).split(X)] + [np.arange(n)]
    return X, y, rows, np.array(rel) * float(np.var(y)), np.array(etas, dtype=float)


@functools.lru_cache(maxsize=None)
def reference(name, intercept, swaps=True):
    """Per row set the restatement's cells on ``X[rows], y[rows]``, each with ``intercept`` (``y_mean - x_mean^T beta`` of those rows)
    added.  Computed once and shared; nobody writes to it."""
    X, y, rows, alphas, etas = case(name, intercept)
    out = []
    for r in rows:
        cells = solve_cells(X[r], y[r], alphas, etas, swaps=swaps, fit_intercept=intercept)
        _, _, _, x_mean, y_mean = gram(X[r], y[r], None, intercept)
        for cell in cells:
            cell["intercept"] = float(y_mean - x_mean @ cell["beta"])
        out.append(cells)
    return out


def masks(n, rows, all_rows_given=True):
    """The row sets as the engine takes them: 0/1 weights and the divisor of each Gram; ``all_rows_given`` False hands the last set
    (all rows) over as None."""
    weights = []
    for r in rows:
        m = np.zeros(n)
        m[r] = 1.0
        weights.append(m)
    if not all_rows_given:
        weights[-1] = None
    return weights, [len(r) for r in rows]


@functools.lru_cache(maxsize=None)
def second_start_case():
    """Two starts -- zero and a fixed vector on four columns -- on the hard law at seed 0, n = 45, three folds and all rows, with an
    intercept: found on the CPU by running the restatement over seeds and start vectors.  At each of the three alphas the second
    start wins in some row sets and loses in others (every lead >= 1e-4).  Returns ``(X, y, row sets, alphas, starts [S, p], the
    reference per row set, the winners [row sets, cells])``."""
    X, y = _hard(0)
    rows = [tr for tr, _ in KFold(3).split(X)] + [np.arange(45)]
    alphas = np.array([0.02, 0.05, 0.1]) * float(np.var(y))
    rng = np.random.default_rng(1000)
    second = np.zeros(14)
    second[rng.choice(14, 4, replace=False)] = rng.choice([-1.0, 1.0], 4)
    starts = np.stack([np.zeros(14), second])
    ref = []
    for r in rows:
        cells = solve_cells(X[r], y[r], alphas, np.zeros(3), starts=np.broadcast_to(starts, (3, 2, 14)), fit_intercept=True)
        _, _, _, x_mean, y_mean = gram(X[r], y[r], None, True)
        for cell in cells:
            cell["intercept"] = float(y_mean - x_mean @ cell["beta"])
        ref.append(cells)
    return X, y, rows, alphas, starts, ref, np.array([[cell["start"] for cell in cells] for cells in ref])


def distinct_supports(cells_by_row_set, cell):
    return len({tuple(np.flatnonzero(cells[cell]["beta"])) for cells in cells_by_row_set})
