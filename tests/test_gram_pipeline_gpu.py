"""ws_gram_kernel at the edges of its row loop (sparse-lm_amd/csrc/ws_kernels.hpp, ws_gram_rows).

The loop keeps the loads of three 4-row steps in flight behind the MFMAs of a step, sixteen rows per iteration, and is
instantiated per tile pattern (1..4 x 1..4 output tiles of a wavefront) and with or without row weights.  So the shapes
here are the ones where it changes course:
  rows      n = 7 (one block, two of its four row parts empty), n = 40 (parts of 8 and 12 rows: the prologue's loads run
            past the end), n = 1000 (15 blocks of 66-67 rows: parts of 16-17 rows, one full iteration and a remainder
            shorter than the prefetch depth), n = 4099;
  builds    fresh selections of 16, 100 (not a multiple of 16), 112 (7 tiles, split by rows) and 144 columns (9 tiles, the
            plain mapping); appends 112 -> 128 (one new tile row), 128 -> 176 (three new tile rows, two column quarters)
            and 64 -> 192 (eight new tile rows: two chunks);
  row sets  none (Dataset.ws_build: the instantiation without weights), one weight vector with zeros, two fold masks in
            one call (two sets, ws_block_owner_kernel with shared, skipped and mixed row blocks).
Every Gram is held against X_W^T diag(w) X_W / n_eff in long double under the componentwise bound of
tests/_gradient_reference.py (the one tests/test_working_set_lanes_gpu.py uses), is symmetric within that bound, holds
exact zeros on the padding, and comes out with the same bits from a second call.
"""

import numpy as np
import pytest

from _gradient_reference import assert_gram_within_bound, ws_build_expected, ws_gram_reference, ws_K
from sparselm_amd import _engine

pytestmark = pytest.mark.gpu
WS, NO_WS = _engine.FLAG_WORKING_SET, _engine.FLAG_NO_WORKING_SET

P = 256
ROWS = [7, 40, 1000, 4099]
BUILDS = [[16], [100], [112], [144], [112, 128], [128, 176], [64, 192]]
ROW_SETS = ["none", "weights", "two_folds"]


@pytest.fixture(scope="module")
def eng():
    return _engine.get_engine(0)


@pytest.fixture(scope="module")
def datasets(eng):
    """One dataset per row count, shared by the cases (the data stay as they are)."""
    made = {}
    for n in ROWS:
        rng = np.random.default_rng(n)
        X, y = rng.standard_normal((n, P)), rng.standard_normal(n)
        X.setflags(write=False)
        made[n] = (X, y, eng.dataset(X, y))
    yield made
    for _, _, ds in made.values():
        ds.close()


_REFS = {}


def _reference(n, X, cols, kind, w):
    key = (n, cols.tobytes(), kind, 0 if w is None else w.tobytes())
    if key not in _REFS:
        _REFS[key] = ws_gram_reference(X, cols, w, None if w is None else w.sum())
    return _REFS[key]


def _row_weights(kind, n):
    """(lanes, n) weights, or None: uniform(0, 2) with every third row zero; two contiguous folds' masks."""
    if kind == "none":
        return None
    if kind == "weights":
        w = np.random.default_rng(n + 1).uniform(0.0, 2.0, n)
        w[::3] = 0.0
        return w[None]
    bounds = np.linspace(0, n, 4).astype(int)
    W = np.ones((2, n))
    W[0, bounds[0]:bounds[1]] = 0.0
    W[1, bounds[1]:bounds[2]] = 0.0
    return W


def _build(ds, cols, k_end, W):
    if W is None:
        return ds.ws_build(cols, k_end)
    B = W.shape[0]
    return ds.working_set_lanes(np.zeros((B, P)), cols, k_end, on_ws=[0] * B, row_weights=W, n_eff=W.sum(axis=1))


@pytest.mark.parametrize("kind", ROW_SETS)
@pytest.mark.parametrize("k_end", BUILDS, ids=lambda k: "-".join(map(str, k)))
@pytest.mark.parametrize("n", ROWS)
def test_gram_at_the_edges_of_the_row_loop(datasets, n, k_end, kind):
    X, _, ds = datasets[n]
    kreal = k_end[-1]
    cols = np.random.default_rng(kreal + len(k_end)).choice(P, kreal, replace=False).astype(np.int32)
    W = _row_weights(kind, n)
    r = _build(ds, cols, k_end, W)
    again = _build(ds, cols, k_end, W)
    assert np.array_equal(r.gram, again.gram), "the same build twice: other bits"
    expect = ws_build_expected(k_end, 1, owner=W is not None)
    assert r.kernels.split(";")[:len(expect)] == expect, r.kernels
    K = ws_K(kreal)
    n_sets = 1 if W is None else W.shape[0]
    assert r.K == K and r.n_sets == n_sets and r.gram.shape == (n_sets, K, K)
    for st in range(n_sets):
        G = r.gram[st]
        ref = _reference(n, X, cols, kind, None if W is None else W[st])
        assert_gram_within_bound(G, ref, f"n={n}, k_end={k_end}, {kind}, set {st}")
        assert np.all(G[kreal:] == 0.0) and np.all(G[:, kreal:] == 0.0), "the padding does not hold zeros"
        # (G_ij and G_ji are each within the bound of the same number)
        assert np.all(np.abs(G - G.T) <= ref.bound + ref.bound.T), "not symmetric within the bound"
        if len(k_end) > 1:  # the mirrored entries of an append are copies
            lo = (k_end[-2] // 16) * 16
            assert np.array_equal(G[:lo, lo:], G[lo:, :lo].T), "mirrored entries differ from their counterparts"


def test_path_on_the_engines_lanes_against_the_plain_iteration(eng):
    n, p = 4096, 600
    rng = np.random.default_rng(n + p)
    X = rng.standard_normal((n, p))
    beta = np.zeros(p)
    beta[rng.choice(p, 12, replace=False)] = rng.uniform(1, 5, 12) * rng.choice([-1, 1], 12)
    y = X @ beta + rng.standard_normal(n)
    amax = np.max(np.abs(X.T @ y / n))
    pts = [(a, 0, 0) for a in np.geomspace(amax, 1e-2 * amax, 20)]
    with eng.dataset(X, y) as ds:
        r1 = ds.solve_path(pts, tol=1e-11, flags=WS)
        r0 = ds.solve_path(pts, tol=1e-11, lanes=4, flags=NO_WS)
    assert r1.converged and r0.converged
    assert r1.ws_builds >= 1 and r1.ws_refined > 0 and r0.ws_builds == 0
    assert np.max(np.abs(r1.betas - r0.betas)) < 1e-8 * np.max(np.abs(r0.betas))
