"""The multi-lane gradient reference and its componentwise bound (tests/_gradient_reference.py) on their own, no GPU: a
correct float64 evaluation in any summation order passes, and each numpy "defective kernel" -- the index mistakes a
multi-lane kernel can make -- is flagged on the lanes it touches.  What tests/test_gradient_lanes_gpu.py concludes from a
kernel passing rests on both directions."""

import numpy as np
import pytest

from _gradient_reference import assert_within_bound, excess, gram_reference, lane_inputs, lanes_reference

B = 18  # (lanes 16 and 17: the vector units' share of xtr18 / rowdot18)


def _data(family, n, p, seed):
    rng = np.random.default_rng(seed)
    if family == "normal":
        X = rng.standard_normal((n, p))
        y = rng.standard_normal(n)
    else:  # ill-conditioned: columns 1e3 + N(0, 1), y with mean 1e4 (cancellation in every residual)
        X = 1e3 + rng.standard_normal((n, p))
        y = 1e4 + rng.standard_normal(n)
    return rng, X, y


def _plain(X, y, Z, W, ne, rows=None, dtype=np.float64):
    """numpy's own evaluation of every lane (float64 by default), optionally over a list of row indices."""
    if rows is not None:
        X, y, W = X[rows], y[rows], W[:, rows]
    X, y, Z, W = (a.astype(dtype) for a in (X, y, Z, W))
    R = X @ Z.T - y[:, None]
    G = (X.T @ (W.T * R)).T / ne[:, None].astype(dtype)
    loss = np.sum(W.T * R * R, axis=0) / (2 * ne.astype(dtype))
    return G.astype(np.float64), loss.astype(np.float64)


def _blocked_reversed(X, y, Z, W, ne, block=37):
    """The same sums in another order: row blocks from the last to the first, each block's own partial sums."""
    n = X.shape[0]
    G = np.zeros(Z.shape)
    loss = np.zeros(Z.shape[0])
    for i1 in range(n, 0, -block):
        i0 = max(0, i1 - block)
        R = X[i0:i1] @ Z.T - y[i0:i1, None]
        G += (X[i0:i1].T @ (W[:, i0:i1].T * R)).T
        loss += np.sum(W[:, i0:i1].T * R * R, axis=0)
    return G / ne[:, None], loss / (2 * ne)


@pytest.fixture(params=["normal", "ill"])
def case(request):
    rng, X, y = _data(request.param, 1001, 53, 11)
    Z, W, ne = lane_inputs(rng, 1001, 53, B)
    return X, y, Z, W, ne, lanes_reference(X, y, Z, W, ne)


def test_the_lane_inputs_differ_lane_by_lane():
    rng, X, y = _data("normal", 1001, 53, 11)
    Z, W, ne = lane_inputs(rng, 1001, 53, 32)
    assert len({Z[l].tobytes() + W[l].tobytes() + ne[l].tobytes() for l in range(32)}) == 32
    assert np.all(Z[2::5] == 0) and np.all(np.abs(Z[3::5]).max(axis=1) > 1e5) and np.all(np.abs(Z[4::5]).max(axis=1) < 1e-4)
    assert np.all(np.count_nonzero(Z[1::5], axis=1) == 3)
    assert len({W[l].tobytes() for l in range(5)}) == 5  # (the five weight kinds among the first five lanes)
    assert np.any(np.abs(ne - W.sum(axis=1)) > 1.0)


def test_correct_evaluations_in_any_order_pass(case):
    X, y, Z, W, ne, ref = case
    for G, loss in (_plain(X, y, Z, W, ne), _blocked_reversed(X, y, Z, W, ne),
                    _plain(X, y, Z, W, ne, rows=np.arange(X.shape[0])[::-1])):
        assert_within_bound(G, loss, ref, "a correct evaluation")


def test_two_lanes_swapped_are_flagged(case):
    X, y, Z, W, ne, ref = case
    G, loss = _plain(X, y, Z, W, ne)
    G[[0, 1]], loss[[0, 1]] = G[[1, 0]], loss[[1, 0]]
    e = excess(G, loss, ref)
    assert e[0] > 1 and e[1] > 1 and np.all(e[2:] <= 1)


def test_lane_seventeen_on_lane_sixteens_weights_is_flagged(case):
    X, y, Z, W, ne, ref = case
    W2 = W.copy()
    W2[17] = W[16]
    G, loss = _plain(X, y, Z, W2, ne)
    e = excess(G, loss, ref)
    assert e[17] > 1 and np.all(np.delete(e, 17) <= 1)


def test_a_dropped_last_row_block_is_flagged(case):
    X, y, Z, W, ne, ref = case
    n = X.shape[0]
    G, loss = _plain(X, y, Z, W, ne, rows=np.arange(n - 8))
    e = excess(G, loss, ref)
    touched = np.any(W[:, n - 8:] != 0, axis=1)
    assert np.all(e[touched] > 1) and np.all(e[~touched] <= 1)
    assert touched.sum() >= B // 2


def test_a_row_counted_twice_is_flagged(case):
    X, y, Z, W, ne, ref = case
    n = X.shape[0]
    row = n - 1
    G, loss = _plain(X, y, Z, W, ne, rows=np.r_[np.arange(n), row])
    e = excess(G, loss, ref)
    touched = W[:, row] != 0
    assert np.all(e[touched] > 1) and np.all(e[~touched] <= 1)


def test_lane_zeros_n_eff_for_every_lane_is_flagged(case):
    X, y, Z, W, ne, ref = case
    G, loss = _plain(X, y, Z, W, np.full(B, ne[0]))
    e = excess(G, loss, ref)
    other = ne != ne[0]
    assert other.sum() >= B // 2
    assert np.all(e[other] > 1) and np.all(e[~other] <= 1)


def test_float32_accumulation_is_flagged(case):
    X, y, Z, W, ne, ref = case
    G, loss = _plain(X, y, Z, W, ne, dtype=np.float32)
    assert np.all(excess(G, loss, ref) > 1)


def test_n_rows_is_the_reference_of_the_first_rows():
    rng, X, y = _data("normal", 400, 30, 5)
    Z, W, ne = lane_inputs(rng, 400, 30, 7, n_rows=100)
    ref = lanes_reference(X, y, Z, W, ne, n_rows=100)
    sub = lanes_reference(X[:100], y[:100], Z, W[:, :100], ne)
    assert np.array_equal(ref.g, sub.g) and np.array_equal(ref.loss, sub.loss)
    G, loss = _plain(X, y, Z, W, ne, rows=np.arange(100))
    assert_within_bound(G, loss, ref)
    G, loss = _plain(X, y, Z, W, ne)  # (all rows: a kernel that ignores n_rows)
    assert np.all(excess(G, loss, ref)[np.any(W[:, 100:] != 0, axis=1)] > 1)


def test_the_float64_reference_doubles_its_bound(monkeypatch):
    import _gradient_reference as gr

    rng, X, y = _data("normal", 300, 20, 2)
    Z, W, ne = lane_inputs(rng, 300, 20, 5)
    exact = lanes_reference(X, y, Z, W, ne)
    monkeypatch.setattr(gr, "LONGDOUBLE_LIMIT", 0)
    f64 = gr.lanes_reference(X, y, Z, W, ne)
    assert exact.exact and not f64.exact
    assert np.allclose(f64.g_bound, 2 * exact.g_bound, rtol=1e-12, atol=0)
    assert_within_bound(f64.g.astype(np.float64), f64.loss.astype(np.float64), exact)


@pytest.mark.parametrize("family", ["normal", "ill"])
def test_a_fold_gram_formed_as_all_rows_minus_the_rest_passes_and_a_wrong_gram_is_flagged(family):
    # what the covariance route's entries are (engine_cov.hip): X^T X of all rows minus the rows left out, then / n_eff
    rng, X, y = _data(family, 600, 24, 9)
    K = 4
    fold = rng.integers(0, K, 600)
    Z, _, _ = lane_inputs(rng, 600, 24, 10)
    GA, cA, yyA = X.T @ X, X.T @ y, y @ y
    grams = []
    for k in range(K):
        out = fold == k
        ne = float(np.sum(~out))
        grams.append(((GA - X[out].T @ X[out]) / ne, (cA - X[out].T @ y[out]) / ne, (yyA - y[out] @ y[out]) / ne, ne))
    idx = np.arange(10) % K
    for l in range(10):
        G, c, yy, ne = grams[idx[l]]
        g = G @ Z[l] - c
        loss = 0.5 * Z[l] @ (G @ Z[l]) - c @ Z[l] + 0.5 * yy
        w = (fold != idx[l]).astype(np.float64)
        ref = lanes_reference(X, y, Z[l:l + 1], w[None, :], [ne], bound_weights=np.maximum(w, 1.0)[None, :])
        assert_within_bound(g, None, ref, "gradient from the fold's Gram")
        assert_within_bound(g, [loss], gram_reference(G, c, yy, Z[l:l + 1]), "the same Gram")
        if np.any(Z[l] != 0):
            G2, c2, yy2, _ = grams[(idx[l] + 1) % K]  # (the neighbouring lane's Gram)
            assert excess(G2 @ Z[l] - c2, None, gram_reference(G, c, yy, Z[l:l + 1]))[0] > 1
