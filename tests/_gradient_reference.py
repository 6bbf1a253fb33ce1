"""A high-precision reference for one gradient pass of several lanes, with a componentwise error bound.

For lane l with point z_l, row weights w_l and scale n_eff_l, over the first ``n_rows`` rows (all when 0):

    r = X z_l - y,    g_l = X^T (w_l * r) / n_eff_l,    loss_l = sum_i w_li r_i^2 / (2 n_eff_l).

The reference is computed in ``np.longdouble`` when n_rows * p <= 2e7 (64-bit significand on x86: its own error is
negligible against the bound), in float64 otherwise -- the bound is then doubled, to cover the reference's own rounding.

Bound (eps = 2^-52, any summation order, FMA or not, partial sums in any tree):

    |G_lj - g_lj|   <= 2 (n_rows + p + 16) eps * A_lj,   A_lj = sum_i |x_ij| w_li (|x_i|.|z_l| + |y_i|) / n_eff_l
    |loss_l - ref|  <= 2 (n_rows + p + 16) eps * sum_i w_li (|x_i|.|z_l| + |y_i|)^2 / (2 n_eff_l)

This is the classical first-order bound of a dot product (gamma_k < 1.01 k u, u = eps / 2) applied to the residual (p + 1
terms), the weighting, the sum over rows (n_rows terms) and the final scaling, with a factor of four to spare.  It does NOT
cover a dropped or doubled row (|x_ij r_i| / n_eff of one row is ~1/n of A_lj, far above n eps A_lj), another lane's point,
weights or n_eff, or float32 accumulation (2^-24 relative).  ``tests/test_gradient_lanes_cpu.py`` checks both directions.

The covariance route computes G_k z - c_k from a Gram of the lane's row set that the engine forms as the Gram of all rows
minus that of the rows left out (engine_cov.hip): its rounding is relative to the rows of the minuend, so ``bound_weights``
(max(w, 1), all rows) stand in for w in A and in the loss term.  ``gram_reference`` checks the same lanes against the Gram the
engine holds, with a bound that involves no rows at all.
"""

from __future__ import annotations

import numpy as np

EPS = 2.0**-52
LONGDOUBLE_LIMIT = 2e7  # n_rows * p up to which the reference is computed in np.longdouble


class LaneReference:
    """g (lanes, p), loss (lanes,) and their componentwise bounds g_bound, loss_bound."""

    def __init__(self, g, loss, g_bound, loss_bound, exact):
        self.g, self.loss, self.g_bound, self.loss_bound, self.exact = g, loss, g_bound, loss_bound, exact


def lanes_reference(X, y, Z, W=None, n_eff=None, n_rows=0, bound_weights=None, cols=None, chunk=8192) -> LaneReference:
    """The reference of every lane: Z (lanes, p); W (lanes, n) or None (ones); n_eff (lanes,) or None (n).  ``cols``: only
    these entries of g (the residuals still use every column)."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    n, p = X.shape
    B = Z.shape[0]
    m = int(n_rows) if n_rows else n
    W = np.ones((B, n)) if W is None else np.asarray(W, dtype=np.float64).reshape(B, n)
    ne = np.full(B, float(n)) if n_eff is None else np.asarray(n_eff, dtype=np.float64).reshape(B)
    Wb = W if bound_weights is None else np.asarray(bound_weights, dtype=np.float64).reshape(B, n)
    exact = m * p <= LONGDOUBLE_LIMIT
    dt = np.longdouble if exact else np.float64
    cols = np.arange(p) if cols is None else np.asarray(cols)
    g = np.zeros((B, cols.size), dtype=dt)
    loss = np.zeros(B, dtype=dt)
    A = np.zeros((B, cols.size))
    Aloss = np.zeros(B)
    Za = np.abs(Z)
    Zd = Z.astype(dt)
    for i0 in range(0, m, chunk):  # (rows in chunks: the full-size case does not hold |X| or a long double X at once)
        i1 = min(m, i0 + chunk)
        Xc = X[i0:i1]
        Xcd = Xc.astype(dt)
        R = Xcd @ Zd.T - y[i0:i1, None].astype(dt)  # (rows, lanes)
        Wc = W[:, i0:i1].T.astype(dt)
        g += (Xcd[:, cols].T @ (Wc * R)).T
        loss += np.sum(Wc * R * R, axis=0)
        Xa = np.abs(Xc)
        S = Xa @ Za.T + np.abs(y[i0:i1])[:, None]  # |x_i|.|z_l| + |y_i|
        Wbc = Wb[:, i0:i1].T
        A += (Xa[:, cols].T @ (Wbc * S)).T
        Aloss += np.sum(Wbc * S * S, axis=0)
    g = g / ne[:, None].astype(dt)
    loss = loss / (2 * ne.astype(dt))
    k = 2.0 * (m + p + 16) * EPS * (1.0 if exact else 2.0)
    return LaneReference(g, loss, k * A / ne[:, None], k * Aloss / (2 * ne), exact)


def gram_reference(G, c, yy, Z) -> LaneReference:
    """g = G z - c and loss = z^T G z / 2 - c^T z + yy / 2 from ONE Gram (G, c, yy) for every lane of Z, with the bound of
    a p-term product: 2 (p + 16) eps (|G||z| + |c|), and for the loss (cancellation-prone by construction)
    2 (p + 16) eps (|z|^T |G| |z| + 2 |c|^T |z| + yy)."""
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    p = Z.shape[1]
    Gd, cd, Zd = G.astype(np.longdouble), c.astype(np.longdouble), Z.astype(np.longdouble)
    g = Zd @ Gd.T - cd[None, :]
    loss = 0.5 * np.sum(Zd * (Zd @ Gd.T), axis=1) - Zd @ cd + 0.5 * np.longdouble(yy)
    Za = np.abs(Z)
    Ga = np.abs(G)
    k = 2.0 * (p + 16) * EPS
    gb = k * (Za @ Ga.T + np.abs(c)[None, :])
    lb = k * (np.sum(Za * (Za @ Ga.T), axis=1) + 2 * Za @ np.abs(c) + abs(yy))
    return LaneReference(g, loss, gb, lb, True)


def excess(G, loss, ref: LaneReference):
    """Per lane: the largest |error| / bound over the lane's gradient entries and its loss (> 1: outside the bound).  An
    entry whose bound is 0 (a column that is zero on the lane's rows) must be exactly 0."""
    G = np.atleast_2d(np.asarray(G, dtype=np.float64))
    err = np.abs(G.astype(np.longdouble) - ref.g).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rg = np.where(ref.g_bound > 0, err / ref.g_bound, np.where(err > 0, np.inf, 0.0))
    out = np.max(rg, axis=1)
    if loss is not None:
        el = np.abs(np.asarray(loss, dtype=np.float64).astype(np.longdouble) - ref.loss).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            rl = np.where(ref.loss_bound > 0, el / ref.loss_bound, np.where(el > 0, np.inf, 0.0))
        out = np.maximum(out, rl)
    return out


def assert_within_bound(G, loss, ref: LaneReference, what=""):
    e = excess(G, loss, ref)
    bad = np.flatnonzero(~(e <= 1.0))
    assert bad.size == 0, f"{what}: lanes {bad.tolist()} outside the componentwise bound (error / bound {e[bad].tolist()})"


Z_KINDS = ("dense", "three", "zero", "big", "small")
W_KINDS = ("mask", "uniform", "ones", "last_row", "no_last_block")


def lane_inputs(rng, n, p, B, n_rows=0, offset=0):
    """Distinct inputs for every lane l, k = (l + offset) % 5: a point of kind Z_KINDS[k] (dense N(0,1), three non-zeros,
    all zero, dense x 1e6, dense x 1e-6 -- a lane that reads a big lane's numbers fails its own bound by far), row weights
    of kind W_KINDS[(l // 5 + k) % 5] (a 0/1 fold mask, uniform(0, 2), ones, only the last row, zero on the last n/16 rows:
    at least the last row block of any launch of 16 or more blocks), and an n_eff that is n_rows, sum w, or neither (a
    kernel that divides by sum w instead of the n_eff passed shows).  `offset` gives the lanes other kinds: fresh inputs."""
    m = int(n_rows) if n_rows else n
    Z = np.zeros((B, p))
    W = np.ones((B, n))
    ne = np.zeros(B)
    for l in range(B):
        k = (l + offset) % 5
        zk = Z_KINDS[k]
        if zk == "dense":
            Z[l] = rng.standard_normal(p)
        elif zk == "three":
            Z[l, rng.choice(p, min(3, p), replace=False)] = rng.standard_normal(min(3, p))
        elif zk == "big":
            Z[l] = 1e6 * rng.standard_normal(p)
        elif zk == "small":
            Z[l] = 1e-6 * rng.standard_normal(p)
        wk = W_KINDS[(l // 5 + k) % 5]  # (so that point and weight kinds meet in every combination over 25 lanes)
        if wk == "mask":
            W[l] = (rng.random(n) >= 0.2).astype(np.float64)
        elif wk == "uniform":
            W[l] = rng.uniform(0.0, 2.0, n)
        elif wk == "last_row":
            W[l] = 0.0
            W[l, n - 1] = 1.0
        elif wk == "no_last_block":
            W[l, n - max(1, n // 16):] = 0.0
        sw = float(np.sum(W[l, :m]))
        ne[l] = (float(m), max(sw, 0.5), 0.73 * m + 1.5)[(l + offset) % 3]
    return Z, W, ne
