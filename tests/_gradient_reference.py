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

The working set W (positions k < Kreal hold feature cols[k], K = max(16, Kreal rounded up to 16), the rest is padding) has a
Gram of its own per row set, G = X_W^T diag(w) X_W / n_eff (ws_kernels.hpp), and at a sample start -X_W^T y / n and
y^T y / 2n.  ``ws_gram_reference`` and ``ws_xty_reference`` give them with the bound of an n-term dot product:

    |G_ij - ref| <= 2 (n + 16) eps * sum_r w_r |x_ri x_rj| / n_eff       (padding rows and columns: exactly 0)

in any order of the row sums (row blocks, interleaved chains, a fixed-order fold of the blocks' partials) and whichever
factor the weight is applied to.  A row block summed twice or left out, another row set's weights or n_eff, a stale tile
row, an entry left unmirrored, float32 accumulation or a gathered column one position off are each far outside it
(``tests/test_working_set_lanes_cpu.py``).  The gradient of a lane whose point is zero outside W is ``lanes_reference``'s
whichever way the residual is formed (from X or from the gathered columns).
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


# ---- the working set ----------------------------------------------------------------------------------------------------------
def ws_K(kreal):
    """Columns of W in use with the padding: max(16, Kreal rounded up to a multiple of 16) (ws_select_kernel)."""
    return max(16, (int(kreal) + 15) // 16 * 16)


class GramReference:
    """G (K, K) and its componentwise bound (0 on the padding: those entries must be exactly 0)."""

    def __init__(self, G, bound, exact):
        self.G, self.bound, self.exact = G, bound, exact


def ws_gram_reference(X, cols, w=None, n_eff=None, chunk=8192) -> GramReference:
    """X_W^T diag(w) X_W / n_eff for W = ``cols`` (w None: ones; n_eff None: n), padded to K; long double while n K <= 2e7."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    cols = np.asarray(cols, dtype=np.int64)
    kr = cols.size
    K = ws_K(kr)
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64).reshape(n)
    ne = float(n) if n_eff is None else float(n_eff)
    exact = n * K <= LONGDOUBLE_LIMIT
    dt = np.longdouble if exact else np.float64
    G = np.zeros((kr, kr), dtype=dt)
    A = np.zeros((kr, kr))
    for i0 in range(0, n, chunk):
        i1 = min(n, i0 + chunk)
        Xw = X[i0:i1][:, cols]
        Xd = Xw.astype(dt)
        G += Xd.T @ (w[i0:i1, None].astype(dt) * Xd)
        Xa = np.abs(Xw)
        A += Xa.T @ (w[i0:i1, None] * Xa)
    k = 2.0 * (n + 16) * EPS * (1.0 if exact else 2.0)
    Gp = np.zeros((K, K), dtype=dt)
    Bp = np.zeros((K, K))
    Gp[:kr, :kr] = G / dt(ne)
    Bp[:kr, :kr] = k * A / ne
    return GramReference(Gp, Bp, exact)


def ws_xty_reference(X, y, cols):
    """(c, c_bound, yy, yy_bound): c = -X_W^T y / n and yy = y^T y / 2n (the gradient and the loss at zero on W, as
    ws_xty_partial / ws_xty_apply_kernel write them), with the same style of bound."""
    X = np.asarray(X, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = X.shape[0]
    Xw = X[:, np.asarray(cols, dtype=np.int64)]
    exact = n * max(1, Xw.shape[1]) <= LONGDOUBLE_LIMIT
    dt = np.longdouble if exact else np.float64
    k = 2.0 * (n + 16) * EPS * (1.0 if exact else 2.0)
    c = -(Xw.astype(dt).T @ y.astype(dt)) / dt(n)
    yy = (y.astype(dt) @ y.astype(dt)) / dt(2 * n)
    return c, k * (np.abs(Xw).T @ np.abs(y)) / n, yy, k * float(y @ y) / (2 * n)


def gram_excess(G, ref: GramReference):
    """The largest |error| / bound over the entries (> 1: outside the bound; a padding entry that is not 0: inf)."""
    G = np.asarray(G, dtype=np.float64)
    err = np.abs(G.astype(np.longdouble) - ref.G).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(ref.bound > 0, err / ref.bound, np.where(err > 0, np.inf, 0.0))
    r = np.where(np.isnan(G), np.inf, r)
    return float(np.max(r))


def assert_gram_within_bound(G, ref: GramReference, what=""):
    e = gram_excess(G, ref)
    assert e <= 1.0, f"{what}: the Gram is outside the componentwise bound (largest error / bound {e})"


def assert_xty_within_bound(c, yy, ref, what=""):
    rc, bc, ryy, byy = ref
    ec = np.abs(np.asarray(c, dtype=np.float64).astype(np.longdouble) - rc).astype(np.float64)
    assert np.all(ec <= bc), f"{what}: X_W^T y outside the bound at positions {np.flatnonzero(ec > bc).tolist()[:8]}"
    assert abs(np.longdouble(yy) - ryy) <= byy, f"{what}: y^T y / 2n = {yy!r}, reference {float(ryy)!r}"


# ---- which kernels a call of slm_working_set_lanes launches (a mirror of engine_path.hip / engine_solve.hip) ----------------
SPLIT_RING = [(C, 3 if C < 5 else 2) for C in (1, 2, 3, 4, 5)]  # rowdot_ring_kernel<8, C, 5, D>: rows of up to 512 C columns


def ws_build_expected(k_end, route=1, xty=False, owner=False, sharded=False):
    """The build kernels: ws_block_owner_kernel once (lanes with row weights, unless SLM_NO_GRAM_OWNER; never on a
    row-sharded dataset), then per build gather (+ xty) + Gram + reduce -- or ws_gram_cov_kernel under covariance passes.
    Row-sharded: the reduce stages this rank's part, and ws_publish_kernel follows the all-reduce of the staging matrix."""
    names = ["ws_block_owner_kernel"] if owner and route == 1 and not sharded else []
    for _ in k_end:
        if route == 2:
            names.append("ws_gram_cov_kernel")
        else:
            names += ["ws_gather_kernel"] + (["ws_xty_partial_kernel", "ws_xty_apply_kernel"] if xty else []) + \
                     ["ws_gram_kernel", "ws_gram_reduce_kernel"] + (["ws_publish_kernel"] if sharded else [])
    return names


def ws_pass_expected(p, B, resid_vec=False, ring=None):
    """The pass of route 1 with control blocks: the residuals from X (launch_rowdot: the ring kernel for up to five lanes,
    or SLM_ROWDOT_RING=1, where one covers p; the matrix-core kernels on the column-major copy otherwise), the residuals
    from W (resid_ws_kernel with SLM_RESID_VEC=1 for up to sixteen lanes, resid_mfma_kernel, resid32_mfma_kernel for
    more), then X^T R (launch_xtr)."""
    p2 = (p + 15) // 16 * 16 // 2
    ring_kernel = next((f"rowdot_ring_kernel<8,{C},5,{D}>" for C, D in SPLIT_RING if 512 * C >= p2), None)
    halves = 1 if B <= 16 else 2
    use_ring = ring_kernel is not None and halves == 1 and (ring == "1" if ring in ("0", "1") else B <= 5)
    if use_ring:
        rowdot = ring_kernel
    elif halves == 1:
        rowdot = "rowdot_mfma_kernel"
    else:
        rowdot = "rowdot18_mfma_kernel" if B <= 18 else "rowdot20_mfma_kernel" if B <= 20 else "rowdot32_mfma_kernel"
    if halves == 2:
        resid = "resid32_mfma_kernel"
    else:
        resid = "resid_ws_kernel<16>" if resid_vec else "resid_mfma_kernel"
    product = "xtr_mfma_kernel" if halves == 1 else \
        "xtr18_mfma_kernel" if B <= 18 else "xtr20_mfma_kernel" if B <= 20 else "xtr32_mfma_kernel"
    return [rowdot, resid, product]


def ws_gram_mapping(k_new, K):
    """ws_gram_kernel's mapping for a build: "row-split" (a fresh selection of up to 8 tiles, or an append, when the new
    tile rows are at most 16) or "generic"."""
    tile_lo, tiles = int(k_new) >> 4, int(K) >> 4
    return "row-split" if (tile_lo > 0 or tiles <= 8) and tiles - tile_lo <= 16 else "generic"
