"""The working set's Gram and X_W^T y references and their bounds (tests/_gradient_reference.py) on their own, no GPU: correct
float64 Grams in the summation orders of the kernels pass, and each numpy "defective build" -- the mistakes a staged,
row-blocked, shared-owner Gram build can make -- is flagged.  What tests/test_working_set_lanes_gpu.py concludes from a
kernel passing rests on both directions.  Also the mirror of the kernel choice that file asserts."""

import numpy as np
import pytest

from _gradient_reference import (
    assert_gram_within_bound,
    assert_xty_within_bound,
    gram_excess,
    ws_build_expected,
    ws_gram_mapping,
    ws_gram_reference,
    ws_K,
    ws_pass_expected,
    ws_xty_reference,
)

N, P = 3001, 97
NBLK = 37  # row blocks of the "kernel" below (a remainder: 3001 = 37 * 81 + 4)


def _data(family, seed=5):
    rng = np.random.default_rng(seed)
    if family == "normal":
        X = rng.standard_normal((N, P))
        y = rng.standard_normal(N)
    else:  # ill-conditioned: columns 1e3 + N(0, 1)
        X = 1e3 + rng.standard_normal((N, P))
        y = 1e4 + rng.standard_normal(N)
    return rng, X, y


def _blocks(n, nblk):
    """The row blocks of ws_gram_kernel / ws_block_owner_kernel: n // nblk rows each, the first n % nblk one more."""
    base, rem = divmod(n, nblk)
    out, r0 = [], 0
    for b in range(nblk):
        r1 = r0 + base + (1 if b < rem else 0)
        out.append((r0, r1))
        r0 = r1
    return out


def _gram_blocked(X, cols, w, ne, nblk=NBLK, weight_on="left", dtype=np.float64, skip=(), twice=(), chains=4):
    """A Gram the way the kernels sum it: per row block, the weight on one factor, then the blocks' partials folded in
    `chains` interleaved chains ((s0 + s1) + (s2 + s3)) and scaled by 1/n_eff.  `skip` / `twice`: blocks left out / counted
    again (the owner table pointing nowhere, or at a block already summed)."""
    kr = len(cols)
    K = ws_K(kr)
    XW = np.zeros((X.shape[0], K), dtype=dtype)
    XW[:, :kr] = X[:, cols]
    w = w.astype(dtype)
    parts = []
    for b, (r0, r1) in enumerate(_blocks(X.shape[0], nblk)):
        A = XW[r0:r1]
        if weight_on == "left":
            P_ = (w[r0:r1, None] * A).T @ A
        else:
            P_ = A.T @ (A * w[r0:r1, None])
        if b in skip:
            P_ = np.zeros_like(P_)
        parts.append(P_)
        if b in twice:
            parts.append(P_)
    s = [np.zeros((K, K), dtype=dtype) for _ in range(chains)]
    for b, P_ in enumerate(parts):
        s[b % chains] += P_
    tot = s[0]
    for c in s[1:]:
        tot = tot + c
    return (tot * dtype(1.0 / ne)).astype(np.float64)


@pytest.fixture(params=["normal", "ill"])
def case(request):
    rng, X, y = _data(request.param)
    cols = rng.choice(P, 45, replace=False)  # (K = 48: a partial last tile)
    w = rng.uniform(0.0, 2.0, N)
    ne = 0.81 * N
    return X, y, cols, w, ne, ws_gram_reference(X, cols, w, ne)


def test_ws_K_pads_to_whole_tiles():
    assert [ws_K(k) for k in (1, 15, 16, 17, 111, 112, 500, 512)] == [16, 16, 16, 32, 112, 112, 512, 512]


def test_the_reference_pads_with_exact_zeros(case):
    X, y, cols, w, ne, ref = case
    kr = len(cols)
    assert ref.G.shape == (48, 48) and ref.exact
    assert np.all(ref.G[kr:] == 0) and np.all(ref.G[:, kr:] == 0) and np.all(ref.bound[kr:] == 0)
    assert np.all(ref.bound[:kr, :kr] > 0)


def test_correct_grams_in_the_kernels_orders_pass(case):
    X, y, cols, w, ne, ref = case
    for kw in ({}, {"weight_on": "right"}, {"chains": 1}, {"nblk": 1}, {"nblk": 256}, {"nblk": N}):
        assert_gram_within_bound(_gram_blocked(X, cols, w, ne, **kw), ref, f"a correct Gram {kw}")
    # numpy's own product, and the rows in reverse
    kr = len(cols)
    G = np.zeros((48, 48))
    G[:kr, :kr] = X[:, cols].T @ (w[:, None] * X[:, cols]) / ne
    assert_gram_within_bound(G, ref, "numpy")
    Xr, wr = X[::-1], w[::-1]
    G[:kr, :kr] = Xr[:, cols].T @ (wr[:, None] * Xr[:, cols]) / ne
    assert_gram_within_bound(G, ref, "reversed rows")


def test_a_row_block_summed_twice_is_flagged(case):
    X, y, cols, w, ne, ref = case
    assert gram_excess(_gram_blocked(X, cols, w, ne, twice=(7,)), ref) > 1


def test_a_dropped_row_block_is_flagged(case):
    X, y, cols, w, ne, ref = case
    for b in (0, 17, NBLK - 1):
        assert gram_excess(_gram_blocked(X, cols, w, ne, skip=(b,)), ref) > 1, b


def test_another_row_sets_weights_or_n_eff_are_flagged(case):
    X, y, cols, w, ne, ref = case
    rng = np.random.default_rng(9)
    fold = (rng.random(N) >= 0.2).astype(np.float64)
    assert gram_excess(_gram_blocked(X, cols, fold, ne), ref) > 1
    w2 = w.copy()
    w2[N // 2] = 0.0  # (one row of one fold: a mask that differs in one row)
    assert gram_excess(_gram_blocked(X, cols, w2, ne), ref) > 1
    assert gram_excess(_gram_blocked(X, cols, w, ne * (1 + 1e-9)), ref) > 1
    assert gram_excess(_gram_blocked(X, cols, w, float(N)), ref) > 1


def test_a_stale_tile_row_from_before_an_append_is_flagged(case):
    # an append at k_new = 40 (mid-tile): tile row 2 (positions 32..47) has to be rebuilt -- kept from the Gram of the first
    # 40 columns its entries against the new columns 40..44 are the old padding's zeros
    X, y, cols, w, ne, ref = case
    old = _gram_blocked(X, cols[:40], w, ne)
    new = _gram_blocked(X, cols, w, ne)
    assert gram_excess(new, ref) <= 1
    stale = new.copy()
    stale[32:48] = old[32:48]
    assert gram_excess(stale, ref) > 1
    # (the old block itself is the same numbers: what an append must keep)
    np.testing.assert_array_equal(old[:32, :32], new[:32, :32])


def test_an_unmirrored_entry_is_flagged(case):
    X, y, cols, w, ne, ref = case
    G = _gram_blocked(X, cols, w, ne)
    for val in (0.0, np.nan):
        bad = G.copy()
        bad[3, 40] = val  # (row 3 < row_lo = 32 of an append at 40: written only by the mirror)
        assert gram_excess(bad, ref) > 1, val


def test_nan_or_nonzero_padding_is_flagged(case):
    X, y, cols, w, ne, ref = case
    G = _gram_blocked(X, cols, w, ne)
    for i, j, val in ((46, 46, 1e-300), (0, 47, np.nan), (47, 0, -0.0 + 1e-310)):
        bad = G.copy()
        bad[i, j] = val
        assert gram_excess(bad, ref) > 1, (i, j, val)


def test_float32_accumulation_is_flagged(case):
    X, y, cols, w, ne, ref = case
    assert gram_excess(_gram_blocked(X, cols, w, ne, dtype=np.float32), ref) > 1


def test_a_gathered_column_off_by_one_position_is_flagged(case):
    X, y, cols, w, ne, ref = case
    shifted = cols.copy()
    shifted[20] = cols[21]  # (position 20 gathered from position 21's feature)
    assert gram_excess(_gram_blocked(X, shifted, w, ne), ref) > 1


def test_xty_reference_and_bound():
    rng, X, y = _data("normal")
    cols = rng.choice(P, 30, replace=False)
    ref = ws_xty_reference(X, y, cols)
    c = -(X[:, cols].T @ y) / N
    yy = float(y @ y) / (2 * N)
    assert_xty_within_bound(c, yy, ref, "numpy")
    with pytest.raises(AssertionError):
        assert_xty_within_bound(-(X[:-1, cols].T @ y[:-1]) / N, yy, ref, "a dropped row")
    with pytest.raises(AssertionError):
        assert_xty_within_bound(c, float(y[1:] @ y[1:]) / (2 * N), ref, "a dropped row of y^T y")
    c32 = (-(X[:, cols].astype(np.float32).T @ y.astype(np.float32)) / np.float32(N)).astype(np.float64)
    with pytest.raises(AssertionError):
        assert_xty_within_bound(c32, yy, ref, "float32")


# ---- the mirror of the kernel choice -------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,B,resid_vec,ring,expect", [
    (600, 1, False, None, ["rowdot_ring_kernel<8,1,5,3>", "resid_mfma_kernel", "xtr_mfma_kernel"]),
    (600, 5, True, None, ["rowdot_ring_kernel<8,1,5,3>", "resid_ws_kernel<16>", "xtr_mfma_kernel"]),
    (600, 5, False, "0", ["rowdot_mfma_kernel", "resid_mfma_kernel", "xtr_mfma_kernel"]),
    (600, 6, False, None, ["rowdot_mfma_kernel", "resid_mfma_kernel", "xtr_mfma_kernel"]),
    (600, 16, True, "1", ["rowdot_ring_kernel<8,1,5,3>", "resid_ws_kernel<16>", "xtr_mfma_kernel"]),
    (5000, 16, False, None, ["rowdot_mfma_kernel", "resid_mfma_kernel", "xtr_mfma_kernel"]),
    (5000, 17, True, None, ["rowdot18_mfma_kernel", "resid32_mfma_kernel", "xtr18_mfma_kernel"]),  # (SLM_RESID_VEC: 16 lanes at most)
    (5000, 18, False, None, ["rowdot18_mfma_kernel", "resid32_mfma_kernel", "xtr18_mfma_kernel"]),
    (5000, 20, False, None, ["rowdot20_mfma_kernel", "resid32_mfma_kernel", "xtr20_mfma_kernel"]),
    (5000, 21, False, None, ["rowdot32_mfma_kernel", "resid32_mfma_kernel", "xtr32_mfma_kernel"]),
    (3000, 3, False, None, ["rowdot_ring_kernel<8,3,5,3>", "resid_mfma_kernel", "xtr_mfma_kernel"]),
    (6000, 3, False, None, ["rowdot_mfma_kernel", "resid_mfma_kernel", "xtr_mfma_kernel"]),  # (no ring kernel beyond 5120)
])
def test_the_pass_mirror(p, B, resid_vec, ring, expect):
    assert ws_pass_expected(p, B, resid_vec, ring) == expect


def test_the_build_mirror():
    assert ws_build_expected([40]) == ["ws_gather_kernel", "ws_gram_kernel", "ws_gram_reduce_kernel"]
    assert ws_build_expected([40, 45], xty=True, owner=True) == \
        ["ws_block_owner_kernel"] + 2 * ["ws_gather_kernel", "ws_xty_partial_kernel", "ws_xty_apply_kernel", "ws_gram_kernel",
                                         "ws_gram_reduce_kernel"]
    assert ws_build_expected([40, 45, 50], route=2, owner=True) == 3 * ["ws_gram_cov_kernel"]


@pytest.mark.parametrize("k_new,K,mapping", [(0, 16, "row-split"), (0, 128, "row-split"), (0, 144, "generic"),
                                              (0, 512, "generic"), (112, 128, "row-split"), (111, 128, "row-split"),
                                              (17, 144, "row-split"), (16, 272, "row-split"), (16, 288, "generic"),
                                              (256, 512, "row-split"), (240, 512, "generic")])
def test_the_gram_mapping_mirror(k_new, K, mapping):
    assert ws_gram_mapping(k_new, K) == mapping
