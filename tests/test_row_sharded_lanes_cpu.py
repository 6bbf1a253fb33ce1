"""The premise of tests/test_row_sharded_lanes_gpu.py, no GPU: the whole-X references and bounds of
tests/_gradient_reference.py apply unchanged to what a row-sharded run computes.

A numpy emulation of the sharded sums: every rank forms the blocked partial Grams and gradients of ITS rows, scales them by
1 / n_eff (n_eff is the job's, not the rank's), and the parts are added in rank order (local_sum_kernel).  A Gram grows in
stages as the engine's does: a build stages the tile rows from row_lo = 16 (k_new // 16) on, with their mirror images, into
a zeroed staging matrix; the parts are summed; the publish moves every entry with i >= row_lo or j >= row_lo into the Gram
and keeps the old block.

Both directions, on every split and rank count the GPU file uses: the correct emulation is inside the bound (the extra
R - 1 additions and the scaling per part are covered by the bound's "any tree" and its factor to spare -- no extra term),
and each realistic fault of the multi-rank state machine is far outside it or breaks what must be exact."""

import numpy as np
import pytest

from _gradient_reference import (
    assert_gram_within_bound,
    assert_within_bound,
    excess,
    gram_excess,
    lanes_reference,
    ws_build_expected,
    ws_gram_reference,
    ws_K,
)
from _ranks import SPLITS, split_bounds

P = 61
K_END = [22, 45]  # an append at k_new = 22: row_lo = 16, mid-tile; K = 48 with a partial last tile
ALL_SPLITS = [(n, s) for n in (40, 1000, 4099, 333) for s in SPLITS[n]]
_ids = [f"{n}-" + ("8x125" if len(s) == 8 else "_".join(map(str, s))) for n, s in ALL_SPLITS]


def _data(n, family="normal", seed=3):
    rng = np.random.default_rng(seed + n)
    X = rng.standard_normal((n, P)) + (1e3 if family == "ill" else 0.0)
    y = rng.standard_normal(n) + (1e4 if family == "ill" else 0.0)
    cols = rng.choice(P, K_END[-1], replace=False)
    w = rng.uniform(0.0, 2.0, n)
    return rng, X, y, cols, w, 0.81 * n


def _row_blocks(n):
    """Row blocks of a rank with n rows (ws_row_blocks: one per 64 rows, at least one)."""
    nblk = max(1, n // 64)
    base, rem = divmod(n, nblk)
    out, r0 = [], 0
    for b in range(nblk):
        r1 = r0 + base + (1 if b < rem else 0)
        out.append((r0, r1))
        r0 = r1
    return out


def _part(X, w, cols, K, inv_n):
    """One rank's Gram part: blocked partial sums folded in four interleaved chains, then scaled (ws_gram_reduce_kernel)."""
    XW = np.zeros((X.shape[0], K))
    XW[:, :len(cols)] = X[:, cols]
    s = [np.zeros((K, K)) for _ in range(4)]
    for b, (r0, r1) in enumerate(_row_blocks(X.shape[0])):
        s[b % 4] += (w[r0:r1, None] * XW[r0:r1]).T @ XW[r0:r1]
    return ((s[0] + s[1]) + (s[2] + s[3])) * inv_n


def sharded_gram(X, w, cols, k_end, ne, split, fault=None):
    """The staged, published Gram of a sharded run (docstring above).  `fault`: one defect of the state machine."""
    G = np.full((512, 512), np.nan)  # (what no publish has written shows)
    k_old = 0
    for k1 in k_end:
        K, row_lo = ws_K(k1), (k_old // 16) * 16
        new = np.zeros((K, K), dtype=bool)
        new[row_lo:, :] = True
        new[:, row_lo:] = True  # the tile rows from row_lo on and their mirror images
        parts = []
        for r, (lo, hi) in enumerate(split_bounds(split)):
            wr = w[:hi - lo] if fault == "other_slice" else w[lo:hi]  # (a rank that forgets its row offset)
            inv_n = 1.0 / (hi - lo) if fault == "own_rows" else 1.0 / ne
            part = _part(X[lo:hi], wr, cols[:k1], K, inv_n)
            part[:row_lo, row_lo:] = part[row_lo:, :row_lo].T  # (the mirror is a copy of the entry: ws_gram_reduce_kernel)
            staged = np.where(new, part, 0.0)  # (zeroed staging, this build's entries)
            parts.append(staged)
        if fault == "dropped":
            parts = parts[:-1]
        if fault == "twice":
            parts = parts + parts[-1:]
        tot = parts[0].copy() if parts else np.zeros((K, K))
        for part in parts[1:]:  # fixed rank order (local_sum_kernel)
            tot = tot + part
        move = new.copy()
        if fault == "old_from_staging":
            move[:] = True
        if fault == "no_mirror":
            move[:row_lo, :] = False
        if fault == "and_corner":  # (the publish condition written with &&)
            move = np.zeros((K, K), dtype=bool)
            move[row_lo:, row_lo:] = True
        G[:K, :K] = np.where(move, tot, G[:K, :K])
        k_old = k1
    K = ws_K(k_end[-1])
    return G[:K, :K].copy()


def sharded_lanes(X, y, Z, W, ne, split, fault=None):
    """Gradients and losses of a sharded pass: every rank's sums over its rows scaled by 1 / n_eff, added in rank order."""
    parts = []
    for lo, hi in split_bounds(split):
        Wr = W[:, :hi - lo] if fault == "other_slice" else W[:, lo:hi]
        scale = np.full(len(ne), float(hi - lo)) if fault == "own_rows" else ne
        R = X[lo:hi] @ Z.T - y[lo:hi, None]
        parts.append(((X[lo:hi].T @ (Wr.T * R)).T / scale[:, None], np.sum(Wr.T * R * R, axis=0) / (2 * scale)))
    if fault == "dropped":
        parts = parts[:-1]
    if fault == "twice":
        parts = parts + parts[-1:]
    g, loss = np.zeros((len(ne), X.shape[1])), np.zeros(len(ne))
    for gp, lp in parts:
        g, loss = g + gp, loss + lp
    return g, loss


@pytest.mark.parametrize("family", ["normal", "ill"])
@pytest.mark.parametrize("n,split", ALL_SPLITS, ids=_ids)
def test_the_sharded_sums_are_inside_the_whole_x_bounds(n, split, family):
    rng, X, y, cols, w, ne = _data(n, family)
    assert sum(split) == n
    for k_end in (K_END, [K_END[-1]]):
        G = sharded_gram(X, w, cols, k_end, ne, split)
        assert_gram_within_bound(G, ws_gram_reference(X, cols, w, ne), f"{len(split)} ranks, stages {k_end}")
    # the old block is that of the stage before, bit for bit; the mirror is exact
    G = sharded_gram(X, w, cols, K_END, ne, split)
    assert np.array_equal(G[:16, :16], sharded_gram(X, w, cols, K_END[:1], ne, split)[:16, :16])
    assert np.array_equal(G[:16, 16:], G[16:, :16].T)
    Z = rng.standard_normal((3, P)) * np.array([1.0, 1e6, 0.0])[:, None]
    W = np.stack([w, (rng.random(n) >= 0.2).astype(np.float64), np.ones(n)])
    nes = np.array([ne, float(n), 0.73 * n + 1.5])
    g, loss = sharded_lanes(X, y, Z, W, nes, split)
    assert_within_bound(g, loss, lanes_reference(X, y, Z, W, nes), f"{len(split)} ranks")


GRAM_FAULTS = ["dropped", "twice", "own_rows", "old_from_staging", "no_mirror", "other_slice", "and_corner"]


@pytest.mark.parametrize("fault", GRAM_FAULTS)
@pytest.mark.parametrize("n,split", ALL_SPLITS, ids=_ids)
def test_a_faulty_gram_exchange_is_flagged(n, split, fault):
    rng, X, y, cols, w, ne = _data(n)
    ref = ws_gram_reference(X, cols, w, ne)
    good = sharded_gram(X, w, cols, K_END, ne, split)
    bad = sharded_gram(X, w, cols, K_END, ne, split, fault)
    prev = sharded_gram(X, w, cols, K_END[:1], ne, split)
    # what the GPU file asserts of a Gram: inside the bound (no NaN, padding 0), the old block kept bit for bit
    flagged = gram_excess(bad, ref) > 1 or not np.array_equal(bad[:16, :16], prev[:16, :16])
    assert flagged, f"{fault} with {len(split)} ranks passes every check"
    assert gram_excess(good, ref) <= 1


@pytest.mark.parametrize("fault", ["dropped", "twice", "own_rows", "other_slice"])
@pytest.mark.parametrize("n,split", ALL_SPLITS, ids=_ids)
def test_a_faulty_gradient_exchange_is_flagged(n, split, fault):
    rng, X, y, cols, w, ne = _data(n)
    Z = rng.standard_normal((2, P))
    W = np.stack([w, rng.uniform(0.0, 2.0, n)])
    nes = np.array([ne, float(n)])
    g, loss = sharded_lanes(X, y, Z, W, nes, split, fault)
    assert np.all(excess(g, loss, lanes_reference(X, y, Z, W, nes)) > 1), fault


def test_lanes_that_differ_on_one_ranks_rows_are_two_sets_everywhere():
    """The agreement the diagnostic needs: "the same on my rows" per rank, and one set only where every rank said so."""
    n, split = 1000, (63, 1, 936)
    rng = np.random.default_rng(0)
    W = np.tile(rng.uniform(0.0, 2.0, n), (3, 1))
    W[1, 5] += 0.5  # lanes 0 and 1 differ on rank 0's rows only; lane 2 is lane 0's set
    local = [np.array([[np.array_equal(W[a, lo:hi], W[b, lo:hi]) for b in range(3)] for a in range(3)], dtype=float)
             for lo, hi in split_bounds(split)]
    assert local[1].all() and local[2].all() and not local[0].all()  # (decided locally: ranks 1 and 2 see ONE set)
    agreed = sum(local) == len(split)
    assert agreed.tolist() == [[True, False, True], [False, True, False], [True, False, True]]


def test_the_build_mirror_of_a_sharded_call():
    assert ws_build_expected([40, 45], owner=True, sharded=True) == \
        2 * ["ws_gather_kernel", "ws_gram_kernel", "ws_gram_reduce_kernel", "ws_publish_kernel"]
