"""The linear term of the model behind a row-sample pass, summed by the gather (csrc/ws_kernels.hpp, ws_gather_xty_kernel and
ws_xty_apply_kernel), through ``Dataset.ws_build(cols, ..., xty=True)``: ``c_k = -X_k^T y / n`` per position of W and the loss at
zero ``y^T y / 2n``, against numpy.

The bound is derived, not measured -- the one of tests/test_sample_f32_gpu.py, for this summation tree.  A term x_ik y_i enters
its thread's sum through one FMA (one rounding).  From there to the result lie: the FMAs of the thread's later row tiles (at most
ceil(n / 32 / row blocks) - 1), five additions of the shuffle tree over the 32 row lanes, the additions of the apply kernel --
at most ceil(row blocks / 256) + 3 within a slice, 31 over the slices --, and two roundings of the scaling by 1 / n.  An addition
of an exact zero does not round, and a path from one of n terms to the result passes at most n - 1 additions in which BOTH
operands hold terms, so at most min(n + 2, tree depth + 3) roundings of 2^-53 relative lie on any path, never more than 3 n:
|error_k| <= 3 n 2^-53 (|X_W|^T |y|)_k / n to first order.  The tree is no deeper than the n roundings that
test_sample_f32_gpu.py allows a kernel (for 33 000 rows: 2 + 5 + 8 + 31 + 2 = 48), so its figure stands unwidened:
4 n 2^-53 (|X_W|^T |y|)_k / n.  The reference is numpy in extended precision, whose own error is nil beside it: at 1 ... 3
rows, where n + 2 roundings are 3 n of the 4 n, the bound is all the kernel's.  The same holds for y^T y / 2n with |y|^T |y|
in place of (|X_W|^T |y|)_k.  X and y are drawn independently with mixed signs: |X_k^T y| is of order sqrt(n) where (|X_k|^T |y|) is of order n,
so the bound is a relative one of the terms, not of the result -- an entry of y or a row left out misses it by orders."""
import numpy as np
import pytest

from sparselm_amd import _engine

pytestmark = pytest.mark.gpu

P = 560
ROWS = [1, 31, 32, 33, 95, 33000]  # no full tile of 32, exact tiles, a ragged last tile, more tiles than the 1 024 row blocks
WIDTHS = [1, 15, 16, 17, 31, 32, 33, 112, 129, 512]  # one position, tile edges of 16 and 32, the headline, two blocks of the apply, the capacity
FUSED = ["ws_gather_xty_kernel", "ws_xty_apply_kernel", "ws_gram_kernel", "ws_gram_reduce_kernel"]
SEPARATE = ["ws_gather_kernel", "ws_xty_partial_kernel", "ws_xty_apply_kernel", "ws_gram_kernel", "ws_gram_reduce_kernel"]


@pytest.fixture(scope="module")
def eng():
    return _engine.get_engine(0)


def scrambled_columns(rng, p, k):
    """k distinct feature indices in scrambled order, made of runs of neighbouring indices (j, j + 1, j + 2, ...)."""
    starts = rng.permutation(np.arange(0, p - 4, 4))
    runs = [np.arange(s, s + int(rng.integers(1, 5))) for s in starts]
    cols = np.concatenate(runs)[: max(k, 1)]
    if cols.size < k:  # (the capacity: fill up with what the runs left out)
        rest = np.setdiff1d(np.arange(p), cols)
        cols = np.concatenate([cols, rng.permutation(rest)[: k - cols.size]])
    cols = rng.permutation(cols[:k])
    assert cols.size == k and np.unique(cols).size == k
    return cols.astype(np.int32)


def reference(X, y, cols):
    n = X.shape[0]
    Xw = X[:, cols].astype(np.longdouble)
    yl = y.astype(np.longdouble)
    c = -(Xw.T @ yl) / np.longdouble(n)
    c_bound = 4.0 * n * 2.0 ** -53 * (np.abs(X[:, cols]).T @ np.abs(y)) / n
    yy = (yl @ yl) / np.longdouble(2 * n)
    yy_bound = 4.0 * n * 2.0 ** -53 * float(y @ y) / (2 * n)
    return c, c_bound, yy, yy_bound


def check(r, X, y, cols, what):
    c, c_bound, yy, yy_bound = reference(X, y, cols)
    err = np.abs(r.xty.astype(np.longdouble) - c).astype(np.float64)
    worst = int(np.argmax(err - c_bound))
    print(f"{what}: worst error {err[worst]:.3e} against bound {c_bound[worst]:.3e}; loss error "
          f"{float(abs(np.longdouble(r.yy) - yy)):.3e} against {yy_bound:.3e}")
    assert np.all(np.isfinite(r.xty)) and np.isfinite(r.yy), what
    assert np.all(err <= c_bound), (what, worst, err[worst], c_bound[worst])
    assert abs(np.longdouble(r.yy) - yy) <= yy_bound, (what, r.yy, float(yy))
    assert r.touched_outside == 0, f"{what}: {r.touched_outside} entries of g outside W were written"


@pytest.mark.parametrize("n", ROWS)
def test_linear_term_from_the_gather_against_numpy(eng, n):
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, P)) * rng.uniform(0.1, 30.0, P)
    y = rng.standard_normal(n) * 7.0 + 0.5
    with eng.dataset(X, y) as ds:
        for k in WIDTHS:
            cols = scrambled_columns(rng, P, k)
            r = ds.ws_build(cols, xty=True)
            again = ds.ws_build(cols, xty=True)
            assert r.kernels.split(";")[:4] == FUSED, r.kernels
            check(r, X, y, cols, f"{n} rows, {k} columns")
            np.testing.assert_array_equal(r.xty, again.xty)
            assert r.yy == again.yy
        # a column outside W keeps what it held: the builds' own check (touched_outside) and, seen from outside, a position
        # past Kreal inside K (idx = -1: 17 columns pad to 32) gives the column next to W no value -- the gradient pass behind
        # the builds then writes the true gradient there, the same whether or not the builds summed X_W^T y
        cols = scrambled_columns(rng, P, 17)
        outside = int(np.setdiff1d(np.arange(P), cols)[0])
        with_term = ds.ws_build(cols, xty=True)
        without = ds.ws_build(cols, xty=False)
        assert with_term.G[0, outside] == without.G[0, outside]
        np.testing.assert_array_equal(with_term.G, without.G)
        np.testing.assert_array_equal(with_term.gram, without.gram)


def test_the_gather_still_gathers_and_appends_are_summed_whole(eng):
    n, k_end = 1000, [20, 45, 130]
    rng = np.random.default_rng(7)
    X = rng.standard_normal((n, P))
    y = rng.standard_normal(n) - 0.3
    cols = scrambled_columns(rng, P, k_end[-1])
    with eng.dataset(X, y) as ds:
        r = ds.ws_build(cols, k_end=k_end, xty=True, want_xw=True)
        assert r.kernels.split(";")[:12] == 3 * FUSED, r.kernels
        XW = np.zeros((n, r.K))
        XW[:, : k_end[-1]] = X[:, cols]
        np.testing.assert_array_equal(r.XW, XW)
        check(r, X, y, cols, "three stages")
        one = ds.ws_build(cols, xty=True)
        np.testing.assert_array_equal(r.xty, one.xty)  # (the sums of an append start at position 0: the same tree)
        # without the column-major copy the gather reads X and the partial sums keep their own launch
        x = ds.ws_build(cols, k_end=k_end, xty=True, gather_from_x=True, want_xw=True)
        assert x.kernels.split(";")[:15] == 3 * SEPARATE, x.kernels
        np.testing.assert_array_equal(x.XW, XW)
        check(x, X, y, cols, "three stages, gathered from X")
        # ... as working_set_lanes(xty=True) asks for on any dataset; both routes fold their partial sums in one apply kernel
        Z = np.zeros((1, P))
        s = ds.working_set_lanes(Z, cols, k_end, on_ws=[0], xty=True)
        assert s.kernels.split(";")[:15] == 3 * SEPARATE, s.kernels
        np.testing.assert_array_equal(s.xty, x.xty)
        assert s.yy == x.yy
