"""The opening's sample product (csrc/sample_kernels.hpp, sample_xty_kernel<U = 8>: a thread's rows in batches of U loads, the
rows that fill no batch in a loop of their own behind them) at the row counts where the first batch or the tail can go wrong --
the sizes any other scheduling of the loads (two alternating register sets were tried, profiles/opening_reads/) has to pass
too -- and whole paths that open on it.

A thread walks ALL rows of its row block, so what matters is the number of rows PER ROW BLOCK: exactly 1, U - 1, U, U + 1,
2 U - 1, 2 U, 2 U + 1 and 3 U + 1.  slm_host::sample_plan (csrc/host_logic.hpp; tests/sample_plan_test.cpp walks it) gives a row
block max(16, ceil(n_s / want)) rows with want = 4 CUs / column blocks, and the last block what is left.  So:
  * up to 2 U = 16 rows per block: n_s = r (one block of r rows) and n_s = 32 + r (two blocks of 16 and one of r),
  * 2 U + 1 and 3 U + 1: n_s = want * r on 4 097 columns (five column blocks), where every block holds exactly r rows.
``plan_rows`` below mirrors the plan for the shapes used and the test asserts the row counts it means to reach.

Reference and bound are those of tests/test_sample_f32_gpu.py: numpy on the float-rounded rows; at most n_s roundings of 2^-53 lie
on any path from a term to the result (one FMA per row, in row order, then the
fixed-order sums of sample_finish_kernel), so |error_j| <= 4 n_s 2^-53 (|X32|^T |y|)_j / n_s covers the kernel and numpy."""
import numpy as np
import pytest

from sparselm_amd import _engine

pytestmark = pytest.mark.gpu

WS = _engine.FLAG_WORKING_SET
U = 8  # engine_solve.hip launches sample_xty_kernel<8>
THREADS, WGS_PER_CU, MIN_ROWS = 256, 4, 16  # slm_host::kSampleThreads, kSampleWgsPerCu, kSampleMinRows


@pytest.fixture(scope="module")
def eng():
    return _engine.get_engine(0)


def plan_rows(n_s, p, cus):
    """(rows per row block, rows of the last block) of slm_host::sample_plan."""
    quads = (p + 3) // 4
    xb = max(1, -(-quads // THREADS))
    want = max(1, WGS_PER_CU * max(1, cus) // xb)
    rows = max(MIN_ROWS, -(-n_s // want))
    yb = -(-n_s // rows)
    return rows, n_s - (yb - 1) * rows, want


def check(g, loss, Xs, ys, what):
    n_s = Xs.shape[0]
    ref = -(Xs.T @ ys) / n_s
    bound = 4.0 * n_s * 2.0 ** -53 * (np.abs(Xs).T @ np.abs(ys)) / n_s
    err = np.abs(g - ref)
    worst = int(np.argmax(err - bound))
    print(f"{what}: worst error {err[worst]:.3e} against bound {bound[worst]:.3e}")
    assert np.all(np.isfinite(g)), what
    assert np.all(err <= bound), (what, worst, err[worst], bound[worst])
    assert abs(loss - ys @ ys / (2 * n_s)) <= 4.0 * n_s * 2.0 ** -53 * (ys @ ys) / (2 * n_s), what


def product(eng, monkeypatch, X, y):
    """The sample product over ALL rows of (X, y) (SLM_SAMPLE_DIV=1), twice; asserts repeatability."""
    monkeypatch.setenv("SLM_SAMPLE_DIV", "1")
    with eng.dataset(X, y) as ds:
        g, loss = ds.sample_product()
        again, loss_again = ds.sample_product()
    np.testing.assert_array_equal(g, again)
    assert loss == loss_again
    return g, loss


@pytest.mark.parametrize("r", [1, U - 1, U, U + 1, 2 * U - 1, 2 * U])
@pytest.mark.parametrize("full_blocks", [0, 2])
def test_row_blocks_of_up_to_two_batches(eng, monkeypatch, r, full_blocks):
    p = 130  # (not a multiple of four: the image pads the row)
    n_s = 16 * full_blocks + r
    rows, last, _ = plan_rows(n_s, p, eng.device_info()["compute_units"])
    assert rows == 16 and last == r, (rows, last)
    rng = np.random.default_rng(100 * r + full_blocks)
    X = rng.standard_normal((n_s, p)) * rng.uniform(0.1, 30.0, p)
    y = rng.standard_normal(n_s) * 7.0 + 1.0
    g, loss = product(eng, monkeypatch, X, y)
    check(g, loss, X.astype(np.float32).astype(np.float64), y, f"{n_s} rows, last block {r}")


@pytest.mark.parametrize("r", [2 * U + 1, 3 * U + 1])
def test_row_blocks_of_more_than_two_batches(eng, monkeypatch, r):
    p = 4097  # five column blocks, the last one a single thread wide
    cus = eng.device_info()["compute_units"]
    want = plan_rows(1, p, cus)[2]
    n_s = want * r
    rows, last, _ = plan_rows(n_s, p, cus)
    assert rows == r and last == r, (rows, last)
    rng = np.random.default_rng(r)
    X = rng.standard_normal((n_s, p)) * 3.0
    y = rng.standard_normal(n_s) * 7.0 + 1.0
    g, loss = product(eng, monkeypatch, X, y)
    check(g, loss, X.astype(np.float32).astype(np.float64), y, f"{n_s} rows in blocks of {r}")


def bench_law(rng, n, p, k):
    """bench.py's law: X ~ N(0, 1), k coefficients 100 U(0, 1), noise of sd 10 (as in tests/test_sample_f32_gpu.py)."""
    X = rng.standard_normal((n, p))
    coef = np.zeros(p)
    coef[rng.choice(p, k, replace=False)] = 100.0 * rng.uniform(size=k)
    return X, X @ coef + 10.0 * rng.standard_normal(n)


def test_a_path_that_opens_on_the_sample_saves_a_pass_and_ends_alike(eng, monkeypatch):
    """n = 8 192, p = 300, 30 informative features, 24 alphas down to 1e-2 alpha_max -- the problem of
    test_paths_open_alike_on_the_image_and_on_the_fp64_rows.  The path that opens on the sample (the product on the image, then
    the build whose gather sums the model's linear term) against the one that opens on all rows: both converge, the first with one
    pass fewer, coefficients within 1e-6 of max |beta|."""
    rng = np.random.default_rng(31)
    X, y = bench_law(rng, 8192, 300, 30)
    amax = np.max(np.abs(X.T @ y)) / len(y)
    pts = [(a, 0, 0) for a in np.geomspace(amax, 1e-2 * amax, 24)]
    monkeypatch.setenv("SLM_SAMPLE_START_MIN_ROWS", "64")
    monkeypatch.delenv("SLM_NO_SAMPLE_START", raising=False)
    with eng.dataset(X, y) as ds:
        sample = ds.solve_path(pts, tol=1e-10, lanes=0, flags=WS)
        monkeypatch.setenv("SLM_NO_SAMPLE_START", "1")
        plain = ds.solve_path(pts, tol=1e-10, lanes=0, flags=WS)
    top = np.max(np.abs(sample.betas))
    print(f"sample start: {sample.grad_launches} passes, {sample.ws_columns} columns; all rows: {plain.grad_launches} passes, "
          f"{plain.ws_columns} columns; max |beta - beta'| / max |beta| {np.max(np.abs(sample.betas - plain.betas)) / top:.3e}")
    assert sample.converged and plain.converged
    assert sample.grad_launches == plain.grad_launches - 1
    assert np.max(np.abs(sample.betas - plain.betas)) <= 1e-6 * top
