"""The opening of a cold shared path on the fp32 image of its sample rows (csrc/sample_kernels.hpp).

Through ``slm_gradient_ex`` route 2 (``Dataset.sample_product``): the vector the opening hands to its provisional tail step,
``g = -X_s^T y / n_s`` over the first ``n // SLM_SAMPLE_DIV`` rows, against numpy on the float-rounded rows; the fall-back to the
fp64 rows where a float cannot hold X; what rewrites X or y; and whole paths against ``SLM_SAMPLE_F64=1`` (the fp64 sample) and
``SLM_NO_SAMPLE_START=1`` (no sample).

The bound of the product is derived, not measured: the kernels add n_s products per column in fp64, in some fixed order, with
one rounding per FMA and per addition of two partial sums -- at most n_s roundings of 2^-53 relative on any path from a term
to the result, so |error_j| <= n_s 2^-53 (|X32|^T |y|)_j / n_s to first order; numpy's own sum carries the same bound, the
scaling by 1 / n_s two more roundings: 4 n_s 2^-53 (|X32|^T |y|)_j / n_s covers both sides with room.  A product that read the
fp64 rows instead would miss it by orders of magnitude (a float's rounding is 2^-24 per term), so passing also shows that the
image was read."""
import numpy as np
import pytest

from sparselm_amd import _engine

pytestmark = pytest.mark.gpu

WS = _engine.FLAG_WORKING_SET
SHAPES = [(256, 1), (400, 3), (1000, 7), (4099, 130), (10000, 513), (6000, 4097)]
DIVISORS = (64, 4, 1)  # (ascending samples: the image is rebuilt larger twice)


@pytest.fixture(scope="module")
def eng():
    return _engine.get_engine(0)


def reference(Xs, ys):
    """-X_s^T y / n_s in fp64 and the bound of the module's docstring."""
    n_s = Xs.shape[0]
    ref = -(Xs.T @ ys) / n_s
    bound = 4.0 * n_s * 2.0 ** -53 * (np.abs(Xs).T @ np.abs(ys)) / n_s
    return ref, bound


def check(g, Xs, ys, what):
    ref, bound = reference(Xs, ys)
    err = np.abs(g - ref)
    worst = int(np.argmax(err - bound))
    print(f"{what}: worst error {err[worst]:.3e} against bound {bound[worst]:.3e}")
    assert np.all(np.isfinite(g)), what
    assert np.all(err <= bound), (what, worst, err[worst], bound[worst])


@pytest.mark.parametrize("n,p", SHAPES)
def test_product_on_the_image_against_numpy(eng, monkeypatch, n, p):
    rng = np.random.default_rng(n + p)
    X = rng.standard_normal((n, p)) * rng.uniform(0.1, 30.0, p)
    y = rng.standard_normal(n) * 7.0 + 1.0
    X32 = X.astype(np.float32).astype(np.float64)
    with eng.dataset(X, y) as ds:
        for div in DIVISORS:
            monkeypatch.setenv("SLM_SAMPLE_DIV", str(div))
            n_s = n // div
            g, loss = ds.sample_product()
            again, loss_again = ds.sample_product()
            check(g, X32[:n_s], y[:n_s], f"{n} x {p} / {div}")
            np.testing.assert_array_equal(g, again)
            assert loss == loss_again
            ys = y[:n_s]
            assert abs(loss - ys @ ys / (2 * n_s)) <= 4.0 * n_s * 2.0 ** -53 * (ys @ ys) / (2 * n_s)
        # the fp64 route of the same call reads X itself
        monkeypatch.setenv("SLM_SAMPLE_F64", "1")
        g64, _ = ds.sample_product()
        check(g64, X[:n_s], y[:n_s], f"{n} x {p} / {div}, fp64 rows")


@pytest.mark.parametrize("kind", ["overflow", "underflow"])
def test_designs_a_float_cannot_hold_keep_the_fp64_rows(eng, kind):
    rng = np.random.default_rng(5)
    n, p = 4099, 130
    X = rng.standard_normal((n, p))
    if kind == "overflow":
        X[17, 41] = 1e39  # finite, inf as a float
    else:
        X[:, 7] = 1e-50 * rng.uniform(1.0, 2.0, n) * rng.choice([-1.0, 1.0], n)  # zero as floats, throughout
    y = rng.standard_normal(n)
    with eng.dataset(X, y) as ds:
        g, _ = ds.sample_product()
        again, _ = ds.sample_product()
    n_s = n // 4
    check(g, X[:n_s], y[:n_s], kind)
    np.testing.assert_array_equal(g, again)
    if kind == "underflow":
        assert g[7] != 0.0


def test_the_product_follows_what_rewrites_x_and_y(eng):
    rng = np.random.default_rng(9)
    n, p = 4099, 130
    X = rng.standard_normal((n, p)) + rng.uniform(-3, 3, p)
    y = rng.standard_normal(n) + 2.0
    n_s = n // 4
    f32 = lambda A: A.astype(np.float32).astype(np.float64)
    with eng.dataset(X, y) as ds:
        g, _ = ds.sample_product()
        check(g, f32(X)[:n_s], y[:n_s], "before")
        xm, ym = ds.center()  # rewrites X (and y) in place
        Xc, yc = X - xm, y - ym
        g, _ = ds.sample_product()
        check(g, f32(Xc)[:n_s], yc[:n_s], "centred")
        y2 = rng.standard_normal(n) * 3.0
        ds.set_targets(y2)  # y only: the image stays
        g, _ = ds.sample_product()
        check(g, f32(Xc)[:n_s], y2[:n_s], "new targets")


def bench_law(rng, n, p, k):
    """bench.py's law: X ~ N(0, 1), k coefficients 100 U(0, 1), noise of sd 10."""
    X = rng.standard_normal((n, p))
    coef = np.zeros(p)
    coef[rng.choice(p, k, replace=False)] = 100.0 * rng.uniform(size=k)
    return X, X @ coef + 10.0 * rng.standard_normal(n)


@pytest.mark.parametrize("head", ["as drawn", "sorted by |y|"])
def test_paths_open_alike_on_the_image_and_on_the_fp64_rows(eng, monkeypatch, head):
    """n = 8 192, p = 300, 30 informative features, 24 alphas down to 1e-2 alpha_max, the engine's choice of lanes.  The path
    that opens on the image against the one on the fp64 sample: the same working set size, the same number of passes,
    converged, coefficients within 1e-6 of max |beta|.  Against the path without a sample: converged, the same coefficients,
    and ONE pass fewer -- what the sample start is for (test_working_set_gpu.py asserts the same of the fp64 sample); its
    working set is chosen from the gradient of all rows and need not have the same size.  Measured as drawn: 154 columns and
    2 passes on the image and on the fp64 sample, 149 and 3 without a sample, coefficients 3.8e-13 apart.  With rows sorted
    by |y| the head of the rows misleads either sample: the paths must still end in the same solutions."""
    rng = np.random.default_rng(31)
    X, y = bench_law(rng, 8192, 300, 30)
    if head != "as drawn":
        order = np.argsort(np.abs(y))
        X, y = np.ascontiguousarray(X[order]), y[order]
    amax = np.max(np.abs(X.T @ y)) / len(y)
    pts = [(a, 0, 0) for a in np.geomspace(amax, 1e-2 * amax, 24)]
    monkeypatch.setenv("SLM_SAMPLE_START_MIN_ROWS", "64")
    runs = {}
    with eng.dataset(X, y) as ds:
        for name, knob in (("image", None), ("fp64 sample", "SLM_SAMPLE_F64"), ("no sample", "SLM_NO_SAMPLE_START")):
            if knob:
                monkeypatch.setenv(knob, "1")
            runs[name] = ds.solve_path(pts, tol=1e-10, lanes=0, flags=WS)
            if knob:
                monkeypatch.delenv(knob)
    top = np.max(np.abs(runs["image"].betas))
    for name, r in runs.items():
        print(f"{head}, {name}: ws_columns {r.ws_columns} grad_launches {r.grad_launches} converged {r.converged} "
              f"max |beta - image| / max |beta| {np.max(np.abs(r.betas - runs['image'].betas)) / top:.3e}")
    new = runs["image"]
    assert new.converged
    for name in ("fp64 sample", "no sample"):
        old = runs[name]
        assert old.converged, name
        assert np.max(np.abs(new.betas - old.betas)) <= 1e-6 * top, name
    if head == "as drawn":
        assert new.ws_columns == runs["fp64 sample"].ws_columns
        assert new.grad_launches == runs["fp64 sample"].grad_launches
        assert new.grad_launches == runs["no sample"].grad_launches - 1
