"""Every multi-lane gradient kernel, lane by lane, with distinct inputs per lane (slm_gradient_lanes).

Each case gives every lane its own point (dense, three non-zeros, zero, x 1e6, x 1e-6), its own row weights (a fold mask,
uniform(0, 2), ones, only the last row, none on the last row block) and its own n_eff, and asserts for every lane:
  1. the kernels the engine reports are the ones this file's mirror of the kernel tables (engine_solve.hip) expects; a call
     no kernel serves raises NotImplementedError -- the entry point never falls back to another route;
  2. the componentwise float64 bound of tests/_gradient_reference.py on G and on the loss (and, on standard normal data, the
     suite's rel-inf < 1e-12 / rtol 1e-12);
  3. lane independence: with the other lanes' points, weights and n_eff replaced, the lane's G and loss keep their bits
     (every MFMA output element and every per-lane accumulator depends on its own lane only);
  4. determinism: the same call twice gives the same bits.
"""

import numpy as np
import numpy.testing as npt
import pytest

from _gradient_reference import assert_within_bound, gram_reference, lane_inputs, lanes_reference
from sparselm_amd import _engine

pytestmark = pytest.mark.gpu

# ---- a mirror of the kernel tables of engine_solve.hip (pick_grad_kernel, pick_split_kernel, launch_rowdot, launch_xtr) ----
GRAD_RING = [(8, C, B, 3 if C < 5 else 2) for B in (1, 2, 3, 4) for C in (1, 2, 3, 4, 5)] + \
            [(8, C, 5, 3) for C in (1, 2, 3, 4)] + [(8, C, 6, 3) for C in (1, 2, 3)]  # (W, C, B, D)
GRAD_DEFAULT = [  # (W, C, R, B)
    (1, 1, 4, 1), (2, 1, 4, 1), (4, 1, 4, 1), (8, 1, 4, 1), (8, 2, 4, 1), (8, 3, 4, 1), (8, 4, 2, 1), (8, 5, 2, 1), (8, 6, 2, 1),
    (8, 8, 2, 1), (8, 10, 1, 1),
    (1, 1, 4, 2), (2, 1, 4, 2), (4, 1, 4, 2), (8, 1, 4, 2), (8, 2, 4, 2), (8, 3, 4, 2), (8, 4, 2, 2), (8, 5, 2, 2), (8, 6, 2, 2),
    (8, 8, 1, 2),
    (1, 1, 4, 3), (2, 1, 4, 3), (4, 1, 4, 3), (8, 1, 4, 3), (8, 2, 4, 3), (8, 3, 4, 3), (8, 4, 2, 3), (8, 5, 2, 3), (8, 6, 1, 3),
    (1, 1, 4, 4), (2, 1, 4, 4), (4, 1, 4, 4), (8, 1, 4, 4), (8, 2, 4, 4), (8, 3, 2, 4), (8, 4, 2, 4), (8, 5, 1, 4),
]
SPLIT_RING = [(C, 3 if C < 5 else 2) for C in (1, 2, 3, 4, 5)]  # rowdot_ring_kernel<8, C, 5, D>
TWO_PASS = "rowdot_kernel;xtr_kernel<4>"
ROWDOT_MFMA = ["rowdot_mfma_kernel", "rowdot18_mfma_kernel", "rowdot20_mfma_kernel", "rowdot32_mfma_kernel"]
XTR_MFMA = ["xtr_mfma_kernel", "xtr18_mfma_kernel", "xtr20_mfma_kernel", "xtr32_mfma_kernel"]
COV_GZ = ["cov_gz_mfma_kernel", "cov_gz32_mfma_kernel"]
ALL_KERNELS = ({f"grad_ring_kernel<{W},{C},{B},{D}>" for W, C, B, D in GRAD_RING}
               | {f"grad_fused_kernel<{W},{C},{R},{B}>" for W, C, R, B in GRAD_DEFAULT}
               | {f"rowdot_ring_kernel<8,{C},5,{D}>" for C, D in SPLIT_RING}
               | set(TWO_PASS.split(";")) | set(ROWDOT_MFMA) | set(XTR_MFMA) | set(COV_GZ))


def _p2(p):
    return (p + 15) // 16 * 16 // 2


def fused_expected(p, B, ring=None):
    """pick_grad_kernel: the name of route 0's kernel for (p, B) under SLM_GRAD_RING=`ring`, None where there is none."""
    p2 = _p2(p)
    if p2 > 5120:
        return TWO_PASS if B == 1 else None
    if ring != "0" and p2 > 256 and (B >= 3 or ring == "1"):
        for W, C, b, D in GRAD_RING:
            if b == B and 64 * W * C >= p2:
                return f"grad_ring_kernel<{W},{C},{B},{D}>"
    for W, C, R, b in GRAD_DEFAULT:
        if b == B and 64 * W * C >= p2:
            return f"grad_fused_kernel<{W},{C},{R},{B}>"
    return None


def split_expected(p, B, ring=None):
    """launch_rowdot + launch_xtr for route 1 (the column-major copy built): "residual;product"."""
    p2 = _p2(p)
    ring_kernel = next((f"rowdot_ring_kernel<8,{C},5,{D}>" for C, D in SPLIT_RING if 512 * C >= p2), None)
    halves = 1 if B <= 16 else 2
    use_ring = ring_kernel is not None and halves == 1 and (ring == "1" if ring in ("0", "1") else B <= 5)
    if use_ring:
        resid = ring_kernel
    elif halves == 1:
        resid = "rowdot_mfma_kernel"
    else:
        resid = "rowdot18_mfma_kernel" if B <= 18 else "rowdot20_mfma_kernel" if B <= 20 else "rowdot32_mfma_kernel"
    product = "xtr_mfma_kernel" if halves == 1 else \
        "xtr18_mfma_kernel" if B <= 18 else "xtr20_mfma_kernel" if B <= 20 else "xtr32_mfma_kernel"
    return f"{resid};{product}"


def cov_expected(B):
    return "cov_gz_mfma_kernel" if B <= 16 else "cov_gz32_mfma_kernel"


# ---- the cases -----------------------------------------------------------------------------------------------------------
P_EDGES = [128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 3072, 3073, 4096, 4097, 5120, 5121, 6144, 6145, 8192, 8193,
           10240]
N_CYCLE = [1, 3, 5, 7, 257, 4099]  # (one row; R - 1, R + 1 around the rows per step; a few rows per block; many)
ROUTE0 = [(p, B, ring) for ring in (None, "0", "1") for p in P_EDGES for B in range(1, 7)] + \
         [(p, 1, None) for p in (10241, 20000)] + [(p, B, None) for p in (10241, 20000) for B in (2, 7)] + \
         [(600, 7, None), (40, 7, "1")]
SPLIT_SHAPES = [(1, 1), (7, 40), (31, 600), (33, 1537), (65, 3000), (129, 4096), (4099, 600), (20011, 40), (257, 5120),
                (513, 5121), (300, 10000), (130, 20000)]
SPLIT_B = (1, 2, 5, 6, 11, 15, 16, 17, 18, 19, 20, 21, 31, 32)
ROUTE1 = [(n, p, B, ring) for n, p in SPLIT_SHAPES for B in SPLIT_B for ring in ((None, "0", "1") if B <= 16 else (None,))] + \
         [(33, 1537, 17, "1"), (4099, 600, 32, "1")]  # (forcing the ring kernel leaves more than sixteen lanes on the mfma kernels)


def _n_for(p, i):
    n = N_CYCLE[i % len(N_CYCLE)]
    return min(n, 257) if p > 4096 else n  # (wide rows: the long double reference stays quick)


def _data(n, p, seed, family="normal"):
    rng = np.random.default_rng(seed)
    if family == "normal":
        return rng.standard_normal((n, p)), rng.standard_normal(n)
    return 1e3 + rng.standard_normal((n, p)), 1e4 + rng.standard_normal(n)


def _set_env(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


@pytest.fixture(scope="module")
def eng():
    return _engine.get_engine(0)


def rel_inf(a, b):
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def check_lanes(ds, X, y, route, B, expect, seed, n_rows=0, family="normal", cov_index=None, refs=None):
    """One case: every lane's own inputs through `route`; assertions 1-4 of the module docstring.  Returns the kernels."""
    n, p = X.shape
    rng = np.random.default_rng(seed)
    Z, W, ne = lane_inputs(rng, n, p, B, n_rows)
    if route == 2:
        W = ne = None
    call = lambda Z, W, ne: ds.gradient_lanes(Z, W, ne, route=route, cov_index=cov_index, n_rows=n_rows)  # noqa: E731
    if expect is None:
        with pytest.raises(NotImplementedError):
            call(Z, W, ne)
        return None
    G, loss, names = call(Z, W, ne)
    assert names == expect, (route, n, p, B, names, expect)
    if route == 2:
        for l in range(B):
            ref_x, ref_g = refs(cov_index[l], Z[l:l + 1])
            assert_within_bound(G[l:l + 1], loss[l:l + 1], ref_x, f"lane {l} against X")
            assert_within_bound(G[l:l + 1], loss[l:l + 1], ref_g, f"lane {l} against the engine's Gram")
    else:
        ref = lanes_reference(X, y, Z, W, ne, n_rows)
        assert_within_bound(G, loss, ref, f"route {route} {names} n={n} p={p} B={B} n_rows={n_rows}")
        if family == "normal":
            for l in range(B):
                assert rel_inf(G[l], ref.g[l].astype(np.float64)) < 1e-12, l
                npt.assert_allclose(loss[l], float(ref.loss[l]), rtol=1e-12, atol=1e-300)
    G2, loss2, _ = call(Z, W, ne)
    assert np.array_equal(G, G2) and np.array_equal(loss, loss2), "not deterministic"
    if B > 1:  # lanes of one parity keep their inputs, the others get fresh ones (fresh kinds, fresh draws)
        Zf, Wf, nef = lane_inputs(np.random.default_rng(seed + 7919), n, p, B, n_rows, offset=2)
        for keep in (np.arange(B) % 2 == 0, np.arange(B) % 2 == 1):
            Zk = np.where(keep[:, None], Z, Zf)
            Wk = None if W is None else np.where(keep[:, None], W, Wf)
            nek = None if ne is None else np.where(keep, ne, nef)
            G3, loss3, _ = call(Zk, Wk, nek)
            assert np.array_equal(G3[keep], G[keep]) and np.array_equal(loss3[keep], loss[keep]), \
                f"lanes {np.flatnonzero(keep).tolist()} changed with the other lanes' inputs"
    return names


# ---- route 0: the fused one-read kernels (register and LDS-ring forms), the two-pass pair ---------------------------------
@pytest.mark.parametrize("p,B,ring", ROUTE0)
def test_fused_kernels_lane_by_lane(eng, monkeypatch, p, B, ring):
    _set_env(monkeypatch, "SLM_GRAD_RING", ring)  # (read when the dataset picks its kernel table)
    n = _n_for(p, P_EDGES.index(p) if p in P_EDGES else B)
    X, y = _data(n, p, p * 131 + B)
    with eng.dataset(X, y) as ds:
        check_lanes(ds, X, y, 0, B, fused_expected(p, B, ring), seed=p * 7 + B)


# ---- route 1: the split pass (residual kernels, then X^T R for every lane slot) -------------------------------------------
@pytest.mark.parametrize("n,p,B,ring", ROUTE1)
def test_split_kernels_lane_by_lane(eng, monkeypatch, n, p, B, ring):
    _set_env(monkeypatch, "SLM_ROWDOT_RING", ring)
    X, y = _data(n, p, n * 31 + p)
    with eng.dataset(X, y) as ds:
        check_lanes(ds, X, y, 1, B, split_expected(p, B, ring), seed=n + p * 3 + B)


@pytest.mark.parametrize("n,p", [(4099, 600), (20011, 40)])
@pytest.mark.parametrize("B", [1, 16])
def test_split_kernels_with_two_xtr_workgroups_per_cu(eng, monkeypatch, n, p, B):
    monkeypatch.setenv("SLM_XTR_WGS_PER_CU", "2")
    X, y = _data(n, p, n + p)
    with eng.dataset(X, y) as ds:
        check_lanes(ds, X, y, 1, B, split_expected(p, B), seed=B + 5)


# ---- the first rows only (sketch and sample starts) ------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(4099, 600), (257, 1537)])
@pytest.mark.parametrize("frac", ["one", "quarter", "all_but_one"])
@pytest.mark.parametrize("route,B,ring", [(0, 1, None), (0, 4, None), (0, 6, None), (0, 2, "1"), (1, 5, None), (1, 11, "1"),
                                          (1, 16, None), (1, 18, None), (1, 32, None)])
def test_first_rows_lane_by_lane(eng, monkeypatch, n, p, frac, route, B, ring):
    _set_env(monkeypatch, "SLM_GRAD_RING" if route == 0 else "SLM_ROWDOT_RING", ring)
    n_rows = {"one": 1, "quarter": n // 4, "all_but_one": n - 1}[frac]
    X, y = _data(n, p, n + p + 1)
    expect = fused_expected(p, B, ring) if route == 0 else split_expected(p, B, ring)
    with eng.dataset(X, y) as ds:
        check_lanes(ds, X, y, route, B, expect, seed=n_rows + B, n_rows=n_rows)


# ---- ill-conditioned data: columns 1e3 + N(0, 1), y of mean 1e4 ------------------------------------------------------------
@pytest.mark.parametrize("route,n,p,B,ring", [(0, 4099, 600, 1, None), (0, 257, 2049, 3, None), (0, 257, 5000, 4, "0"),
                                              (0, 513, 1000, 6, None), (0, 300, 10241, 1, None), (1, 4099, 600, 5, None),
                                              (1, 4099, 600, 11, "1"), (1, 2000, 1537, 16, None), (1, 513, 5121, 18, None),
                                              (1, 4099, 600, 20, None), (1, 300, 10000, 32, None)])
def test_ill_conditioned_data_lane_by_lane(eng, monkeypatch, route, n, p, B, ring):
    _set_env(monkeypatch, "SLM_GRAD_RING" if route == 0 else "SLM_ROWDOT_RING", ring)
    X, y = _data(n, p, n * 3 + p, family="ill")
    expect = fused_expected(p, B, ring) if route == 0 else split_expected(p, B, ring)
    with eng.dataset(X, y) as ds:
        check_lanes(ds, X, y, route, B, expect, seed=n + B, family="ill")


# ---- route 2: the covariance route (cov_gz*_mfma_kernel + cov_reduce + cov_loss over the folds' Grams) ----------------------
def _cov_dataset(eng, X, y, K, seed):
    n, p = X.shape
    fold = np.random.default_rng(seed).integers(0, K, n)
    masks = [(fold != k).astype(np.float64) for k in range(K)]
    ds = eng.dataset(X, y)
    ds.covariance_folds(masks, [int(m.sum()) for m in masks])
    assert ds.covariance_count() == K
    entries = []
    for e in range(K):
        G, c, sc = ds.covariance_download(e)
        # (which fold's rows: the entry whose Gram is nearest the fold's own)
        k = int(np.argmin([np.max(np.abs(G - X.T @ (m[:, None] * X) / m.sum())) for m in masks]))
        entries.append((G, c, sc["yy"], masks[k], sc["n_eff"]))
    assert sorted(int(e[4]) for e in entries) == sorted(int(m.sum()) for m in masks)

    def refs(index, z):
        G, c, yy, w, ne = entries[index]
        ref_x = lanes_reference(X, y, z, w[None, :], [ne], bound_weights=np.maximum(w, 1.0)[None, :])
        return ref_x, gram_reference(G, c, yy, z)

    return ds, refs


@pytest.mark.parametrize("family", ["normal", "ill"])
@pytest.mark.parametrize("n,p,K", [(513, 40, 3), (4099, 257, 5), (2000, 600, 4)])
@pytest.mark.parametrize("B", [1, 5, 16, 17, 32])
def test_covariance_route_lane_by_lane(eng, n, p, K, B, family):
    X, y = _data(n, p, n + p + K, family)
    ds, refs = _cov_dataset(eng, X, y, K, seed=n + K)
    with ds:
        for order in ("forward", "reversed"):  # (neighbouring lanes on different Grams, both ways round)
            idx = np.arange(B) % K
            if order == "reversed":
                idx = (K - 1) - idx
            check_lanes(ds, X, y, 2, B, cov_expected(B), seed=B + K + len(order), family=family, cov_index=idx.astype(np.int32),
                        refs=refs)


# ---- what no route serves: an error, never another route -------------------------------------------------------------------
def test_calls_no_kernel_serves_raise(eng, monkeypatch):
    monkeypatch.delenv("SLM_GRAD_RING", raising=False)
    rng = np.random.default_rng(4)
    X, y = _data(300, 600, 1)
    Z = rng.standard_normal((7, 600))
    with eng.dataset(X, y) as ds:
        with pytest.raises(NotImplementedError, match="7-lane"):  # route 0: six lanes at most
            ds.gradient_lanes(Z, route=0)
        with pytest.raises(NotImplementedError, match="no covariance entries"):
            ds.gradient_lanes(Z[:2], route=2, cov_index=[0, 0])
        ds.covariance_folds([np.r_[np.ones(150), np.zeros(150)]], [150])
        with pytest.raises(NotImplementedError, match="no row_weights or n_rows"):
            ds.gradient_lanes(Z[:2], np.ones((2, 300)), route=2, cov_index=[0, 0])
        with pytest.raises(NotImplementedError, match="no row_weights or n_rows"):
            ds.gradient_lanes(Z[:2], route=2, cov_index=[0, 0], n_rows=10)
        with pytest.raises(ValueError):  # (an entry the dataset does not have)
            ds.gradient_lanes(Z[:2], route=2, cov_index=[0, 1])
        with pytest.raises(ValueError):
            ds.gradient_lanes(np.zeros((33, 600)), route=1)
        with pytest.raises(ValueError):
            ds.gradient_lanes(Z[:2], -np.ones((2, 300)), route=0)
        with pytest.raises(ValueError):
            ds.gradient_lanes(Z[:2], n_eff=[1.0, 0.0], route=1)
    X, y = _data(5, 512, 2)
    with eng.dataset(X, y) as ds:  # five and six lanes exist only as LDS-ring kernels, which start above 512 columns
        for B in (5, 6):
            with pytest.raises(NotImplementedError):
                ds.gradient_lanes(np.ones((B, 512)), route=0)
    X, y = _data(5, 10241, 3)
    with eng.dataset(X, y) as ds:  # beyond 10 240 columns route 0 is the one-lane two-pass pair
        with pytest.raises(NotImplementedError):
            ds.gradient_lanes(np.ones((2, 10241)), route=0)


# ---- every kernel of the tables runs and is named ----------------------------------------------------------------------------
def _planned():
    """The kernels the cases of this file expect to name (from the mirror of the tables)."""
    names = set()
    for p, B, ring in ROUTE0:
        names.update((fused_expected(p, B, ring) or "").split(";"))
    for n, p, B, ring in ROUTE1:
        names.update(split_expected(p, B, ring).split(";"))
    names.update(cov_expected(B) for B in (1, 32))
    return names - {""}


def test_the_cases_reach_every_kernel_of_the_tables():
    assert _planned() == ALL_KERNELS, sorted(ALL_KERNELS ^ _planned())


def _one_per_kernel():
    """For every kernel of the tables one small call that should launch it: (route, p, B, env)."""
    cases = []
    for W, C, B, D in GRAD_RING:
        cases.append((0, max(513, 128 * W * C), B, "1"))
    for W, C, R, B in GRAD_DEFAULT:
        cases.append((0, 128 * W * C, B, "0"))
    cases.append((0, 10241, 1, None))
    for C, D in SPLIT_RING:
        cases.append((1, 1024 * C, 5, None))
    for B in (16, 18, 20, 32):
        cases.append((1, 600, B, None))
    for B in (16, 32):
        cases.append((2, 40, B, None))
    return cases


def test_every_kernel_of_the_tables_is_launched_and_named(eng, monkeypatch):
    seen = set()
    for route, p, B, env in _one_per_kernel():
        _set_env(monkeypatch, "SLM_GRAD_RING", env if route == 0 else None)
        _set_env(monkeypatch, "SLM_ROWDOT_RING", None)
        n = 60 if route == 2 else 7  # (three folds of sixty rows: none empty)
        X, y = _data(n, p, p + B)
        if route == 2:
            ds, refs = _cov_dataset(eng, X, y, 3, seed=p)
            with ds:
                names = check_lanes(ds, X, y, 2, B, cov_expected(B), seed=B, cov_index=(np.arange(B) % 3).astype(np.int32),
                                    refs=refs)
        else:
            with eng.dataset(X, y) as ds:
                expect = fused_expected(p, B, env) if route == 0 else split_expected(p, B)
                names = check_lanes(ds, X, y, route, B, expect, seed=p + B)
        seen.update(names.split(";"))
    assert seen == ALL_KERNELS, sorted(ALL_KERNELS ^ seen)


# ---- the headline shape -----------------------------------------------------------------------------------------------------
def test_headline_shape_lane_by_lane(eng, monkeypatch):
    # 100 000 x 5 000 (a row block of ~390 rows per CU, the XCD tile remap): 18 lanes (rowdot18 + xtr18: lanes 16 and 17 on the
    # vector units) and 32 (both planes); float64 reference on a seeded sample of 512 columns, the residuals in full
    monkeypatch.delenv("SLM_ROWDOT_RING", raising=False)
    n, p = 100_000, 5_000
    rng = np.random.default_rng(12)
    coef = np.zeros(p)
    coef[rng.choice(p, 40, replace=False)] = 10.0 * rng.standard_normal(40)
    cols = np.sort(np.random.default_rng(13).choice(p, 512, replace=False))
    with eng.synthetic_dataset(n, p, seed=5, coef=coef, noise_sd=5.0) as ds:
        X, y = ds.download()
        for B in (18, 32):
            Z, W, ne = lane_inputs(np.random.default_rng(B), n, p, B)
            G, loss, names = ds.gradient_lanes(Z, W, ne, route=1)
            assert names == split_expected(p, B)
            ref = lanes_reference(X, y, Z, W, ne, cols=cols)
            assert not ref.exact
            assert_within_bound(G[:, cols], loss, ref, f"{B} lanes at {n} x {p}")
            G2, loss2, _ = ds.gradient_lanes(Z, W, ne, route=1)
            assert np.array_equal(G, G2) and np.array_equal(loss, loss2)
