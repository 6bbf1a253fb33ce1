"""The kernels that build the working set W and the residual kernels that read it, against a reference (slm_working_set_lanes).

W is built in stages (a fresh selection, then appends) exactly as a solve queues it after a selection; then one gradient pass
of up to 32 lanes runs on it, each lane with its own point, row weights, n_eff and on-W flag.  Every case asserts:
  1. the kernels the engine reports are the ones the mirror in tests/_gradient_reference.py expects;
  2. the componentwise bounds of tests/_gradient_reference.py: the Gram entries of the row sets (padding exactly 0), X_W^T y,
     every lane's gradient and loss -- and bit for bit what has to be exact: the gathered columns, the old block of a Gram
     across an append, the mirrored entries, the covariance route's sub-matrix;
  3. determinism: the same call twice gives the same bits.
"""

import hashlib

import numpy as np
import pytest

from _gradient_reference import (
    assert_gram_within_bound,
    assert_within_bound,
    assert_xty_within_bound,
    gram_reference,
    lane_inputs,
    lanes_reference,
    ws_build_expected,
    ws_gram_mapping,
    ws_gram_reference,
    ws_K,
    ws_pass_expected,
    ws_xty_reference,
)
from sparselm_amd import _engine

pytestmark = pytest.mark.gpu

ALL_KERNELS = {"ws_block_owner_kernel", "ws_gather_kernel", "ws_xty_partial_kernel", "ws_xty_apply_kernel", "ws_gram_kernel",
               "ws_gram_reduce_kernel", "ws_gram_cov_kernel", "resid_ws_kernel<16>", "resid_mfma_kernel", "resid32_mfma_kernel",
               "rowdot_ring_kernel<8,1,5,3>", "rowdot_mfma_kernel", "rowdot18_mfma_kernel", "rowdot32_mfma_kernel",
               "xtr_mfma_kernel", "xtr18_mfma_kernel", "xtr32_mfma_kernel", "cov_gz_mfma_kernel", "cov_gz32_mfma_kernel"}


@pytest.fixture(scope="module")
def eng():
    return _engine.get_engine(0)


def _set_env(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


def _data(n, p, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, p)), rng.standard_normal(n)


def _stages(p, k_end, seed):
    return np.random.default_rng(seed).choice(p, int(k_end[-1]), replace=False).astype(np.int32)


def _on_w(Z, cols, on_ws):
    """Points of the lanes with on_ws: zero outside W (the model solver's points)."""
    Z = Z.copy()
    out = np.ones(Z.shape[1], dtype=bool)
    out[cols] = False
    Z[np.asarray(on_ws, dtype=bool)[:, None] & out[None, :]] = 0.0
    return Z


def _expected_sets(W, ne):
    first = {}
    return np.array([first.setdefault((b"" if W is None else W[l].tobytes(), ne[l].tobytes()), len(first))
                     for l in range(len(ne))], dtype=np.int32)


_GRAM_REFS = {}


def _gram_ref(X, cols, w, ne):
    """ws_gram_reference, kept for the cases that ask again (the long double product is the slow part of this file)."""
    h = hashlib.sha1()
    for a in (X[:, cols], np.zeros(0) if w is None else w, np.array([0.0 if ne is None else ne])):
        h.update(np.ascontiguousarray(a).tobytes())
    key = h.hexdigest()
    if key not in _GRAM_REFS:
        if len(_GRAM_REFS) > 64:
            _GRAM_REFS.clear()
        _GRAM_REFS[key] = ws_gram_reference(X, cols, w, ne)
    return _GRAM_REFS[key]


def _call(ds, Z, cols, k_end, on_ws, W=None, ne=None, **kw):
    r = ds.working_set_lanes(Z, cols, k_end, on_ws=on_ws, row_weights=W, n_eff=ne, **kw)
    r2 = ds.working_set_lanes(Z, cols, k_end, on_ws=on_ws, row_weights=W, n_eff=ne, **kw)
    assert r.kernels == r2.kernels
    assert np.array_equal(r.G, r2.G) and np.array_equal(r.loss, r2.loss) and np.array_equal(r.gram, r2.gram), "not deterministic"
    if r.XW is not None:
        assert np.array_equal(r.XW, r2.XW), "gather not deterministic"
    if r.xty is not None:
        assert np.array_equal(r.xty, r2.xty) and r.yy == r2.yy, "xty not deterministic"
    return r


def check_ws(ds, X, y, Z, cols, k_end, on_ws, W=None, ne=None, resid_vec=False, ring=None, owner=None, xty=False,
             gather_from_x=False, gram_sets=None):
    """One call of route 1 with assertions 1-3 (the Grams of the first `gram_sets` row sets; None: all).  Returns it."""
    n, p = X.shape
    B = Z.shape[0]
    kreal = int(k_end[-1])
    r = _call(ds, Z, cols, k_end, on_ws, W, ne, xty=xty, gather_from_x=gather_from_x, want_xw=True)
    expect = ws_build_expected(k_end, 1, xty, owner if owner is not None else W is not None) + \
        ws_pass_expected(p, B, resid_vec, ring)
    assert r.kernels == ";".join(expect), (r.kernels, expect)
    K = ws_K(kreal)
    assert r.K == K
    # the gathered columns, bit for bit, with zero padding
    XW = np.zeros((n, K))
    XW[:, :kreal] = X[:, cols[:kreal]]
    assert np.array_equal(r.XW, XW), "gathered columns differ from X[:, cols]"
    # the Gram of every row set
    sets = _expected_sets(W, np.full(B, float(n)) if ne is None else np.asarray(ne, dtype=np.float64))
    assert np.array_equal(r.set_of, sets) and r.n_sets == sets.max() + 1
    for st in range(r.n_sets if gram_sets is None else min(gram_sets, r.n_sets)):
        l = int(np.flatnonzero(sets == st)[0])
        ref = _gram_ref(X, cols[:kreal], None if W is None else W[l], None if ne is None else ne[l])
        assert_gram_within_bound(r.gram[st], ref, f"set {st} of {r.n_sets}, k_end {list(k_end)}")
    if xty:
        assert_xty_within_bound(r.xty, r.yy, ws_xty_reference(X, y, cols[:kreal]), f"n={n}")
    ref = lanes_reference(X, y, Z, W, ne)
    assert_within_bound(r.G, r.loss, ref, f"route 1 on W {r.kernels} n={n} p={p} B={B}")
    return r


# ---- gather + Gram: the stages of every ws_gram_kernel mapping -----------------------------------------------------------
STAGES = [
    [1], [17], [111], [128],          # fresh, up to 8 tiles (row-split)
    [144], [256], [500], [512],       # fresh, more than 8 tiles (generic)
    [40, 45], [111, 128], [100, 260], [112, 144, 176], [17, 33, 34, 111],  # appends of up to 16 new tile rows (row-split)
    [17, 300], [16, 512], [1, 500],   # appends of more than 16 new tile rows (generic)
]


@pytest.mark.parametrize("k_end", STAGES, ids=lambda k: "-".join(map(str, k)))
@pytest.mark.parametrize("n", [40, 1000])
def test_staged_gram_and_gather(eng, monkeypatch, record_property, k_end, n):
    _set_env(monkeypatch, "SLM_RESID_VEC", None)
    _set_env(monkeypatch, "SLM_ROWDOT_RING", None)
    p = 600
    X, y = _data(n, p, n + k_end[-1])
    cols = _stages(p, k_end, len(k_end) * 7 + k_end[0])
    rng = np.random.default_rng(k_end[-1])
    W = np.tile(rng.uniform(0.0, 2.0, n), (2, 1))  # (fractional weights: two lanes of one set)
    ne = np.array([0.9 * n, 0.9 * n])
    Z = _on_w(rng.standard_normal((2, p)), cols, [1, 1])
    record_property("gram_mappings", sorted({ws_gram_mapping(k0, ws_K(k1)) for k0, k1 in zip([0] + list(k_end[:-1]), k_end)}))
    with eng.dataset(X, y) as ds:
        for gx in (False, True):  # (from the column-major copy, and from X)
            r = check_ws(ds, X, y, Z, cols, k_end, [1, 1], W, ne, gather_from_x=gx)
        G = r.gram[0]
        K = r.K
        kreal = k_end[-1]
        assert np.all(G[kreal:] == 0) and np.all(G[:, kreal:] == 0)
        row_lo = 0
        if len(k_end) > 1:
            # the stage before: its Gram keeps its bits in the old block, the mirror copies the new rows bit for bit
            prev = _call(ds, Z, cols, k_end[:-1], [0, 0], W, ne)  # (Z lies on the final W, not on this one)
            row_lo = (k_end[-2] // 16) * 16
            assert np.array_equal(G[:row_lo, :row_lo], prev.gram[0][:row_lo, :row_lo]), "the old block changed across an append"
            assert np.array_equal(G[:row_lo, row_lo:], G[row_lo:, :row_lo].T), "mirrored entries differ from their counterparts"
            # a one-shot build of the same columns agrees within the bound (not bit for bit: other tiles, another mapping)
            one = _call(ds, Z, cols, [kreal], [1, 1], W, ne)
            assert_gram_within_bound(one.gram[0], _gram_ref(X, cols, W[0], ne[0]), "one-shot")
        # the new x new block: symmetric within the bound (each entry is checked above); bitwise symmetry is recorded only --
        # the two tiles of a pair round (x_ri w_r) x_rj differently
        new = G[row_lo:K, row_lo:K]
        record_property("new_block_bitwise_symmetric", bool(np.array_equal(new, new.T)))


# ---- row sets: fold masks that make row blocks all ones, all zeros or mixed; the owner table on and off -------------------
def _fold_lanes(n, n_sets, lanes_per_set, seed):
    """Contiguous folds (KFold's masks) for the first sets, uniform(0, 2) weights for the last; n_eff = sum of the weights."""
    rng = np.random.default_rng(seed)
    bounds = np.linspace(0, n, max(n_sets, 2) + 1).astype(int)
    rows = []
    for st in range(n_sets):
        if st == n_sets - 1 and n_sets > 1:
            w = rng.uniform(0.0, 2.0, n)
        else:
            w = np.ones(n)
            w[bounds[st]:bounds[st + 1]] = 0.0
        rows.append(w)
    W = np.repeat(np.array(rows), lanes_per_set, axis=0)
    ne = np.repeat(np.array([max(w.sum(), 1.0) for w in rows]), lanes_per_set)
    return W, ne


@pytest.mark.parametrize("n_sets,lanes_per_set,n,kreal", [(1, 3, 33000, 45), (2, 2, 33000, 45), (5, 2, 33000, 45),
                                                          (32, 1, 8192, 13)])
def test_row_sets_and_the_owner_table(eng, monkeypatch, n_sets, lanes_per_set, n, kreal):
    _set_env(monkeypatch, "SLM_RESID_VEC", None)
    _set_env(monkeypatch, "SLM_ROWDOT_RING", None)
    p = 200
    X, y = _data(n, p, n_sets + n)
    k_end = [kreal // 2, kreal]
    cols = _stages(p, k_end, n_sets)
    W, ne = _fold_lanes(n, n_sets, lanes_per_set, n_sets)
    B = W.shape[0]
    on = (np.arange(B) % 2 == 0).astype(np.int32)
    Z = _on_w(np.random.default_rng(B).standard_normal((B, p)), cols, on)
    with eng.dataset(X, y) as ds:
        monkeypatch.delenv("SLM_NO_GRAM_OWNER", raising=False)
        shared = check_ws(ds, X, y, Z, cols, k_end, on, W, ne)
        monkeypatch.setenv("SLM_NO_GRAM_OWNER", "1")
        alone = check_ws(ds, X, y, Z, cols, k_end, on, W, ne, owner=False)
    # (engine_path.hip, ws_row_blocks: whether or not the owner table shares the blocks, the same sums bit for bit)
    assert np.array_equal(shared.gram, alone.gram), "SLM_NO_GRAM_OWNER=1 changed the Grams' bits"
    assert np.array_equal(shared.G, alone.G) and np.array_equal(shared.loss, alone.loss)


# ---- X_W^T y at a sample start --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 64, 32768, 33000, 100000])
@pytest.mark.parametrize("p", [8, 300])
def test_xty_partials(eng, monkeypatch, n, p):
    # (p = 8 is the regression case of the xty kernels' partial sums: 512 row blocks x 513 doubles from 32 768 rows on, more
    #  than the gradient's partial buffer holds at rows of up to 32 columns -- they now go to the Gram's partial block)
    _set_env(monkeypatch, "SLM_RESID_VEC", None)
    _set_env(monkeypatch, "SLM_ROWDOT_RING", None)
    X, y = _data(n, p, n + p)
    k_end = [5, 7] if p < 16 else [60, 100]
    cols = _stages(p, k_end, n)
    Z = _on_w(np.random.default_rng(n).standard_normal((1, p)), cols, [1])
    with eng.dataset(X, y) as ds:
        check_ws(ds, X, y, Z, cols, k_end, [1], xty=True)


# ---- route 1 on W: the residual kernels lane by lane ------------------------------------------------------------------------
LANES = (1, 5, 6, 15, 16, 17, 18, 20, 21, 31, 32)
MASKS = ("all", "none", "alternating", "half1", "last")


def _mask(kind, B):
    l = np.arange(B)
    return {"all": l >= 0, "none": l < 0, "alternating": l % 2 == 0, "half1": l >= 16, "last": l == B - 1}[kind].astype(np.int32)


def _case_inputs(n, p, B, cols, on, seed):
    Z, W, ne = lane_inputs(np.random.default_rng(seed), n, p, B)  # (dense, sparse, zero, x 1e6, x 1e-6 points)
    return _on_w(Z, cols, on), W, ne


def _residual_case(ds, X, y, B, kind, cols, k_end, resid_vec, ring, seed):
    n, p = X.shape
    on = _mask(kind, B)
    Z, W, ne = _case_inputs(n, p, B, cols, on, seed)
    r = check_ws(ds, X, y, Z, cols, k_end, on, W, ne, resid_vec=resid_vec == "1", ring=ring, gram_sets=2)
    if B > 1:  # lane independence: the other lanes' points, weights, n_eff AND on-W flags replaced
        Zf, Wf, nef = lane_inputs(np.random.default_rng(seed + 7919), n, p, B, offset=2)
        for keep in (np.arange(B) % 2 == 0, np.arange(B) % 2 == 1):
            ok = np.where(keep, on, 1 - on).astype(np.int32)
            Zk = _on_w(np.where(keep[:, None], Z, Zf), cols, ok)
            r3 = _call(ds, Zk, cols, k_end, ok, np.where(keep[:, None], W, Wf), np.where(keep, ne, nef))
            assert np.array_equal(r3.G[keep], r.G[keep]) and np.array_equal(r3.loss[keep], r.loss[keep]), \
                f"lanes {np.flatnonzero(keep).tolist()} changed with the other lanes' inputs"
    return r


@pytest.mark.parametrize("B", LANES)
@pytest.mark.parametrize("n", [40, 1000, 4099])
def test_residual_route_lane_by_lane(eng, monkeypatch, B, n):
    p = 200
    X, y = _data(n, p, n * 3 + B)
    k_end = [37, 61]
    cols = _stages(p, k_end, B + n)
    with eng.dataset(X, y) as ds:
        for i, kind in enumerate(MASKS):
            if kind == "half1" and B <= 16:
                continue
            for resid_vec, ring in (("0", None), ("1", "1"), ("0", "0"), ("1", None)):
                if B > 16 and (resid_vec, ring) != ("0", None) and i % 2:
                    continue  # (more than sixteen lanes: neither switch changes a kernel; every second mask is enough)
                _set_env(monkeypatch, "SLM_RESID_VEC", resid_vec)
                _set_env(monkeypatch, "SLM_ROWDOT_RING", ring)
                _residual_case(ds, X, y, B, kind, cols, k_end, resid_vec, ring, seed=B * 31 + n)


@pytest.mark.parametrize("B,kind", [(1, "none"), (3, "alternating"), (5, "all"), (6, "alternating"), (18, "last")])
def test_an_all_zero_lane_off_w(eng, monkeypatch, B, kind):
    # lanes at zero that take their residual from X: rowdot_ring_kernel's (and rowdot_mfma_kernel's) shortcut e = -y, which
    # only a call with control blocks reaches (PathCtl::zzero)
    _set_env(monkeypatch, "SLM_RESID_VEC", None)
    _set_env(monkeypatch, "SLM_ROWDOT_RING", None)
    n, p = 1000, 200
    X, y = _data(n, p, B)
    k_end = [30]
    cols = _stages(p, k_end, B)
    on = _mask(kind, B)
    Z, W, ne = _case_inputs(n, p, B, cols, on, B)
    Z[~on.astype(bool)] = 0.0
    with eng.dataset(X, y) as ds:
        check_ws(ds, X, y, Z, cols, k_end, on, W, ne, gram_sets=1)


def test_residual_route_agrees_with_residuals_from_x(eng, monkeypatch):
    _set_env(monkeypatch, "SLM_RESID_VEC", None)
    _set_env(monkeypatch, "SLM_ROWDOT_RING", None)
    n, p = 4099, 300
    X, y = _data(n, p, 77)
    k_end = [50, 90]
    cols = _stages(p, k_end, 3)
    with eng.dataset(X, y) as ds:
        for B in (5, 16, 18, 32):
            on = _mask("all", B)
            Z, W, ne = _case_inputs(n, p, B, cols, on, B)
            r = check_ws(ds, X, y, Z, cols, k_end, on, W, ne, gram_sets=1)
            Gx, lx, _ = ds.gradient_lanes(Z, W, ne, route=1)
            ref = lanes_reference(X, y, Z, W, ne)
            assert_within_bound(Gx, lx, ref, "residuals from X")
            assert_within_bound(r.G, r.loss, ref, "residuals from W")


def test_calls_the_diagnostic_refuses(eng):
    n, p = 100, 50
    X, y = _data(n, p, 1)
    cols = np.arange(10, dtype=np.int32)
    Z = np.zeros((2, p))
    Z[1, 20] = 1.0
    with eng.dataset(X, y) as ds:
        with pytest.raises(ValueError, match="outside"):
            ds.working_set_lanes(Z, cols, [10], on_ws=[0, 1])
        ds.working_set_lanes(Z, cols, [10], on_ws=[1, 0])  # (lane 1 off W: fine)
        with pytest.raises(ValueError):
            ds.working_set_lanes(Z, np.array([1, 1], dtype=np.int32), [2])  # (a repeated column)
        with pytest.raises(ValueError):
            ds.working_set_lanes(Z, cols, [5, 5])  # (an append of nothing)
        with pytest.raises(NotImplementedError, match="no covariance entries"):
            ds.working_set_lanes(Z, cols, [10], route=2, cov_index=[0, 0])


# ---- the covariance route on W ----------------------------------------------------------------------------------------------
def _cov_dataset(eng, X, y, F):
    n = X.shape[0]
    bounds = np.linspace(0, n, F + 1).astype(int)
    masks = []
    for k in range(F):
        m = np.ones(n)
        m[bounds[k]:bounds[k + 1]] = 0.0
        masks.append(m)
    ds = eng.dataset(X, y)
    ds.covariance_folds(masks, [int(m.sum()) for m in masks])
    return ds, [ds.covariance_download(e) for e in range(ds.covariance_count())]


def check_cov(ds, entries, Z, cols, k_end, on, ci):
    B = Z.shape[0]
    kreal = int(k_end[-1])
    K = ws_K(kreal)
    r = _call(ds, Z, cols, k_end, on, route=2, cov_index=ci)
    product = "cov_gz_mfma_kernel" if B <= 16 else "cov_gz32_mfma_kernel"
    expect = ws_build_expected(k_end, 2) + [product + ("+listed" if np.all(on) else "")]
    assert r.kernels == ";".join(expect), (r.kernels, expect)
    for st in range(r.n_sets):
        Gc = entries[int(ci[int(np.flatnonzero(r.set_of == st)[0])])][0]
        sub = np.zeros((K, K))
        sub[:kreal, :kreal] = Gc[np.ix_(cols[:kreal], cols[:kreal])]
        assert np.array_equal(r.gram[st], sub), "ws_gram_cov_kernel's G differs from G_cov[idx][:, idx]"
    for l in range(B):
        Gc, c, sc = entries[int(ci[l])]
        assert_within_bound(r.G[l:l + 1], r.loss[l:l + 1], gram_reference(Gc, c, sc["yy"], Z[l:l + 1]), f"lane {l}")
    return r


@pytest.mark.parametrize("B", [1, 5, 16, 17, 32])
def test_covariance_route_on_w(eng, B):
    n, p, F = 2000, 300, 3
    X, y = _data(n, p, B + 1)
    k_end = [40, 77]
    cols = _stages(p, k_end, B)
    ds, entries = _cov_dataset(eng, X, y, F)
    with ds:
        ci = (np.arange(B) % F).astype(np.int32)
        for kind in ("all", "last_off"):  # (one lane off W: the product reads every row of its Gram)
            on = np.ones(B, dtype=np.int32)
            if kind == "last_off":
                on[-1] = 0
            Z = _on_w(np.random.default_rng(B + len(kind)).standard_normal((B, p)), cols, on)
            check_cov(ds, entries, Z, cols, k_end, on, ci)


# ---- every kernel named above runs and is named --------------------------------------------------------------------------
def test_every_kernel_is_launched_and_named(eng, monkeypatch):
    _set_env(monkeypatch, "SLM_ROWDOT_RING", None)
    monkeypatch.delenv("SLM_NO_GRAM_OWNER", raising=False)
    n, p = 300, 200
    X, y = _data(n, p, 5)
    k_end = [20, 40]
    cols = _stages(p, k_end, 5)
    seen = set()
    with eng.dataset(X, y) as ds:
        for B, kind, resid_vec, xty in ((1, "none", "0", True), (6, "all", "0", False), (6, "all", "1", False),
                                        (18, "last", "0", False), (32, "alternating", "0", False)):
            _set_env(monkeypatch, "SLM_RESID_VEC", resid_vec)
            on = _mask(kind, B)
            Z, W, ne = _case_inputs(n, p, B, cols, on, B)
            r = check_ws(ds, X, y, Z, cols, k_end, on, W, ne, resid_vec=resid_vec == "1", gram_sets=1)
            seen.update(r.kernels.split(";"))
            if xty:  # (X_W^T y needs no row weights)
                r = check_ws(ds, X, y, Z, cols, k_end, on, xty=True)
                seen.update(r.kernels.split(";"))
    ds, entries = _cov_dataset(eng, X, y, 3)
    with ds:
        for B in (1, 17):
            on = np.ones(B, dtype=np.int32)
            Z = _on_w(np.random.default_rng(B).standard_normal((B, p)), cols, on)
            r = check_cov(ds, entries, Z, cols, k_end, on, (np.arange(B) % 3).astype(np.int32))
            seen.update(k.split("+")[0] for k in r.kernels.split(";"))
    assert seen == ALL_KERNELS, sorted(ALL_KERNELS ^ seen)


# ---- the full size ----------------------------------------------------------------------------------------------------------
def test_full_size_working_set(eng, monkeypatch):
    # 100 000 x 5 000: 18 lanes (resid32 + xtr18 on W, rowdot18 for the lanes off W), K = 272 (an append to 268) and 512
    _set_env(monkeypatch, "SLM_RESID_VEC", None)
    _set_env(monkeypatch, "SLM_ROWDOT_RING", None)
    monkeypatch.delenv("SLM_NO_GRAM_OWNER", raising=False)
    n, p, B = 100_000, 5_000, 18
    rng = np.random.default_rng(21)
    coef = np.zeros(p)
    coef[rng.choice(p, 40, replace=False)] = 10.0 * rng.standard_normal(40)
    sample = np.sort(np.random.default_rng(22).choice(p, 256, replace=False))
    with eng.synthetic_dataset(n, p, seed=6, coef=coef, noise_sd=5.0) as ds:
        X, y = ds.download()
        for k_end in ([200, 268], [512]):
            cols = _stages(p, k_end, k_end[0])
            on = (np.arange(B) % 3 != 2).astype(np.int32)
            Z, W, ne = _case_inputs(n, p, B, cols, on, k_end[0])
            r = _call(ds, Z, cols, k_end, on, W, ne)
            expect = ws_build_expected(k_end, 1, owner=True) + ws_pass_expected(p, B)
            assert expect[-3:] == ["rowdot18_mfma_kernel", "resid32_mfma_kernel", "xtr18_mfma_kernel"]
            assert r.kernels == ";".join(expect), r.kernels
            sets = _expected_sets(W, ne)
            assert np.array_equal(r.set_of, sets)
            for st in (0, r.n_sets - 1):
                l = int(np.flatnonzero(sets == st)[0])
                ref = ws_gram_reference(X, cols, W[l], ne[l])
                assert not ref.exact
                assert_gram_within_bound(r.gram[st], ref, f"set {st} at {n} x {p}, K {r.K}")
            ref = lanes_reference(X, y, Z, W, ne, cols=sample)
            assert_within_bound(r.G[:, sample], r.loss, ref, f"{B} lanes at {n} x {p}, K {r.K}")
