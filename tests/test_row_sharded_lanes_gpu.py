"""The row-sharded state machine below a solve, against the whole-X references: slm_gradient_lanes and slm_working_set_lanes
on row-sharded datasets, the ranks being threads of this process joined by the in-process communicator (tests/_ranks.py).

What runs is a sharded solve's own: the all-reduce behind the fused and the split pass (local_sum_kernel's rank-order sum),
the staging matrix of the Gram parts and its zeroing, ws_gram_reduce_kernel's staged branch, the all-reduce of the staging
matrix with the stop words behind it, ws_publish_kernel and the 1 / n_global scaling of ws_bind.  Every rank's output is held
to the references of tests/_gradient_reference.py on the WHOLE X -- their bounds hold for partial sums in any tree, and a
fixed-order sum over at most eight ranks is one (tests/test_row_sharded_lanes_cpu.py checks that premise and that the faults
of an exchange fall outside) -- and to what must be exact: the ranks' bits are the same, a call twice gives the same bits,
the gathered columns are this rank's rows of X, an append keeps the old block and mirrors the new entries, and every call
enters the same pinned number of collectives on every rank.

The row splits (tests/_ranks.py) are explicit row counts: ranks differ in their number of row blocks, one rank holds less
than a block (1, 3 or 7 rows), eight ranks are the communicator's most.  All assertions run after the ranks have joined: a
failing rank never leaves its peers waiting, and no test depends on the communicator's timeout (30 s: a mismatch ends as an
error).  Sharded solves stay at sixteen lanes, so more than sixteen lanes are out of scope here."""

import numpy as np
import pytest

from _gradient_reference import (
    assert_gram_within_bound,
    assert_within_bound,
    lane_inputs,
    lanes_reference,
    ws_build_expected,
    ws_gram_reference,
    ws_K,
    ws_pass_expected,
)
from _ranks import SPLITS, run_ranks, split_bounds
from sparselm_amd import _engine
from test_gradient_lanes_gpu import fused_expected, split_expected

pytestmark = pytest.mark.gpu

TIMEOUT_S = 30.0
KNOBS = ("SLM_RESID_VEC", "SLM_ROWDOT_RING", "SLM_GRAD_RING", "SLM_NO_GRAM_OWNER")


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    """The environment knobs are read at every call: set (here: cleared) before the rank threads start."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)


def _sid(split):
    return f"{len(split)}x{split[0]}" if len(split) > 3 else "_".join(map(str, split))


_CACHE = {}


def _cached(key, make):
    """References are computed once and shared by the cases that meet them on different splits."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _data(n, p):
    def make():
        rng = np.random.default_rng(1000 * n + p)
        return rng.standard_normal((n, p)), rng.standard_normal(n)
    return _cached(("data", n, p), make)


def _same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- (a) gradients ------------------------------------------------------------------------------------------------------------
GRAD_SHAPES = [((40, 30), s) for s in SPLITS[40]] + [((1000, 129), s) for s in SPLITS[1000]] + \
              [((4099, 48), s) for s in SPLITS[4099]] + [((333, 1537), s) for s in SPLITS[333]]


def _grad_calls(p):
    """(route, lanes): route 0 with every lane count the fused tables serve at this width, route 1 with 1, 5 and 16."""
    return [(0, B) for B in range(1, 7) if fused_expected(p, B) is not None] + [(1, B) for B in (1, 5, 16)]


def _grad_inputs(n, p, route, B):
    def make():
        X, y = _data(n, p)
        Z, W, ne = lane_inputs(np.random.default_rng(7 * n + p + 100 * route + B), n, p, B)
        return Z, W, ne, lanes_reference(X, y, Z, W, ne)
    return _cached(("grad", n, p, route, B), make)


@pytest.mark.parametrize("shape,split", GRAD_SHAPES, ids=[f"{n}x{p}-{_sid(s)}" for (n, p), s in GRAD_SHAPES])
def test_sharded_gradients_lane_by_lane(shape, split):
    """Every lane with its own point, its slice of its own row weights and the job's n_eff (lane_inputs: among them weights
    that are zero on whole ranks): each rank's gradients and losses inside the whole-X bound, the same bits on every rank and
    on a second call, one collective per call."""
    n, p = shape
    assert sum(split) == n
    X, y = _data(n, p)
    calls = _grad_calls(p)
    inputs = [_grad_inputs(n, p, route, B) for route, B in calls]
    bounds = split_bounds(split)

    def work(r, eng):
        lo, hi = bounds[r]
        out = []
        with eng.dataset(X[lo:hi], y[lo:hi]) as ds:
            ds.set_global_rows(n)
            for (route, B), (Z, W, ne, _) in zip(calls, inputs):
                c0 = eng.comm_collectives()
                first = ds.gradient_lanes(Z, W[:, lo:hi], ne, route=route)
                c1 = eng.comm_collectives()
                again = ds.gradient_lanes(Z, W[:, lo:hi], ne, route=route)
                out.append((first, again, c1 - c0, eng.comm_collectives() - c1))
        return out

    out, counts, infos = run_ranks(len(split), work, timeout_s=TIMEOUT_S)
    assert infos == [(r, len(split)) for r in range(len(split))] and len(set(counts)) == 1
    for k, ((route, B), (Z, W, ne, ref)) in enumerate(zip(calls, inputs)):
        expect = fused_expected(p, B) if route == 0 else split_expected(p, B)
        for r in range(len(split)):
            (G, loss, names), again, d0, d1 = out[r][k]
            what = f"route {route}, {B} lanes, rank {r} of {split}"
            assert names == expect, (what, names, expect)
            assert_within_bound(G, loss, ref, what)
            assert _same_bits((G, loss), out[0][k][0][:2]), f"{what}: not rank 0's bits"
            assert _same_bits((G, loss), again[:2]), f"{what}: not deterministic"
            assert (d0, d1) == (1, 1), f"{what}: {d0} and {d1} collectives for one call"


@pytest.mark.parametrize("split", [SPLITS[1000][2], SPLITS[1000][4]], ids=_sid)
def test_dataset_row_weights_and_no_n_eff(split):
    """Row weights of the dataset (each rank its slice), no per-lane weights, n_eff NULL: the scale is n_global on every rank,
    never the rank's own row count."""
    n, p = 1000, 129
    X, y = _data(n, p)
    w = np.random.default_rng(5).uniform(0.0, 2.0, n)
    Z = np.random.default_rng(6).standard_normal((3, p))
    ref = _cached(("grad-rw", n, p), lambda: lanes_reference(X, y, Z, np.tile(w, (3, 1)), None))
    bounds = split_bounds(split)

    def work(r, eng):
        lo, hi = bounds[r]
        with eng.dataset(X[lo:hi], y[lo:hi], row_weight=w[lo:hi]) as ds:
            ds.set_global_rows(n)
            return [ds.gradient_lanes(Z, None, None, route=route) for route in (0, 1)]

    out, counts, _ = run_ranks(len(split), work, timeout_s=TIMEOUT_S)
    assert len(set(counts)) == 1
    for r in range(len(split)):
        for k in range(2):
            G, loss, _ = out[r][k]
            assert_within_bound(G, loss, ref, f"route {k}, rank {r} of {split}")
            assert _same_bits((G, loss), out[0][k][:2])


# ---- (b) the staged Gram ------------------------------------------------------------------------------------------------------
# One of each ws_gram_kernel mapping and the appends across tile boundaries (STAGES of tests/test_working_set_lanes_gpu.py).
# Every stage meets an uneven split, every split an append, the eight ranks one append.
_A, _B, _C, _D, _E = SPLITS[1000]
_F, _G, _H = SPLITS[40]
STAGED = [
    (40, [1], _G), (40, [17], _H), (40, [128], _G), (40, [144], _H), (40, [40, 45], _F), (40, [40, 45], _G),
    (40, [17, 33, 34, 111], _H), (40, [100, 260], _G), (40, [16, 512], _H), (40, [16, 512], _F),
    (1000, [1], _C), (1000, [17], _B), (1000, [128], _B), (1000, [144], _C), (1000, [40, 45], _A), (1000, [40, 45], _E),
    (1000, [40, 45], _C), (1000, [17, 33, 34, 111], _B), (1000, [17, 33, 34, 111], _D), (1000, [100, 260], _C),
    (1000, [100, 260], _E), (1000, [16, 512], _B), (1000, [16, 512], _D),
]
P_STAGED = 600


def _staged_inputs(n, k_end):
    def make():
        X, y = _data(n, P_STAGED)
        rng = np.random.default_rng(n + 31 * k_end[-1] + len(k_end))
        cols = rng.choice(P_STAGED, k_end[-1], replace=False).astype(np.int32)
        W = np.tile(rng.uniform(0.0, 2.0, n), (2, 1))  # (fractional weights: two lanes of one set)
        ne = np.array([0.9 * n, 0.9 * n])
        Z = np.zeros((2, P_STAGED))
        Z[:, cols] = rng.standard_normal((2, len(cols)))  # (points on W)
        return cols, W, ne, Z, ws_gram_reference(X, cols, W[0], ne[0]), lanes_reference(X, y, Z, W, ne)
    return _cached(("staged", n, tuple(k_end)), make)


def _ws_call(eng, ds, Z, cols, k_end, on_ws, W, ne, **kw):
    """One call with the collectives it entered."""
    c0 = eng.comm_collectives()
    r = ds.working_set_lanes(Z, cols, k_end, on_ws=on_ws, row_weights=W, n_eff=ne, **kw)
    r.collectives = eng.comm_collectives() - c0
    return r


@pytest.mark.parametrize("n,k_end,split", STAGED, ids=[f"{n}-{'-'.join(map(str, k))}-{_sid(s)}" for n, k, s in STAGED])
def test_sharded_staged_gram(n, k_end, split):
    """W built in stages on every rank's rows, from the column-major copy and from X: the all-reduced, published Gram against
    the reference on the whole X with the lane's global weights and n_eff."""
    X, y = _data(n, P_STAGED)
    cols, W, ne, Z, gref, lref = _staged_inputs(n, k_end)
    bounds = split_bounds(split)

    def work(r, eng):
        lo, hi = bounds[r]
        with eng.dataset(X[lo:hi], y[lo:hi]) as ds:
            ds.set_global_rows(n)
            runs = [[_ws_call(eng, ds, Z, cols, k_end, [1, 1], W[:, lo:hi], ne, gather_from_x=gx, want_xw=True) for _ in range(2)]
                    for gx in (False, True)]
            prev = _ws_call(eng, ds, Z, cols, k_end[:-1], [0, 0], W[:, lo:hi], ne) if len(k_end) > 1 else None
        return runs, prev

    out, counts, _ = run_ranks(len(split), work, timeout_s=TIMEOUT_S)
    assert len(set(counts)) == 1
    kreal, K = k_end[-1], ws_K(k_end[-1])
    expect = ws_build_expected(k_end, 1, owner=True, sharded=True) + ws_pass_expected(P_STAGED, 2)
    assert expect.count("ws_publish_kernel") == len(k_end) and "ws_block_owner_kernel" not in expect
    for r, (lo, hi) in enumerate(bounds):
        runs, prev = out[r]
        for gx, (first, again) in zip((False, True), runs):
            what = f"rank {r} of {split}, stages {k_end}, gather_from_x {gx}"
            assert first.kernels == ";".join(expect), (what, first.kernels)
            assert first.collectives == again.collectives == len(k_end) + 2, what
            assert first.n_sets == 1 and first.set_of.tolist() == [0, 0] and first.K == K, what
            G = first.gram[0]
            assert_gram_within_bound(G, gref, what)  # (NaN and non-zero padding are outside it)
            assert np.all(G[kreal:] == 0) and np.all(G[:, kreal:] == 0), what
            XW = np.zeros((hi - lo, K))
            XW[:, :kreal] = X[lo:hi][:, cols]
            assert np.array_equal(first.XW, XW), f"{what}: the gathered columns are not this rank's rows of X[:, cols]"
            assert_within_bound(first.G, first.loss, lref, what)
            assert _same_bits((first.gram, first.G, first.loss, first.XW), (again.gram, again.G, again.loss, again.XW)), \
                f"{what}: not deterministic"
            assert _same_bits((first.gram, first.G, first.loss), [getattr(out[0][0][int(gx)][0], f) for f in ("gram", "G", "loss")]), \
                f"{what}: not rank 0's bits"
            if prev is not None:
                row_lo = (k_end[-2] // 16) * 16
                assert prev.collectives == len(k_end) + 1, what
                assert np.array_equal(G[:row_lo, :row_lo], prev.gram[0][:row_lo, :row_lo]), f"{what}: the old block changed across an append"
                assert np.array_equal(G[:row_lo, row_lo:], G[row_lo:, :row_lo].T), f"{what}: mirrored entries differ from their counterparts"
        assert np.array_equal(runs[0][0].gram, runs[1][0].gram), f"rank {r}: the gather source changed the Gram's bits"


@pytest.mark.parametrize("split", [_B, _C], ids=_sid)
def test_no_weights_and_no_n_eff_scale_by_the_global_row_count(split):
    """No row weights (ws_gram_kernel<false>) and n_eff NULL: 1 / n_global in every rank's part, not 1 / its own rows."""
    n, p, k_end = 1000, 200, [22, 45]
    X, y = _data(n, p)
    cols = np.random.default_rng(3).choice(p, k_end[-1], replace=False).astype(np.int32)
    Z = np.zeros((2, p))
    Z[0, cols] = np.random.default_rng(4).standard_normal(len(cols))
    gref, lref = _cached(("plain", n, p), lambda: (ws_gram_reference(X, cols), lanes_reference(X, y, Z)))
    bounds = split_bounds(split)

    def work(r, eng):
        lo, hi = bounds[r]
        with eng.dataset(X[lo:hi], y[lo:hi]) as ds:
            ds.set_global_rows(n)
            return _ws_call(eng, ds, Z, cols, k_end, [1, 0], None, None)

    out, counts, _ = run_ranks(len(split), work, timeout_s=TIMEOUT_S)
    assert len(set(counts)) == 1
    for r, res in enumerate(out):
        assert res.n_sets == 1 and res.collectives == len(k_end) + 2
        assert_gram_within_bound(res.gram[0], gref, f"rank {r} of {split}")
        assert_within_bound(res.G, res.loss, lref, f"rank {r} of {split}")
        assert _same_bits((res.gram, res.G, res.loss), (out[0].gram, out[0].G, out[0].loss))


# ---- (c) row sets across ranks ------------------------------------------------------------------------------------------------
def _expected_sets(W, ne):
    first = {}
    return np.array([first.setdefault((W[l].tobytes(), ne[l].tobytes()), len(first)) for l in range(len(ne))], dtype=np.int32)


@pytest.mark.parametrize("split", [_C, _A, _E], ids=_sid)
def test_row_sets_are_agreed_among_the_ranks(split):
    """Fold masks whose folds are a rank's rows (that rank's part of the lane's Gram is exactly zero), two lanes of one set,
    two lanes whose weights differ only on rank 0's rows (one set by rank 1's slices, two sets by the whole weights: two on
    every rank), and a uniform(0, 2) lane whose n_eff is not the sum of its weights."""
    n, p, k_end = 1000, 200, [22, 45]
    X, y = _data(n, p)
    bounds = split_bounds(split)
    rng = np.random.default_rng(len(split))
    cols = rng.choice(p, k_end[-1], replace=False).astype(np.int32)
    rows = []
    for lo, hi in (bounds[0], bounds[-1]):  # the folds: the first and the last rank's rows
        m = np.ones(n)
        m[lo:hi] = 0.0
        rows.append((m, m.sum()))
    u = rng.uniform(0.0, 2.0, n)
    rows += [(u, 0.8 * n), (u.copy(), 0.8 * n)]  # one set
    v = rng.uniform(0.0, 2.0, n)
    v2 = v.copy()
    v2[bounds[0][0]] += 0.25  # differs on rank 0's first row only
    rows += [(v, float(n)), (v2, float(n))]
    rows.append((rng.uniform(0.0, 2.0, n), 0.73 * n + 1.5))
    W = np.array([w for w, _ in rows])
    ne = np.array([e for _, e in rows])
    B = len(rows)
    sets = _expected_sets(W, ne)
    assert sets.tolist() == [0, 1, 2, 2, 3, 4, 5]
    on = (np.arange(B) % 2).astype(np.int32)
    Z = np.random.default_rng(9).standard_normal((B, p))
    off_w = np.ones(p, dtype=bool)
    off_w[cols] = False
    Z[np.ix_(on.astype(bool), off_w)] = 0.0
    grefs = [ws_gram_reference(X, cols, W[int(np.flatnonzero(sets == st)[0])], ne[int(np.flatnonzero(sets == st)[0])])
             for st in range(sets.max() + 1)]
    lref = lanes_reference(X, y, Z, W, ne)

    def work(r, eng):
        lo, hi = bounds[r]
        with eng.dataset(X[lo:hi], y[lo:hi]) as ds:
            ds.set_global_rows(n)
            return [_ws_call(eng, ds, Z, cols, k_end, on, W[:, lo:hi], ne) for _ in range(2)]

    out, counts, _ = run_ranks(len(split), work, timeout_s=TIMEOUT_S)
    assert len(set(counts)) == 1
    for r, (res, again) in enumerate(out):  # (first, on every rank: the sets are those of the whole weights)
        assert res.n_sets == sets.max() + 1 and np.array_equal(res.set_of, sets), (f"rank {r} of {split}", res.set_of.tolist())
    for r, (res, again) in enumerate(out):
        what = f"rank {r} of {split}"
        assert res.collectives == again.collectives == len(k_end) + 2, what
        for st, gref in enumerate(grefs):
            assert_gram_within_bound(res.gram[st], gref, f"{what}, set {st}")
        assert_within_bound(res.G, res.loss, lref, what)
        assert _same_bits((res.gram, res.G, res.loss), (again.gram, again.G, again.loss)), f"{what}: not deterministic"
        assert _same_bits((res.gram, res.G, res.loss), (out[0][0].gram, out[0][0].G, out[0][0].loss)), f"{what}: not rank 0's bits"


# ---- (d) the pass on W --------------------------------------------------------------------------------------------------------
def _mask(kind, B):
    l = np.arange(B)
    return {"all": l >= 0, "none": l < 0, "alternating": l % 2 == 0}[kind].astype(np.int32)


PASS_CASES = [(B, kind) for B in (1, 5, 16) for kind in ("all", "none", "alternating")]


def _pass_inputs(n, p, cols, B, kind):
    def make():
        X, y = _data(n, p)
        on = _mask(kind, B)
        Z, W, ne = lane_inputs(np.random.default_rng(B * 31 + n + len(kind)), n, p, B)
        off_w = np.ones(p, dtype=bool)
        off_w[cols] = False
        Z[np.ix_(on.astype(bool), off_w)] = 0.0
        return on, Z, W, ne, lanes_reference(X, y, Z, W, ne)
    return _cached(("pass", n, p, B, kind), make)


@pytest.mark.parametrize("n,split", [(1000, _B), (1000, _C), (1000, _E), (40, _H)], ids=lambda v: _sid(v) if isinstance(v, tuple) else str(v))
def test_sharded_pass_on_w(n, split):
    """Lanes on W (residuals from this rank's gathered columns) and off it (from its rows of X), every lane with its own point,
    weights and n_eff: gradients and losses inside the whole-X bound, the ranks bit-identical."""
    p, k_end = 200, [37, 61]
    X, y = _data(n, p)
    cols = np.random.default_rng(n).choice(p, k_end[-1], replace=False).astype(np.int32)
    inputs = [_pass_inputs(n, p, cols, B, kind) for B, kind in PASS_CASES]
    bounds = split_bounds(split)

    def work(r, eng):
        lo, hi = bounds[r]
        with eng.dataset(X[lo:hi], y[lo:hi]) as ds:
            ds.set_global_rows(n)
            return [_ws_call(eng, ds, Z, cols, k_end, on, W[:, lo:hi], ne) for on, Z, W, ne, _ in inputs]

    out, counts, _ = run_ranks(len(split), work, timeout_s=TIMEOUT_S)
    assert len(set(counts)) == 1
    for k, ((B, kind), (on, Z, W, ne, ref)) in enumerate(zip(PASS_CASES, inputs)):
        expect = ws_build_expected(k_end, 1, owner=True, sharded=True) + ws_pass_expected(p, B)
        for r in range(len(split)):
            res = out[r][k]
            what = f"{B} lanes, on W: {kind}, rank {r} of {split}"
            assert res.kernels == ";".join(expect), (what, res.kernels)
            assert res.collectives == len(k_end) + 2, what
            assert_within_bound(res.G, res.loss, ref, what)
            assert _same_bits((res.G, res.loss, res.gram, res.set_of), (out[0][k].G, out[0][k].loss, out[0][k].gram, out[0][k].set_of)), \
                f"{what}: not rank 0's bits"


# ---- (e) one rank -------------------------------------------------------------------------------------------------------------
def test_a_single_rank_gives_the_plain_engines_bits():
    """One in-process rank through both entries.  Bit for bit, the Grams included: the staged route sums the same row blocks in
    the same order into the staging matrix, a one-rank all-reduce copies, and the publish copies (the plain engine's owner
    table changes no bit either -- tests/test_working_set_lanes_gpu.py -- and at 1 000 rows the row blocks are the same)."""
    n, p, k_end = 1000, 200, [22, 45]
    X, y = _data(n, p)
    cols = np.random.default_rng(8).choice(p, k_end[-1], replace=False).astype(np.int32)
    B = 5
    on = _mask("alternating", B)
    Z, W, ne = lane_inputs(np.random.default_rng(12), n, p, B)
    off_w = np.ones(p, dtype=bool)
    off_w[cols] = False
    Z[np.ix_(on.astype(bool), off_w)] = 0.0

    def both(eng, ds):
        grads = [ds.gradient_lanes(Z[:b], W[:b], ne[:b], route=route) for route, b in ((0, 4), (1, B))]  # (fused: four lanes at most here)
        return grads, _ws_call(eng, ds, Z, cols, k_end, on, W, ne, want_xw=True)

    def work(r, eng):
        with eng.dataset(X, y) as ds:
            return both(eng, ds)

    out, counts, infos = run_ranks(1, work, timeout_s=TIMEOUT_S)
    assert infos == [(0, 1)] and counts[0] == 2 + len(k_end) + 2
    plain_eng = _engine.get_engine(0)
    with plain_eng.dataset(X, y) as ds:
        grads0, ws0 = both(plain_eng, ds)
    grads1, ws1 = out[0]
    for (G1, l1, k1), (G0, l0, k0) in zip(grads1, grads0):
        assert k1 == k0 and np.array_equal(G1, G0) and np.array_equal(l1, l0)
    assert ws0.collectives == 0 and ws1.collectives == len(k_end) + 2
    assert ws1.kernels.split(";") == [k for k in ws_build_expected(k_end, 1, sharded=True)] + ws_pass_expected(p, B)
    assert ws0.kernels.split(";") == ws_build_expected(k_end, 1, owner=True) + ws_pass_expected(p, B)
    assert ws1.n_sets == ws0.n_sets == B and np.array_equal(ws1.set_of, ws0.set_of)
    assert np.array_equal(ws1.gram, ws0.gram), "the staged route changed the Gram's bits"
    assert _same_bits((ws1.G, ws1.loss, ws1.XW), (ws0.G, ws0.loss, ws0.XW))
    for st in range(B):
        assert np.array_equal(ws1.gram[st][:16, 16:], ws1.gram[st][16:, :16].T)


# ---- what the entries refuse on a row-sharded dataset, before any collective ----------------------------------------------------
def test_refusals_come_before_the_first_collective():
    n, p = 100, 50
    X, y = _data(n, p)
    cols = np.arange(10, dtype=np.int32)
    Z = np.zeros((2, p))

    def work(r, eng):
        lo, hi = split_bounds((60, 40))[r]
        seen = []
        with eng.dataset(X[lo:hi], y[lo:hi]) as ds:
            ds.set_global_rows(n)
            for call, match in ((lambda: ds.gradient_lanes(Z, route=2, cov_index=[0, 0]), "route 2"),
                                (lambda: ds.gradient_lanes(Z, route=0, n_rows=10), "n_rows"),
                                (lambda: ds.working_set_lanes(Z, cols, [10], route=2, cov_index=[0, 0]), "route 2"),
                                (lambda: ds.working_set_lanes(Z, cols, [10], xty=True), "X_W\\^T y"),
                                (lambda: ds.working_set_lanes(Z, cols, [10], xty_build=True), "X_W\\^T y")):
                with pytest.raises(NotImplementedError, match=match):
                    call()
                seen.append(eng.comm_collectives())
        return seen

    out, counts, _ = run_ranks(2, work, timeout_s=TIMEOUT_S)
    assert out == [[0] * 5, [0] * 5] and counts == [0, 0]
