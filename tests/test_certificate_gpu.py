"""Every point of a path, on every route that can accept one, audited against X (tests/_certificate.py): the reported point's
distance to optimality may not exceed what its own KKT record allows, and the record meets the tail's acceptance rule.

The point tests elsewhere compare a path with the oracle at a few chosen points, to a tolerance relative to max|beta|: a
column certified out on a gradient that was wrong there -- the one failure a certified partial pass (csrc/light_kernels.hpp)
can have -- shows as a small violation of that column's optimality condition, which only an audit of every point sees.
Each case also checks, through the counters PathResult reports, that its route was taken."""

import re

import numpy as np
import pytest

from _certificate import assert_certified, audit_path, lambda_max
from sparselm_amd import _engine
from sparselm_amd.distributed import row_range

pytestmark = pytest.mark.gpu

WS = _engine.FLAG_WORKING_SET | _engine.FLAG_FRESH_L


@pytest.fixture(scope="module")
def eng():
    return _engine.get_engine(0)


def _noisy(n, p, k, seed, noise=3.0):
    """A path whose end sits at the noise floor: features no earlier gradient can tell enter at its last points."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p))
    beta = np.zeros(p)
    beta[rng.choice(p, k, replace=False)] = 30.0 * rng.uniform(0.1, 1.0, k)
    return X, X @ beta + noise * rng.standard_normal(n)


def _penalty(kind, X, y, K, rng):
    """(points, a, groups) of a path from the top of `kind`'s range down to 1e-3 of it."""
    n, p = X.shape
    g0 = X.T @ y / n
    if kind in ("l1", "weighted"):
        a = rng.uniform(0.5, 2.0, p) if kind == "weighted" else None
        top = float(np.max(np.abs(g0) / (1.0 if a is None else a)))
        return [(s, 0.0, 0.0) for s in np.geomspace(top, 1e-3 * top, K)], a, None
    G = p // 10
    groups = rng.permutation(np.repeat(np.arange(G), 10)).astype(np.int32)
    top = float(np.max(np.sqrt(np.bincount(groups, weights=g0 * g0, minlength=G))))
    l1 = 0.0 if kind == "group" else 0.4
    return [(l1 * s, (1.0 - l1) * s, 0.0) for s in np.geomspace(top, 1e-2 * top, K)], None, groups


# ---- certified partial passes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [1, 2, 3, 4, 8])
def test_light_pass_paths_are_certified_at_every_point(eng, monkeypatch, lanes):
    """Misses forced by a small first working set and small appends (SLM_WS_KINIT / SLM_WS_APPEND), lag hand-over on and off
    (SLM_NO_LAG_HANDOVER), four penalty kinds; every path misses and -- on a shared path -- takes light passes.  Light passes
    need a shared path (PathCall::light_eligible): one lane walks its path alone and re-verifies over X, audited all the
    same."""
    monkeypatch.setenv("SLM_WS_KINIT", "16")
    monkeypatch.setenv("SLM_WS_APPEND", "4")
    for seed, kind in enumerate(("l1", "weighted", "group", "sparse-group")):
        X, y = _noisy(10_000, 1000, 25, 1000 + 4 * lanes + seed)
        pts, a, groups = _penalty(kind, X, y, 36, np.random.default_rng(seed))
        L_true = lambda_max(X)
        with eng.dataset(X, y) as ds:
            if groups is not None:
                ds.set_groups(groups, int(groups.max()) + 1)
            for lag in ("", "1"):
                if lag:
                    monkeypatch.setenv("SLM_NO_LAG_HANDOVER", lag)
                res = ds.solve_path(pts, a=a, lanes=lanes, flags=WS)
                monkeypatch.delenv("SLM_NO_LAG_HANDOVER", raising=False)
                assert res.converged and res.ws_misses > 0, (kind, lag)
                assert lanes == 1 or res.light_passes > 0, (kind, lag)
                assert_certified(res, pts, X=X, y=y, a=a, groups=groups, L_true=L_true)


@pytest.mark.parametrize("lanes", [18, 24])
def test_wide_lane_paths_are_certified_at_every_point(eng, lanes):
    """17-20 lanes (the vector unit's xtr kernels) and 21-32 (the second MFMA block)."""
    X, y = _noisy(16_000, 1500, 30, lanes)
    pts, _, _ = _penalty("l1", X, y, 64, None)
    with eng.dataset(X, y) as ds:
        res = ds.solve_path(pts, lanes=lanes, flags=WS)
    assert res.converged and res.ws_refined > 0
    assert_certified(res, pts, X=X, y=y)


def test_model_gram_rounds_are_certified_at_every_point(eng, monkeypatch):
    monkeypatch.setenv("SLM_MG", "2")  # (rounds at any size, from the first snapshot on)
    rng = np.random.default_rng(640)
    n, p = 4000, 640
    X = rng.standard_normal((n, p))
    bt = np.zeros(p)
    bt[rng.choice(p, 30, replace=False)] = 10 * rng.uniform(0.2, 1.0, 30)
    y = X @ bt + 100.0 * rng.standard_normal(n)
    pts, _, _ = _penalty("l1", X, y, 40, None)
    with eng.dataset(X, y) as ds:
        res = ds.solve_path(pts, lanes=16, flags=_engine.FLAG_WORKING_SET, tol=1e-9)
    assert res.converged and res.mg_rounds > 0
    assert_certified(res, pts, X=X, y=y, tol=1e-9)


def test_covariance_passes_under_fold_masks_are_certified_at_every_point(eng):
    rng = np.random.default_rng(4)
    n, p = 5000, 300
    X = rng.standard_normal((n, p))
    bt = np.zeros(p)
    bt[rng.choice(p, 20, replace=False)] = rng.uniform(1.0, 3.0, 20)
    y = X @ bt + rng.standard_normal(n)
    G = p // 10
    groups = rng.permutation(np.repeat(np.arange(G), 10)).astype(np.int32)
    folds = rng.permutation(n) % 4
    masks = [(folds != f).astype(float) for f in range(4)]
    nes = [int(m.sum()) for m in masks]
    with eng.dataset(X, y) as ds:
        ds.set_groups(groups, G)
        ds.covariance_folds(masks, nes)
        assert ds.covariance_count() == 4
        g0, _ = ds.gradient(None)
        al = np.geomspace(float(np.max(np.abs(g0))), 0.02 * float(np.max(np.abs(g0))), 8)
        specs = [dict(points=np.c_[0.4 * al, 0.6 * al, 0 * al] * (1 + 0.1 * (l // 4)), row_weight=masks[l % 4], n_eff=nes[l % 4])
                 for l in range(8)]
        out = ds.solve_lanes(specs, tol=1e-10, flags=_engine.FLAG_WORKING_SET | _engine.FLAG_COVARIANCE)
    for spec, res in zip(specs, out):
        assert res.converged
        assert_certified(res, spec["points"], X=X, y=y, groups=groups, tol=1e-10, row_weight=spec["row_weight"], n_eff=spec["n_eff"])


@pytest.mark.parametrize("n_ranks", [2, 3])
def test_row_sharded_paths_are_certified_at_every_point(n_ranks):
    """Two and three in-process ranks (slm_comm_init_local), each holding its rows: every rank's points against all of X."""
    import threading

    rng = np.random.default_rng(n_ranks)
    n, p = 6001, 400
    X = rng.standard_normal((n, p)) + 0.3
    bt = np.zeros(p)
    bt[rng.choice(p, 12, replace=False)] = rng.uniform(1, 4, 12) * rng.choice([-1, 1], 12)
    y = X @ bt + 0.5 * rng.standard_normal(n) + 2.0
    pts, _, _ = _penalty("l1", X, y, 12, None)
    engines = [_engine.Engine(0) for _ in range(n_ranks)]
    _engine.init_local_comm(engines, timeout_s=30.0)
    out, err = [None] * n_ranks, [None] * n_ranks

    def body(r):
        try:
            lo, hi = row_range(n, r, n_ranks)
            with engines[r].dataset(X[lo:hi], y[lo:hi]) as ds:
                ds.set_global_rows(n)
                out[r] = ds.solve_path(pts, tol=1e-10, flags=_engine.FLAG_WORKING_SET, lanes=2)
        except BaseException as exc:  # noqa: BLE001 - re-raised below
            err[r] = exc

    threads = [threading.Thread(target=body, args=(r,)) for r in range(n_ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    counts = [e.comm_collectives() for e in engines]
    for e in engines:
        e.comm_destroy()
        e.close()
    for exc in err:
        if exc is not None:
            raise exc
    assert counts[0] > 0 and len(set(counts)) == 1
    L_true = lambda_max(X)
    for res in out:
        assert res.converged and res.ws_refined > 0
        assert_certified(res, pts, X=X, y=y, tol=1e-10, L_true=L_true)


# ---- chained light passes: a base gradient that is itself a hybrid one ------------------------------------------------

_PASS = re.compile(r"\[slm\] pass (\d+) .*\| light (\d+) of (\d+) .*\| lanes \(point\.iter/flags\):(.*?) \| lt id (\d+) ok (\d+) "
                   r"\| lanes \(rejects/epoch/slack\):(.*)$")


def parse_trace(text):
    """The SLM_TRACE=3 lines of a solve: per polled pass, (pass, used, attempts, id, ok, [(done, rejects, epoch, slack)])."""
    out = []
    for line in text.splitlines():
        m = _PASS.search(line)
        if not m:
            continue
        flags = m.group(4).split()
        lt = [tuple(v.split("/")) for v in m.group(7).split()]
        lanes = [("d" in f, int(r), int(e), float(s)) for f, (r, e, s) in zip(flags, lt)]
        out.append((int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(5)), int(m.group(6)), lanes))
    return out


def chained(snaps):
    """Passes whose standing attempt served a lane on a hybrid base gradient: the lane's epoch was an earlier attempt's and is
    now this one's (it accepted a point on the new hybrid gradient)."""
    out = []
    for t in range(1, len(snaps)):
        _, used0, _, _, _, lanes0 = snaps[t - 1]
        pas, used, _, lid, ok, lanes = snaps[t]
        if ok == 1 and used > used0:
            out += [(pas, l) for l, (_, _, ep, _) in enumerate(lanes) if ep == lid and 0 < lanes0[l][2] < lid]
    return out


# Seeds 7 and 11 (weighted l1, two lanes, forced misses) came out of a bounded search over 384 light-pass paths (seeds 0-11 x
# lanes 2/3/4/8 x four penalty kinds x default / forced misses), the only two whose last point failed the audit: dist(0, dF)
# 3.5e-5 and 6.2e-4 against bounds of 2.2e-8 and 2.5e-8, on ACTIVE columns that had entered as borderline columns.  Their
# light passes come in chains: the borderline columns of an attempt on a hybrid base gradient took g_j(z) + X_j^T dR / n,
# which carries the base's error on a column the attempt before had not read (light_kernels.hpp, top).
@pytest.mark.parametrize("seed", [7, 11])
def test_chained_light_passes_keep_their_certificate(eng, monkeypatch, capfd, seed):
    """Traced (SLM_TRACE=3: per polled pass each lane's rejects and the epoch / slack of its base gradient): tracing changes no
    bit; the path takes a light pass on a hybrid base gradient; the bookkeeping obeys its invariant -- an epoch names an
    attempt that has been made, a base gradient from a pass over X (epoch 0) carries no slack; and every point is certified."""
    monkeypatch.setenv("SLM_WS_KINIT", "16")
    monkeypatch.setenv("SLM_WS_APPEND", "4")
    X, y = _noisy(10_000, 1000, 25, 1000 + seed)
    pts, a, _ = _penalty("weighted", X, y, 36, np.random.default_rng(seed))
    with eng.dataset(X, y) as ds:
        plain = ds.solve_path(pts, a=a, lanes=2, flags=WS)
        capfd.readouterr()
        monkeypatch.setenv("SLM_TRACE", "3")
        traced = ds.solve_path(pts, a=a, lanes=2, flags=WS)
        monkeypatch.delenv("SLM_TRACE")
    snaps = parse_trace(capfd.readouterr().err)
    assert np.array_equal(plain.betas, traced.betas) and plain.light_passes == traced.light_passes > 0
    assert plain.converged
    assert chained(snaps), snaps
    for _, used, att, lid, ok, lanes in snaps:
        assert used <= att and lid == att
        for done, rej, ep, slack in lanes:
            assert 0 <= ep <= lid and (ep != 0 or slack == 0.0) and rej >= 0
    assert_certified(plain, pts, X=X, y=y, a=a)


def test_device_generated_data_is_audited_through_its_own_gradient(eng):
    """Draw 1004 of the headline's law (test_baseline_configs_gpu: the path whose lanes hand a tail point over, three passes),
    100k x 5k generated on the device, solved twice: the audit takes its gradients from Dataset.gradient and lambda_max from
    power steps on them."""
    N, P = 100_000, 5_000
    rng = np.random.default_rng(0)
    coef = np.zeros(P)
    coef[rng.choice(P, size=50, replace=False)] = 100.0 * rng.uniform(size=50)
    with eng.synthetic_dataset(N, P, seed=1004, coef=coef, noise_sd=10.0) as ds:
        g0, _ = ds.gradient(None)
        amax = float(np.max(np.abs(g0)))
        pts = [(a, 0.0, 0.0) for a in np.geomspace(amax, 1e-3 * amax, 50)]
        first = ds.solve_path(pts, lanes=0, flags=_engine.FLAG_FRESH_L)
        res = ds.solve_path(pts, lanes=0, flags=_engine.FLAG_FRESH_L)
        assert first.converged and res.converged and first.grad_launches == 3
        L_true = lambda_max(None, gradient=lambda b: ds.gradient(b)[0], p=P)
        for r in (first, res):
            assert_certified(r, pts, gradient=lambda b: ds.gradient(b)[0], L_true=L_true)
