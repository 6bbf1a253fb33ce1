"""The working-set model solver (ws_solve_kernel / ws_refine_lane) alone, against a reference minimiser
(slm_working_set_model_solve, tests/_model_reference.py).

Every case gives distinct values per lane and per position.  MUST-SETTLE cases assert, per lane: settled_bound (derived from
the stopping rule), the distance bound ||x - x*|| <= bound / lambda_min, L <= 1.155 lambda_max, served == 1, fewer than
WS_INNER_MAX iterations, and the write-back contract -- outside W z equals zprev exactly (the start differs from it there on
purpose), beta equals z in mode 0 and still holds the sentinel in mode 1, zsup is numpy's answer, t / have_base / zzero as
ws_refine_lane documents them.  Which fault class of tests/test_model_solver_cpu.py each family would catch:
  edge sizes ............ a column dropped at the end of a product (K - 1, a batch tail of the dense product through L2, the
                          LDS product), the z0 shift of one thread part, a wrong ws_sum width at the TPC switch
  non-zero count ........ a column dropped at a batch tail of the listed product (nnz = 1 mod 12 TPC)
  penalties ............. a threshold not scaled by the step, the ridge factor left out, a group norm one member short, pa in
                          place of pb, groups across tile / wavefront boundaries
  spectral / accelerated  a spectral step that claims a curvature it has not got
  lanes ................. another lane's penalty / Gram / point (bit for bit against the lane alone)
  direct steps .......... a face Hessian with a wrong entry, a projection that leaves the orthant, mu from the wrong factor
MAY-NOT-SETTLE cases assert the monotone rule and the contract only; DECLINES leave nothing written.
"""

import numpy as np
import pytest

from _model_reference import (
    WS_INNER_MAX,
    WS_MAX_REPEATS,
    judge_monotone,
    judge_settled,
    make_case,
    model_minimiser,
    spd,
    spectrum,
    support_case,
    ws_K,
    ws_tpc,
)
from sparselm_amd import _engine

pytestmark = pytest.mark.gpu

COUNTERS = ("refined", "inner_iters", "newton_steps", "newton_fails", "newton_nopd", "newton_factors", "newton_unknowns")


@pytest.fixture(scope="module")
def eng():
    return _engine.get_engine(0)


def _solve(eng, cases, set_of=None, grams=None, **kw):
    """One call for lanes that share W (and the groups): cases[l] is lane l."""
    c0 = cases[0]
    for c in cases:
        assert np.array_equal(c.cols, c0.cols) and c.p == c0.p
    X = np.random.default_rng(1).standard_normal((4, c0.p))  # (no X is read: the dataset carries p, ld and the groups)
    with eng.dataset(X, np.zeros(4)) as ds:
        if c0.gid is not None:
            ds.set_groups(c0.gid, c0.n_groups)
        if grams is None:
            grams = np.stack([c.gram for c in cases])
            set_of = np.arange(len(cases))
        stack = lambda name: np.stack([getattr(c, name) for c in cases])  # noqa: E731
        return ds.working_set_model_solve(c0.cols, grams, stack("zprev"), stack("gprev"), stack("z_start"), stack("a0"),
                                          stack("b0"), stack("d0"), stack("point"), [c.tol for c in cases],
                                          [c.mode for c in cases], set_of=set_of, **kw)


def _zsup(c, z):
    out = np.ones(c.p, dtype=bool)
    out[c.cols] = False
    return int(not np.any(z[out] != 0.0))


def _check_settled(c, o, l=0, record=None, tag=""):
    bad, fig = judge_settled(c.mdl, c.cols, c.zprev, c.z_start, c.mode, c.tol, o.z[l], o.beta[l], int(o.served[l]),
                             float(o.Lw[l if o.Lw.size > 1 else 0]))
    print(f"{tag} lane {l}: k {c.k} kkt {fig.get('kkt')} bound {fig.get('bound')} dist {fig.get('dist')} "
          f"dist_bound {fig.get('dist_bound')} inner {o.inner_iters} newton {o.newton_steps} mu {o.mu[l]} Lw {o.Lw}")
    assert bad == [], bad
    assert o.zsup[l] == _zsup(c, o.z[l])
    assert o.zzero[l] == 0
    if c.mode == 0:
        assert o.t[l] == 1.0 and o.have_base[l] == 1  # (t reset; have_base left alone)
    else:
        assert o.t[l] == 7.0 and o.have_base[l] == 0  # (the refined point is the new base; t left alone)
    assert o.repeats[l] == 1 and o.last_point[l] == l
    return fig


def _check_one(c, o, **kw):
    assert o.refined == 1 and o.inner_iters < WS_INNER_MAX
    return _check_settled(c, o, **kw)


# ---------------------------------------------------------------------------------------------------------------------------
# must settle
# ---------------------------------------------------------------------------------------------------------------------------
EDGE_SIZES = [1, 15, 16, 17, 111, 112, 113, 128, 250, 256, 257, 272, 500, 512]


@pytest.mark.parametrize("preset", [False, True])
@pytest.mark.parametrize("cond", [10.0, 1e3])
@pytest.mark.parametrize("kreal", EDGE_SIZES)
def test_edge_sizes(eng, kreal, cond, preset):
    c = make_case(kreal, 700, 100 + kreal, cond=cond, tol=1e-8, mode=kreal % 2)  # (1e-8: the estimators' default tolerance)
    Lw = [1.05 * spectrum(c.mdl)[1]] if preset else None
    o = _solve(eng, [c], Lw=Lw)
    _check_one(c, o, tag=f"edge {kreal} {cond} {preset}")


@pytest.mark.parametrize("K", [128, 272])
@pytest.mark.parametrize("which", ["0", "1", "12tpc-1", "12tpc", "12tpc+1", "24tpc+1", "K"])
def test_nonzero_count(eng, K, which):
    tpc = ws_tpc(K)
    nnz = {"0": 0, "1": 1, "12tpc-1": 12 * tpc - 1, "12tpc": 12 * tpc, "12tpc+1": 12 * tpc + 1, "24tpc+1": 24 * tpc + 1, "K": K}[which]
    c = support_case(K, 700, nnz, 200 + K)
    assert ws_K(c.k) == K
    ref = model_minimiser(c.mdl)
    assert int(np.count_nonzero(ref.x)) == nnz == int(np.count_nonzero(c.z_start[c.cols]))
    o = _solve(eng, [c])
    _check_one(c, o, tag=f"nnz {K} {which}")
    assert int(np.count_nonzero(o.z[0][c.cols])) == nnz


def test_per_feature_weights_over_six_decades(eng):
    c = make_case(200, 700, 301, tol=1e-8)
    rng = np.random.default_rng(301)
    c.a0[:] = np.geomspace(1e-3, 1e3, c.p)[rng.permutation(c.p)]
    c.a0[c.cols[::7]] = 0.0
    c.point = np.array([0.05, 0.0, 0.0])
    from _model_reference import Model

    c.mdl = Model(c.mdl.G, c.mdl.g0, c.mdl.z0, 0.05 * c.a0[c.cols])
    _check_one(c, _solve(eng, [c]), tag="weights")


@pytest.mark.parametrize("which", ["b", "d", "b+d"])
def test_singleton_groups(eng, which):
    c = make_case(150, 700, 310, penalty="weighted_l1_ridge", tol=1e-8)
    from _model_reference import Model

    sa = c.point[0]
    sb = sa if "b" in which else 0.0
    sd = c.point[2] if "d" in which else 0.0
    c.point = np.array([0.5 * sa, sb, sd])
    c.mdl = Model(c.mdl.G, c.mdl.g0, c.mdl.z0, 0.5 * sa * c.a0[c.cols], sb * c.b0[c.cols], sd * c.d0[c.cols])
    _check_one(c, _solve(eng, [c]), tag=f"singleton {which}")


GROUP_SIZES = [1, 2, 8, 16, 17, 200, 3, 16, 5]  # (groups that straddle 16-tiles and wavefronts)


@pytest.mark.parametrize("penalty", ["group", "sparse_group", "ridged_group"])
def test_real_groups(eng, penalty):
    c = make_case(sum(GROUP_SIZES), 700, 320, penalty=penalty, group_sizes=GROUP_SIZES, tol=1e-8, strength=0.15)
    _check_one(c, _solve(eng, [c]), tag=penalty)


def test_grouped_dataset_without_group_term(eng):
    """sb = sd = 0 on a dataset with real groups: the grouped instance with no group curvature."""
    c = make_case(sum(GROUP_SIZES), 700, 321, penalty="sparse_group", group_sizes=GROUP_SIZES, tol=1e-8)
    from _model_reference import Model

    c.point = np.array([c.point[0], 0.0, 0.0])
    c.mdl = Model(c.mdl.G, c.mdl.g0, c.mdl.z0, c.mdl.a, 0.0, 0.0, c.mdl.gidx)
    o = _solve(eng, [c])
    assert o.kernels.startswith("ws_solve_kernel<true,0>")
    _check_one(c, o, tag="grouped sb=0")


def test_whole_groups_zero_and_others_active(eng):
    c = make_case(sum(GROUP_SIZES), 700, 322, penalty="group", group_sizes=GROUP_SIZES, tol=1e-8, strength=0.15)
    from _model_reference import Model

    heavy = np.arange(c.mdl.ng) % 2 == 1  # (every other group of W pays fifty times as much)
    c.b0[np.unique(c.gid[c.cols[np.isin(c.mdl.gidx, np.flatnonzero(heavy))]])] *= 50.0
    c.mdl = Model(c.mdl.G, c.mdl.g0, c.mdl.z0, c.mdl.a, np.where(heavy, 50.0, 1.0) * c.mdl.b, c.mdl.d, c.mdl.gidx)
    ref = model_minimiser(c.mdl)
    norms = np.array([np.linalg.norm(ref.x[m].astype(float)) for m in c.mdl.members])
    assert np.any(norms == 0.0) and np.any(norms > 0.0)
    o = _solve(eng, [c])
    _check_one(c, o, tag="zero groups")
    got = np.array([np.linalg.norm(o.z[0][c.cols][m]) for m in c.mdl.members])
    assert np.array_equal(got == 0.0, norms == 0.0)


@pytest.mark.parametrize("kreal", [100, 300])
def test_spectral_and_accelerated_steps_agree(eng, kreal, monkeypatch):
    c = make_case(kreal, 700, 330 + kreal, cond=100.0, tol=1e-8)
    o1 = _solve(eng, [c])
    f1 = _check_one(c, o1, tag="bb default")
    monkeypatch.setenv("SLM_WS_BB", "0")
    o0 = _solve(eng, [c])
    f0 = _check_one(c, o0, tag="bb 0")
    assert np.linalg.norm(o1.z[0] - o0.z[0]) <= (f1["bound"] + f0["bound"]) / f1["lam_min"]


def _lanes(n_lanes, kreal, seed, n_sets):
    pens = ["lasso", "weighted_l1_ridge"]
    return [make_case(kreal, 700, seed, penalty=pens[l % 2], tol=[1e-6, 1e-8, 1e-10][l % 3], mode=(l // 2) % 2, lane=l,
                      cond=[10.0, 30.0, 100.0][l % 3] if n_sets == n_lanes else 10.0,
                      gram_seed=seed + 1000 * (l % n_sets), strength=0.1 + 0.05 * (l % 5)) for l in range(n_lanes)]


@pytest.mark.parametrize("n_lanes,n_sets", [(1, 1), (5, 2), (18, 5), (32, 2), (32, 5)])
def test_lanes_match_each_lane_alone(eng, n_lanes, n_sets):
    cases = _lanes(n_lanes, 130, 400 + n_lanes, n_sets)
    set_of = np.arange(n_lanes) % n_sets
    grams = np.stack([cases[s].gram for s in range(n_sets)])
    o = _solve(eng, cases, set_of=set_of, grams=grams)
    assert o.refined == n_lanes
    for l, c in enumerate(cases):
        alone = _solve(eng, [c])
        assert np.array_equal(o.z[l], alone.z[0]) and np.array_equal(o.beta[l], alone.beta[0], equal_nan=True), l
        assert o.mu[l] == alone.mu[0] and o.zsup[l] == alone.zsup[0] and o.served[l] == 1
        _check_settled(c, alone, tag=f"lanes {n_lanes}/{n_sets} alone {l}")


def _hard_case(kind, cond, seed, least_squares=True):
    """An ill-conditioned face.  g0 is the gradient of a least-squares loss whose unpenalised minimiser lies a distance of order
    one from the expansion point (make_case): what a pass over X delivers.  (With g0 drawn freely the model's minimiser lies
    1 / lambda_min away through that many more sign changes; measured: at condition 1e8 the per-feature solve then uses up
    all its direct steps and is accepted by the monotone rule alone -- allowed for a solve that does not settle, so that draw
    sits among the may-not-settle cases below.)"""
    if kind == "lasso":
        return make_case(120, 700, seed, cond=cond, penalty="lasso", tol=1e-8, strength=0.05, least_squares=least_squares)
    return make_case(sum(GROUP_SIZES[:5]) + 40, 700, seed, cond=cond, penalty="group", group_sizes=GROUP_SIZES[:5] + [40], tol=1e-8,
                     strength=0.05, least_squares=least_squares)


@pytest.mark.parametrize("cond", [1e6, 1e8])
@pytest.mark.parametrize("kind", ["lasso", "group"])
def test_direct_steps(eng, kind, cond, monkeypatch, record_property):
    c = _hard_case(kind, cond, 500)
    o = _solve(eng, [c], direct=True)
    fig = _check_one(c, o, tag=f"direct {kind} {cond}")
    assert o.newton_steps > 0 and o.hard_lane[0] == 1
    lam_min, lam_max = fig["lam_min"], fig["lam_max"]
    # mu is half a Rayleigh quotient of the Gram or half an inverse-iteration estimate of a face Hessian's smallest eigenvalue
    assert o.mu[0] > 0.0
    assert 0.5 * lam_min * (1.0 - 1e-9) <= o.mu[0] <= 0.5 * lam_max
    ratio = o.mu[0] / fig["ref"].face_min_eig
    record_property("mu_over_face_lambda_min", ratio)
    print(f"mu ratio {kind} {cond}: mu {o.mu[0]} face lambda_min {fig['ref'].face_min_eig} ratio {ratio}")
    # the two launches and the one solver give the same bits
    monkeypatch.setenv("SLM_WS_ONE_SOLVER", "1")
    o1 = _solve(eng, [c], direct=True)
    assert o1.kernels in ("ws_solve_kernel<false,1>", "ws_solve_kernel<true,1>")
    assert np.array_equal(o1.z, o.z) and np.array_equal(o1.beta, o.beta, equal_nan=True) and o1.mu[0] == o.mu[0]
    monkeypatch.delenv("SLM_WS_ONE_SOLVER")


@pytest.mark.parametrize("cond", [1e6, 1e8])
@pytest.mark.parametrize("kind", ["lasso", "group"])
def test_start_hard(eng, kind, cond):
    """WsCtl::hard_lane preset: the solve opens in direct mode and must still end within the bound.

    The regression test of WS_NEWTON_MAX (ws_kernels.hpp): with 64 direct steps per refinement lasso / 1e8 used them up, ran
    the 40 iterations left to it and ended unsettled after 104 iterations, model_kkt 5.2e-3 against a bound of 3.6e-9 and 2.3
    from the minimiser against 0.68 (accepted by the monotone rule alone).  In direct mode on such a face one coordinate
    changes sides per step; from this start (80 of 120 coordinates non-zero, 30 at the minimiser) the solve takes 129."""
    c = _hard_case(kind, cond, 500)
    oh = _solve(eng, [c], direct=True, hard=True)
    assert oh.want_full[0] == 0
    _check_one(c, oh, tag=f"hard {kind} {cond}")


# kind, positions, preset direct mode -- each the smallest case of one regime of a direct step (faces of 5, 32, 105, 51 and
# 148 non-zeros at the minimiser):
REGIMES = [("lasso", 16, True),           # a face of one 16-tile; hard presets direct mode, so a direct step is certain
           ("lasso", 100, False),         # K = 112, the largest Gram held in LDS; two tiles
           ("lasso", 300, False),         # K = 304: two threads per position, Gram through L2
           ("sparse_group", 84, False),   # the l1 kink inside active groups
           ("sparse_group", 300, False)]  # the same with two threads per position and the 200-member group
REGIMES_UNSETTLED = REGIMES[4:]  # (measured: 4 direct steps, 39 factorisations, 57 iterations, model_kkt 1.5e-3 against a bound
                                 #  of 1.6e-8 -- the solve uses up its refusals and ends unsettled; test_regime_that_does_not_settle)


def _regime_case(kind, k):
    sizes = None if kind == "lasso" else GROUP_SIZES[:5] + [40] if k == 84 else GROUP_SIZES[:6] + [56]
    return make_case(k, 700, 500, cond=1e6, tol=1e-8, strength=0.05, least_squares=True, penalty=kind, group_sizes=sizes)


def _regime_solve(eng, kind, k, hard, monkeypatch):
    """The solve of one regime, with what holds whether or not it settles: direct steps were taken, and the two launches and
    the one solver give the same bits."""
    c = _regime_case(kind, k)
    if kind == "sparse_group":
        assert c.point[0] > 0.0 and c.point[1] > 0.0  # (an l1 term AND a group term)
    o = _solve(eng, [c], direct=True, hard=hard)
    print(f"regime {kind} {k}: inner {o.inner_iters} newton {o.newton_steps} factors {o.newton_factors} unknowns {o.newton_unknowns} "
          f"nnz {np.count_nonzero(o.z[0][c.cols])}")
    if hard:  # (test_start_hard's)
        assert o.want_full[0] == 0 and o.newton_factors > 0
    else:  # (test_direct_steps')
        assert o.newton_steps > 0 and o.hard_lane[0] == 1
        monkeypatch.setenv("SLM_WS_ONE_SOLVER", "1")
        o1 = _solve(eng, [c], direct=True)
        assert o1.kernels in ("ws_solve_kernel<false,1>", "ws_solve_kernel<true,1>")
        assert np.array_equal(o1.z, o.z) and np.array_equal(o1.beta, o.beta, equal_nan=True) and o1.mu[0] == o.mu[0]
        monkeypatch.delenv("SLM_WS_ONE_SOLVER")
    return c, o


@pytest.mark.parametrize("kind,k,hard", REGIMES[:4])
def test_direct_steps_by_regime(eng, kind, k, hard, monkeypatch):
    c, o = _regime_solve(eng, kind, k, hard, monkeypatch)
    fig = _check_one(c, o, tag=f"regime {kind} {k}")
    if not hard:
        assert o.mu[0] > 0.0
        assert 0.5 * fig["lam_min"] * (1.0 - 1e-9) <= o.mu[0] <= 0.5 * fig["lam_max"]


# ---------------------------------------------------------------------------------------------------------------------------
# may not settle: the monotone rule and the write-back contract only
# ---------------------------------------------------------------------------------------------------------------------------
def _check_monotone(c, o, tag):
    bad = judge_monotone(c.mdl, c.cols, c.zprev, c.z_start, c.mode, o.z[0], o.beta[0], int(o.served[0]))
    print(f"{tag}: served {o.served[0]} inner {o.inner_iters} newton {o.newton_steps} nopd {o.newton_nopd}")
    assert bad == [], bad


@pytest.mark.parametrize("kind,k,hard", REGIMES_UNSETTLED)
def test_regime_that_does_not_settle(eng, kind, k, hard, monkeypatch):
    """The l1 kink inside active groups with two threads per position and the 200-member group: the solve takes direct steps
    and ends unsettled (REGIMES_UNSETTLED), so what it returns is judged by the monotone rule, as _hard_case describes for the
    freely drawn gradient."""
    c, o = _regime_solve(eng, kind, k, hard, monkeypatch)
    assert o.refined == 1
    _check_monotone(c, o, f"regime {kind} {k}")


@pytest.mark.parametrize("cond", [1e6, 1e8])
@pytest.mark.parametrize("kind", ["lasso", "group"])
def test_ill_conditioned_without_direct_steps(eng, kind, cond):
    c = _hard_case(kind, cond, 500)
    o = _solve(eng, [c], direct=False)
    assert o.newton_steps == 0 and o.kernels.count(";") == 0
    _check_monotone(c, o, f"no direct {kind} {cond}")


@pytest.mark.parametrize("cond", [1e6, 1e8])
def test_free_gradient_on_an_ill_conditioned_face(eng, cond):
    """g0 drawn freely (see _hard_case): the solve may use up its direct steps; what it returns is no worse than the start."""
    c = _hard_case("lasso", cond, 500, least_squares=False)
    _check_monotone(c, _solve(eng, [c], direct=True), f"free g0 {cond}")


def test_singular_gram(eng):
    """A duplicated column: the face is not positive definite, the direct steps are refused, the iteration carries on."""
    k = 60
    A = np.random.default_rng(600).standard_normal((200, k))
    A *= np.geomspace(1.0, 1e-3, k)  # (ill-conditioned enough to ask for direct steps)
    A[:, 1] = A[:, 0]
    c = make_case(k, 700, 600, G=A.T @ A / 200, tol=1e-10, strength=0.01)
    c.a0[c.cols[:2]] = 0.0  # (both copies free and non-zero: the face holds the singular pair)
    c.z_start[c.cols[:2]] = [0.3, -0.2]
    from _model_reference import Model

    c.mdl = Model(c.mdl.G, c.mdl.g0, c.mdl.z0, c.point[0] * c.a0[c.cols])
    o = _solve(eng, [c], direct=True, hard=True)
    assert o.newton_nopd > 0
    _check_monotone(c, o, "singular")


def test_indefinite_gram(eng):
    G = spd(40, 10.0, 610)
    w, Q = np.linalg.eigh(G)
    w[0] = -0.2 * w[-1]
    G = (Q * w) @ Q.T
    c = make_case(40, 700, 610, G=0.5 * (G + G.T), tol=1e-8)
    _check_monotone(c, _solve(eng, [c], direct=True), "indefinite")


# ---------------------------------------------------------------------------------------------------------------------------
# declines: nothing written
# ---------------------------------------------------------------------------------------------------------------------------
def _check_untouched(c, o):
    assert np.array_equal(o.z[0], c.z_start) and np.all(np.isnan(o.beta[0]))
    assert o.served[0] == 0 and o.mu[0] == -1.0 and o.t[0] == 7.0 and o.have_base[0] == 1 and o.zzero[0] == 1
    assert all(getattr(o, n) == 0 for n in COUNTERS)
    assert o.Lw[0] == 0.0


@pytest.mark.parametrize("flag", ["invalid", "building", "disabled"])
def test_declines_on_the_working_sets_state(eng, flag):
    c = make_case(50, 700, 700)
    o = _solve(eng, [c], **{flag: True})
    _check_untouched(c, o)
    assert o.zsup[0] == 0 and o.repeats[0] == 0  # (no usable W: the point does not count as on it)


def test_declines_when_stale_and_moved_outside(eng):
    c = make_case(50, 700, 701)
    o = _solve(eng, [c], stale=True)  # (the start differs from zprev outside W)
    _check_untouched(c, o)
    out = np.ones(c.p, dtype=bool)
    out[c.cols] = False
    c.z_start[out] = c.zprev[out]
    c.tol = 1e-8
    _check_one(c, _solve(eng, [c], stale=True), tag="stale, nothing moved")


def test_declines_after_too_many_repeats(eng):
    c = make_case(50, 700, 702, tol=1e-8)
    o = _solve(eng, [c], repeats=WS_MAX_REPEATS, last_point=0, last_cols=c.k)
    _check_untouched(c, o)
    assert o.repeats[0] == WS_MAX_REPEATS
    o = _solve(eng, [c], repeats=WS_MAX_REPEATS - 1, last_point=0, last_cols=c.k)
    assert o.served[0] == 1 and o.repeats[0] == WS_MAX_REPEATS
    # (the same count at another point, or with fewer columns then, is a new matter)
    assert _solve(eng, [c], repeats=WS_MAX_REPEATS, last_point=3, last_cols=c.k).served[0] == 1
    assert _solve(eng, [c], repeats=WS_MAX_REPEATS, last_point=0, last_cols=c.k - 1).served[0] == 1


@pytest.mark.parametrize("where", ["gram", "gprev"])
@pytest.mark.parametrize("value", [np.nan, np.inf])
@pytest.mark.parametrize("preset", [False, True])
def test_declines_on_non_finite_model(eng, where, value, preset):
    c = make_case(50, 700, 703)
    Lw = [1.05 * spectrum(c.mdl)[1]] if preset else None
    if where == "gram":
        c.gram[7, 9] = c.gram[9, 7] = value
    else:
        c.gprev[c.cols[11]] = value
    o = _solve(eng, [c], allow_nonfinite=True, Lw=Lw)
    assert np.array_equal(o.z[0], c.z_start) and np.all(np.isnan(o.beta[0]))
    assert o.served[0] == 0 and o.mu[0] == -1.0 and all(getattr(o, n) == 0 for n in COUNTERS)


# ---------------------------------------------------------------------------------------------------------------------------
# launches and arguments
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True])
def test_kernels_launched(eng, grouped, monkeypatch):
    g = "true" if grouped else "false"
    c = make_case(24, 700, 800, penalty="group" if grouped else "lasso", group_sizes=[8, 16] if grouped else None, tol=1e-8)
    assert _solve(eng, [c], direct=True).kernels == f"ws_solve_kernel<{g},0>;ws_solve_kernel<{g},1>"
    assert _solve(eng, [c], direct=False).kernels == f"ws_solve_kernel<{g},0>"
    monkeypatch.setenv("SLM_WS_ONE_SOLVER", "1")
    assert _solve(eng, [c], direct=True).kernels == f"ws_solve_kernel<{g},1>"
    assert _solve(eng, [c], direct=False).kernels == f"ws_solve_kernel<{g},0>"


def test_bad_arguments_are_refused(eng):
    c = make_case(24, 700, 810, penalty="group", group_sizes=[8, 16])

    def refused(**changes):
        d = make_case(24, 700, 810, penalty="group", group_sizes=[8, 16])
        kw = {}
        for name, v in changes.items():
            if name in ("flags",):
                kw[name] = v
            else:
                setattr(d, name, v)
        with pytest.raises((_engine.EngineError, ValueError)):
            _solve(eng, [d], **kw)

    cols = c.cols.copy()
    cols[3] = cols[2]
    refused(cols=cols)  # repeated
    members = np.flatnonzero(c.gid == c.gid[c.cols[0]])
    other = np.setdiff1d(np.arange(c.p), c.cols)
    cols = c.cols.copy()
    cols[0] = other[np.flatnonzero(np.bincount(c.gid)[c.gid[other]] == 3)[0]]
    assert members.size in (8, 16)
    refused(cols=cols)  # a split group
    for name in ("zprev", "z_start", "a0", "b0", "d0", "gprev", "gram"):
        v = getattr(c, name).copy()
        v.flat[5] = np.nan
        refused(**{name: v})
    refused(flags=1 << 20)
    pad = c.gram.copy()
    assert ws_K(c.k) > c.k
    pad[-1, -1] = 1.0
    refused(gram=pad)  # a non-zero entry on the padding
    with pytest.raises((_engine.EngineError, ValueError)):  # K over 512
        X = np.zeros((4, 700))
        with eng.dataset(X, np.zeros(4)) as ds:
            k = 513
            ds.working_set_model_solve(np.arange(k), np.zeros((1, 528, 528)), np.zeros((1, 700)), np.zeros((1, 700)),
                                       np.zeros((1, 700)), np.ones((1, 700)), np.zeros((1, 700)), np.zeros((1, 700)),
                                       np.array([[1.0, 0, 0]]), 1e-8, 0)
