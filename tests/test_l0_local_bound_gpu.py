"""The local bound on the GPU (``slm_solve_l0_local_bound``, ``l0_local_bound_kernel`` in csrc/l0_local_bound_kernels.hpp).

1. The kernel equals the host twin: on the device's own Gram (downloaded, so that no rounding of the Gram build stands between
   them) ``u_out``, sweeps, status, bound and relaxed value equal the numpy restatement of the rule BIT FOR BIT -- the restatement
   that tests/test_l0_local_bound_cpu.py shows to equal the host twin bit for bit -- and the bound is within the certificate's
   tolerance of ``lower_bound`` evaluated by plain numpy products at the kernel's own ``u_out``: the certificate is checked, not
   the route.  Shapes (tests/_l0_local_bound_cases.py): one column, the slot edges 63 / 64 / 65 / 130, 1024 columns on 40 rows,
   a rank-deficient 12 x 20 design with a zero column.
2. The bound is a bound: on the hard law (30 x 10, AR(1) 0.9, seeds 0..2) at every cell of eta {0, 0.01, 1} x M {0.7, 100} x alpha
   {1e-3, 0.1, 0.5}, ``lower_bounds_ <= F*_bruteforce + 1e-9 max(|F*|, alpha)``, no cell excluded; ``gap(l0_local_search) >= -1e-9``
   at the slot-edge shapes.
3. Where ``converged_`` holds the bound is the relaxation's optimum as an independent solver (FISTA, own gap <= 1e-10) finds it.
4. One sweep is still a bound.  5. A warm start from an ``L0LocalPath``.  6. ``big_M = 0``, ``alpha = 0``, ``eta = 0``.
7. The surface: an intercept and sample weights through the same Gram, both routes bit for bit, the import and every refusal's
   class by either route (the ctypes leg runs whether or not the binding loads)."""

import functools
import warnings

import numpy as np
import pytest
from sklearn.exceptions import ConvergenceWarning

from _l0_local_bound_cases import cases, draw, run_rule
from _l0_local_bound_reference import ALPHAS, BIG_MS, ETAS, brute_force, certificate_tolerance, fista, hard_problem, lower_bound, objective
from _l0_local_reference import gram

pytestmark = pytest.mark.gpu

SLACK = 1e-9  # of max(|F*|, alpha): the issue's allowance for the rounding of the certificate


def engine_case(k, binding=None):
    """Case ``k`` on the device: ``(bounds, relaxed values, u, stats, infos, the device's G, the device's c)``."""
    from sparselm_amd import _engine

    with _engine.get_engine().dataset(k["X"], k["y"]) as ds:
        out = ds.solve_l0_local_bound(k["alphas"], k["etas"], big_M=k["big_M"], starts=k["starts"], max_sweeps=k["max_sweeps"],
                                      gap_tol=k["gap_tol"], binding=binding)
        G, c, _ = ds.covariance_download(0)
    return out + (G, c)


# ---- 1. the kernel equals the host twin -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases()))
def test_the_kernel_equals_the_twin(name):
    k = cases()[name]
    lower, primal, u, stats, infos, G, c = engine_case(k)
    ref = run_rule(G, c, k)  # the rule on the device's own Gram
    for e, run in enumerate(ref):
        alpha, eta = float(k["alphas"][e]), float(k["etas"][e])
        print(f"{name} cell {e}: alpha {alpha:.4g} eta {eta:.4g} M {k['big_M']}: rule sweeps {run['sweeps']} status {run['status']} changes "
              f"{run['changes']} lower {run['lower']:.15e} primal {run['primal']:.15e}; kernel sweeps {stats[e, 0]} status {stats[e, 1]} lower "
              f"{lower[e]:.15e} primal {primal[e]:.15e} max |u - u_rule| {np.max(np.abs(u[e] - run['u'])):.2e}")
        assert stats[e, 0] == run["sweeps"] and stats[e, 1] == run["status"]
        np.testing.assert_array_equal(u[e], run["u"])  # change for change: the same bits
        assert lower[e] == run["lower"] and primal[e] == run["primal"]
        # the certificate at the kernel's own u, by plain numpy products
        at_u = max(lower_bound(G, c, alpha, eta, k["big_M"], u[e]), lower_bound(G, c, alpha, eta, k["big_M"], np.zeros(len(c))))
        assert abs(lower[e] - at_u) <= certificate_tolerance(G, alpha, u[e], lower[e])
        assert np.all(np.abs(u[e]) <= k["big_M"]) and lower[e] <= primal[e] + certificate_tolerance(G, alpha, u[e], lower[e])
        assert infos[e]["lower_bound"] == lower[e] and infos[e]["relaxed_objective"] == primal[e] and infos[e]["sweeps"] == run["sweeps"]
        assert infos[e]["converged"] == (run["status"] == 0) and infos[e]["status"] == ("closed" if run["status"] == 0 else "sweep_cap")
    if name.startswith("rank_deficient"):
        assert G[7, 7] == 0.0 and c[7] == 0.0 and not u[:, 7].any()  # the zero column keeps u = 0; its term of the sum is counted (above)
    if name.startswith("p1024"):
        assert all(len({int(j) // 64 for j in np.flatnonzero(u[e])}) >= 8 for e in range(len(u))) and not stats[:, 1].any()


# ---- 2. the bound is a bound ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hard_bounds(seed, M, max_sweeps=500, warm=False):
    """``l0_local_bound`` on the hard law over alpha x eta at box ``M``: ``(the result, whether it warned, the ``L0LocalPath`` it
    started from or None)``.  Computed once."""
    from sparselm_amd.miqp import l0_local_bound, l0_local_search

    X, y, _, _ = hard_problem(seed)
    starts = l0_local_search(X, y, alphas=ALPHAS, etas=ETAS, big_M=M) if warm else None
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        res = l0_local_bound(X, y, alphas=ALPHAS, etas=ETAS, big_M=M, max_sweeps=max_sweeps, starts=starts)
    return res, any(issubclass(w.category, ConvergenceWarning) for w in seen), starts


def check_bounds(seed, M, res):
    for a, alpha in enumerate(ALPHAS):
        for e, eta in enumerate(ETAS):
            best = brute_force(seed, alpha, eta, M)
            print(f"seed {seed} M {M} alpha {alpha} eta {eta}: F* {best:.9e} bound {res.lower_bounds_[a, e]:.9e} relative gap "
                  f"{(best - res.lower_bounds_[a, e]) / max(abs(best), alpha):.3e} sweeps {res.sweeps_[a, e]} converged {res.converged_[a, e]}")
            assert res.lower_bounds_[a, e] <= best + SLACK * max(abs(best), alpha)  # no cell excluded


@pytest.mark.parametrize("M", BIG_MS)
@pytest.mark.parametrize("seed", range(3))
def test_the_bound_is_a_bound(seed, M):
    check_bounds(seed, M, hard_bounds(seed, M)[0])


@pytest.mark.parametrize("p", [1, 63, 64, 65, 130])
def test_the_gap_of_the_local_search_is_never_negative(p):
    from sparselm_amd.miqp import l0_local_bound, l0_local_search

    X, y = draw(80, p, 6, p)
    alphas, etas = np.array([0.01, 0.05, 0.3]) * float(np.var(y)), [0.0, 0.02, 0.5]
    for M in (100.0, 0.6):
        path = l0_local_search(X, y, alphas=alphas, etas=etas, big_M=M)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", ConvergenceWarning)
            bound = l0_local_bound(X, y, alphas=alphas, etas=etas, big_M=M, max_sweeps=300)
        gap = bound.gap(path)
        print(f"p {p} M {M}: gaps\n{gap}\nconverged\n{bound.converged_}")
        assert gap.shape == (3, 3) and np.all(gap >= -1e-9)


# ---- 3. the relaxation's optimum where converged ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M", BIG_MS)
@pytest.mark.parametrize("seed", range(3))
def test_a_converged_bound_is_the_relaxations_optimum(seed, M):
    res, warned, _ = hard_bounds(seed, M)
    _, _, G, c = hard_problem(seed)
    for a, alpha in enumerate(ALPHAS):
        for e, eta in enumerate(ETAS):
            if not res.converged_[a, e]:
                assert eta == 0.0 and M == 100.0  # at most these may be left open within 500 sweeps
                continue
            P, _, gap = fista(G, c, alpha, eta, M)
            assert gap <= 1e-10
            assert abs(res.lower_bounds_[a, e] - P) <= 1e-6 * max(abs(P), alpha), (alpha, eta)
            assert abs(res.relaxed_objectives_[a, e] - P) <= 1e-6 * max(abs(P), alpha)
    assert warned == (not res.converged_.all())


# ---- 4. early stop is still valid ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", BIG_MS)
@pytest.mark.parametrize("seed", range(3))
def test_one_sweep_is_still_a_bound(seed, M):
    """``max_sweeps = 1`` on the cells of test 2, all of them: the call says SLM_ERR_NOT_CONVERGED, Python warns, the values are bounds."""
    from sparselm_amd import _engine

    res, warned, _ = hard_bounds(seed, M, max_sweeps=1)
    assert warned and not res.converged_.all() and np.all(res.sweeps_ == 1)
    check_bounds(seed, M, res)
    X, y, _, _ = hard_problem(seed)
    with _engine.get_engine().dataset(X, y) as ds:
        lower, _, _, stats, infos = ds.solve_l0_local_bound(np.repeat(ALPHAS, 3), np.tile(ETAS, 3), big_M=M, max_sweeps=1)
    assert all(i["call_status"] == _engine.SLM_ERR_NOT_CONVERGED for i in infos) and not all(i["converged"] for i in infos)
    assert np.array_equal(lower.reshape(3, 3), res.lower_bounds_) and np.all(stats[:, 0] == 1) and stats[:, 1].any()


# ---- 5. warm start -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", BIG_MS)
def test_a_warm_start_from_the_local_search(M):
    cold, _, _ = hard_bounds(1, M)
    warm, _, path = hard_bounds(1, M, warm=True)
    _, _, G, c = hard_problem(1)
    check_bounds(1, M, warm)
    for a, alpha in enumerate(ALPHAS):
        for e, eta in enumerate(ETAS):
            assert warm.lower_bounds_[a, e] >= lower_bound(G, c, alpha, eta, M, np.zeros(10)) - SLACK * max(abs(cold.lower_bounds_[a, e]), alpha)
            if cold.converged_[a, e] and warm.converged_[a, e]:
                assert abs(warm.lower_bounds_[a, e] - cold.lower_bounds_[a, e]) <= 1e-6 * max(abs(cold.lower_bounds_[a, e]), alpha)
    assert np.all(warm.gap(path) >= -1e-9)


# ---- 6. the edge cells -----------------------------------------------------------------------------------------------------------------
def test_alpha_zero_is_the_box_ridge_optimum_and_a_zero_box_gives_zero():
    from sparselm_amd import _engine
    from sparselm_amd.miqp import l0_local_bound

    X, y, G, c = hard_problem(2)
    for M in BIG_MS:
        res = l0_local_bound(X, y, alphas=[0.0], etas=ETAS, big_M=M, gap_tol=1e-12, max_sweeps=5000)
        for e, eta in enumerate(ETAS):
            best = brute_force(2, 0.0, eta, M)  # alpha = 0: the minimum of the ridge problem inside the box
            print(f"alpha 0 eta {eta} M {M}: F* {best:.12e} bound {res.lower_bounds_[0, e]:.12e} sweeps {res.sweeps_[0, e]}")
            assert res.converged_[0, e] and abs(res.lower_bounds_[0, e] - best) <= 1e-9 * abs(best)
            assert res.lower_bounds_[0, e] <= best + SLACK * abs(best)
    res = l0_local_bound(X, y, alphas=ALPHAS, etas=ETAS, big_M=0.0, starts=np.ones(10))
    assert not res.lower_bounds_.any() and not res.relaxed_objectives_.any() and not res.relaxed_coefs_.any()
    assert res.converged_.all() and not res.sweeps_.any()
    with _engine.get_engine().dataset(X, y) as ds:
        lower, primal, u, stats, infos = ds.solve_l0_local_bound([0.1, 0.2], [0.0, 1.0], big_M=0.0)
        assert not lower.any() and not primal.any() and not u.any() and not stats.any() and all(i["converged"] for i in infos)
        assert ds.covariance_count() == 0  # no launch: not even the Gram the launch would read was built
    # eta = 0 under the loose box: a bound all the same (how far below the optimum: the documents have the figures)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        res = l0_local_bound(X, y, alphas=[0.5], etas=[0.0], big_M=100.0, max_sweeps=500)
    best = brute_force(2, 0.5, 0.0, 100.0)
    print(f"eta 0 M 100 alpha 0.5: F* {best:.9e} bound {res.lower_bounds_[0, 0]:.9e}")
    assert res.lower_bounds_[0, 0] <= best + SLACK * max(abs(best), 0.5)


# ---- 7. the surface -------------------------------------------------------------------------------------------------------------------
def test_an_intercept_and_sample_weights_reach_the_same_gram():
    """``fit_intercept`` and ``sample_weight`` go through ``_LocalProblem`` as they do for ``l0_local_search``: the bound is the
    certificate on numpy's weighted, centred Gram at the returned ``relaxed_coefs_``, in the units of the search's objectives."""
    from sparselm_amd.miqp import l0_local_bound, l0_local_search

    X, y = draw(60, 20, 4, 5)
    X = X + 3.0  # (column means far from zero: centring matters)
    w = np.random.default_rng(7).uniform(0.5, 2.0, 60)
    G, c, _, _, _ = gram(X, y, sample_weight=w, fit_intercept=True)
    alphas, etas = np.array([0.01, 0.1]) * float(np.var(y)), [0.0, 0.05]
    for M in (100.0, 0.6):
        path = l0_local_search(X, y, alphas=alphas, etas=etas, big_M=M, fit_intercept=True, sample_weight=w)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", ConvergenceWarning)
            bound = l0_local_bound(X, y, alphas=alphas, etas=etas, big_M=M, fit_intercept=True, sample_weight=w, max_sweeps=2000)
        for a, alpha in enumerate(alphas):
            for e, eta in enumerate(etas):
                u = bound.relaxed_coefs_[a, e]
                at_u = max(lower_bound(G, c, alpha, eta, M, u), lower_bound(G, c, alpha, eta, M, np.zeros(20)))
                F = objective(G, c, alpha, eta, path.coefs_[a, e])
                print(f"M {M} alpha {alpha:.4g} eta {eta}: bound {bound.lower_bounds_[a, e]:.12e} numpy {at_u:.12e}; search {path.objectives_[a, e]:.12e} "
                      f"numpy {F:.12e}; converged {bound.converged_[a, e]}")
                assert abs(bound.lower_bounds_[a, e] - at_u) <= certificate_tolerance(G, alpha, u, at_u)
                assert abs(path.objectives_[a, e] - F) <= 1e-9 * max(abs(F), alpha)  # the same G, c and units
        assert np.all(bound.gap(path) >= -1e-9)


def test_both_routes_bit_for_bit():
    from sparselm_amd import _engine

    if _engine.load_binding() is None:
        pytest.skip("the compiled binding is not built")
    k = cases()["slots65_start_outside_the_box"]
    a, b = engine_case(k, binding=False), engine_case(k, binding=True)
    for x, y_ in zip(a[:4], b[:4]):
        assert x.tobytes() == y_.tobytes()
    assert a[4] == b[4] and a[2].any()


@pytest.mark.parametrize("route", [False, True], ids=["ctypes", "binding"])
def test_the_import_and_every_refusal(route):
    from sparselm_amd import _engine
    from sparselm_amd.miqp import L0LocalBound, l0_local_bound  # noqa: F401

    if route and _engine.load_binding() is None:
        pytest.skip("the compiled binding is not built")  # (the ctypes leg runs all the same)
    k = cases()["slots65_start_outside_the_box"]
    X, y = k["X"], k["y"]
    wide = np.random.default_rng(0).standard_normal((8, 1025))
    with _engine.get_engine().dataset(wide, np.ones(8)) as ds:
        with pytest.raises(NotImplementedError, match="up to 1024 columns"):
            ds.solve_l0_local_bound([0.1], [0.1], binding=route)
        assert ds.covariance_count() == 0
    with _engine.get_engine().dataset(X, y) as ds:
        bad_start = np.zeros((1, 65))
        bad_start[0, 3] = np.nan
        for bad, words in ((dict(alphas=[0.1, -0.1], etas=[0.0, 0.0]), "alphas\\[1\\]"), (dict(alphas=[0.1], etas=[np.inf]), "etas\\[0\\]"),
                           (dict(alphas=[0.1], etas=[0.0], big_M=-1.0), "big_M"), (dict(alphas=[0.1], etas=[0.0], gap_tol=-1.0), "gap_tol"),
                           (dict(alphas=[0.1], etas=[0.0], n_cells=0), "n_cells must be >= 1"),
                           (dict(alphas=np.full(8193, 0.1), etas=0.0), "at most 8192 cells"),
                           (dict(alphas=[0.1], etas=[0.0], starts=bad_start), "starts\\[3\\] is not a finite number")):
            with pytest.raises(ValueError, match=words):
                ds.solve_l0_local_bound(binding=route, **bad)
        # the order: the cells before big_M, big_M before the alphas, the alphas before gap_tol
        with pytest.raises(ValueError, match="n_cells"):
            ds.solve_l0_local_bound([-1.0], [0.0], big_M=-1.0, gap_tol=-1.0, n_cells=0, binding=route)
        with pytest.raises(ValueError, match="big_M"):
            ds.solve_l0_local_bound([-1.0], [0.0], big_M=-1.0, gap_tol=-1.0, binding=route)
        with pytest.raises(ValueError, match="alphas"):
            ds.solve_l0_local_bound([-1.0], [0.0], gap_tol=-1.0, binding=route)
        assert ds.covariance_count() == 0  # every refusal came before a device was touched: no Gram was built
        ds.set_groups(np.arange(65) // 5, 13)
        with pytest.raises(NotImplementedError, match="groups"):
            ds.solve_l0_local_bound([0.1], [0.1], binding=route)
