"""The l0 local search with an l1 term on the GPU (``slm_solve_l0_local_l1``, ``l0_local_l1_kernel`` in csrc/l0_local_kernels.hpp)
against the numpy restatement of its rule (tests/_l1l0_local_reference.py; the problems: tests/_l1l0_local_cases.py), against the
penalised entry at lam = 0, and, where the columns fit, against ``L1L0`` on the same device.

The restatement reports the smallest relative margin by which it took any decision (a threshold ``gain > alpha``, ``|u|`` against
``lam``, a swap, the lead of an entering column; with several starts, the lead of the winning start's objective).  Every comparison
first asserts that this margin is >= 1e-6, so that rounding -- the kernel contracts multiply-adds and sums in another order --
cannot change a decision; no case is skipped.  Then: identical supports, swap counts and winning starts, objectives (after the
polish) to the family's 1e-10 relative, the polish not raising F, the box, and the certificate ``is_l1_swap_inescapable``."""

import warnings

import numpy as np
import pytest
from sklearn.exceptions import ConvergenceWarning

from _l0_local_reference import gram, hard_law
from _l1l0_local_cases import MARGIN_MIN, cases, reference, second_start_optimum, var
from _l1l0_local_reference import is_l1_swap_inescapable, solve_cells
from test_l0_local_gpu import draw

pytestmark = pytest.mark.gpu

OBJ_RTOL, CERT_TOL = 1e-10, 1e-8


def engine_cells(X, y, alphas, l1s, ridges, big_M=100.0, starts=None, swaps=True, binding=None):
    """One row set, the dataset's own rows: ``(betas [cells, p], objectives, winners, stats [cells, starts, 4], infos)``."""
    from sparselm_amd import _engine

    with _engine.get_engine().dataset(X, y) as ds:
        b, _, o, w, stats, infos = ds.solve_l0_local_l1([None], [0], alphas, l1s, ridges, big_M=big_M, starts=None if starts is None else starts[None],
                                                        swaps=swaps, binding=binding)
    return b[0], o[0], w[0], stats[0], infos[0]


def check_cells(ref, k, betas, objectives, winners, infos):
    for e, cell in enumerate(ref):
        alpha, lam, big_M = k["alphas"][e], k["l1s"][e], k["big_M"]
        print(f"cell {e}: alpha {alpha:.4g} lam {lam:.4g} ridge {k['ridges'][e]:.4g} margin {cell['margin']:.3e} lead {cell['lead']:.3e} "
              f"reference objective {cell['objective']:.12e} swaps {cell['swaps']} start {cell['start']} nnz {np.count_nonzero(cell['beta'])}; "
              f"engine objective {objectives[e]:.12e} swaps {infos[e]['swaps']} start {winners[e]} sweeps {infos[e]['sweeps']}")
        assert cell["status"] == 0 and cell["margin"] >= MARGIN_MIN and cell["lead"] >= MARGIN_MIN  # the premise
        assert infos[e]["converged"] and infos[e]["status"] == "fixed_point" and infos[e]["proven_optimal"] is False
        np.testing.assert_array_equal(betas[e] != 0.0, cell["beta"] != 0.0)
        assert infos[e]["swaps"] == cell["swaps"] and winners[e] == cell["start"]
        scale = max(abs(cell["objective"]), alpha, np.finfo(float).tiny)
        assert abs(objectives[e] - cell["objective"]) <= OBJ_RTOL * scale and objectives[e] == infos[e]["objective"]
        assert abs(infos[e]["descent_objective"] - cell["descent_objective"]) <= OBJ_RTOL * scale
        assert infos[e]["objective"] <= infos[e]["descent_objective"] + OBJ_RTOL * scale  # the polish does not raise it
        assert np.all(np.abs(betas[e]) <= big_M)
        ok, why = is_l1_swap_inescapable(cell["H"], cell["c"], alpha, lam, big_M, betas[e], CERT_TOL, swaps=k["swaps"])
        assert ok, why


def compare(name):
    """The comparison every case shares.  Returns (the restatement's cells, the engine's betas, objectives, infos)."""
    k, ref = cases()[name], reference(name)
    betas, objectives, winners, _, infos = engine_cells(k["X"], k["y"], k["alphas"], k["l1s"], k["ridges"], k["big_M"], k["starts"], k["swaps"])
    check_cells(ref, k, betas, objectives, winners, infos)
    return ref, betas, objectives, infos


# ---- 1. widths: one column, the slot boundary, several slots, all sixteen -----------------------------------------------------------
def test_one_column():
    _, betas, objectives, _ = compare("p1")
    assert betas[0][0] != 0.0 and betas[1][0] == 0.0 and objectives[1] == 0.0 and betas[2][0] != 0.0


@pytest.mark.parametrize("p", [63, 64, 65, 130])
def test_slot_boundaries(p):
    """63: one slot with an idle lane; 64: one full slot; 65: a second slot of one lane; 130: three slots, and one cell swaps."""
    ref, betas, _, infos = compare(f"slots{p}")
    if p == 130:
        assert sum(info["swaps"] for info in infos) >= 1
    assert not betas[2].any()  # (alpha = 0.3 var y keeps every column out)


@pytest.mark.parametrize("name", ["p1024_zero", "p1024_wrong_start"])
def test_every_slot_live_at_1024_columns(name):
    _, betas, _, _ = compare(name)
    live = np.flatnonzero(betas[0])
    assert set(live // 64) == set(range(16)) and live.size == 16  # every slot holds an active column


# ---- 2. the ends of the ranges --------------------------------------------------------------------------------------------------------
def test_no_ridge_with_fewer_rows_than_columns():
    compare("rows_below_columns")


def test_big_m_binds():
    _, betas, _, _ = compare("box")
    assert int(np.sum(np.abs(betas[0]) == 0.6)) == 4


def test_a_lam_above_max_c_empties_the_support():
    _, betas, objectives, _ = compare("lam_above_max_c")
    assert not betas.any() and not objectives.any()


def test_alpha_zero_is_a_lasso_fixed_point():
    """alpha = 0: the rule is the lasso's coordinate descent; the returned point satisfies the lasso's optimality conditions."""
    ref, betas, _, _ = compare("alpha_zero")
    k = cases()["alpha_zero"]
    for e, cell in enumerate(ref):
        g = cell["H"] @ betas[e] - cell["c"]
        lam = k["l1s"][e]
        on = betas[e] != 0.0
        assert on.any() and not on.all()
        assert np.max(np.abs(g[on] + lam * np.sign(betas[e][on]))) <= 1e-10 * lam
        assert np.all(np.abs(g[~on]) <= lam * (1.0 + 1e-10))


# ---- 3. starts, swaps, the problems of one launch -----------------------------------------------------------------------------------
def test_a_second_start_wins():
    exact, _ = second_start_optimum()
    ref, _, objectives, _ = compare("second_start")
    assert ref[0]["start"] == 1 and ref[0]["F"][1] < ref[0]["F"][0]
    assert abs(objectives[0] - exact) <= OBJ_RTOL * abs(exact)
    ref, _, _, _ = compare("second_start_reversed")  # the other order: the winner's index follows
    assert ref[0]["start"] == 0


def test_the_hard_law_with_swaps_and_without():
    ref_s, _, obj_s, infos = compare("hard_law_swaps")
    ref_d, _, obj_d, infos_d = compare("hard_law_descent")
    assert [i["swaps"] for i in infos] == [1, 1, 0] and not any(i["swaps"] for i in infos_d)
    assert obj_s[0] < obj_d[0] and obj_s[1] < obj_d[1] and obj_s[2] == obj_d[2]
    _, _, _, infos2 = compare("hard_law_two_swaps")
    assert [i["swaps"] for i in infos2] == [2, 2]


def test_more_problems_than_one_grid_pass():
    """2080 problems: with more problems than the grid has waves the grid-stride loop serves the rest.  Eight distinct cells
    repeated, so that the restatement runs eight times; the same cell gives the same bytes wherever it sits."""
    X, y = draw(30, 6, 3, 11)
    distinct = np.array([(0.001, 0.01), (0.003, 0.05), (0.01, 0.02), (0.03, 0.1), (0.1, 0.01), (0.3, 0.05), (3.0, 0.01), (0.0, 0.2)])
    al, l1 = distinct[:, 0] * var(y), distinct[:, 1].copy()
    ref = solve_cells(X, y, al, l1)
    assert all(cell["margin"] >= MARGIN_MIN and cell["status"] == 0 for cell in ref) and len({tuple(cell["beta"] != 0) for cell in ref}) >= 2
    cells = 2080
    idx = np.arange(cells) % 8
    betas, objectives, winners, stats, infos = engine_cells(X, y, al[idx], l1[idx], np.zeros(cells))
    assert betas.shape == (cells, 6) and not winners.any() and stats.shape == (cells, 1, 4)
    for e in range(cells):
        cell = ref[e % 8]
        assert np.array_equal(betas[e] != 0.0, cell["beta"] != 0.0) and infos[e]["swaps"] == cell["swaps"], e
        assert abs(objectives[e] - cell["objective"]) <= OBJ_RTOL * max(abs(cell["objective"]), al[e % 8]), e
        assert betas[e].tobytes() == betas[e % 8].tobytes(), e


def test_sixteen_weighted_row_sets_with_an_intercept():
    """16 row sets of one dataset [X | 1], each with its own weights, in one launch: against the restatement on each set's weighted,
    centred Gram, and against the single call per row set."""
    from sparselm_amd import _engine

    X, y = draw(50, 16, 4, 13)
    X, y = X + 3.0, y + 5.0
    rng = np.random.default_rng(2)
    weights = [rng.uniform(0.2, 2.0, 50) * (rng.uniform(size=50) > 0.15) for _ in range(16)]
    weights = [w * (50 / w.sum()) for w in weights]
    al, l1, rd = np.array([0.01, 0.1, 0.0]) * var(y), np.array([0.05, 0.02, 0.2]), np.array([0.0, 0.01, 0.0])
    Xd = np.hstack([X, np.ones((50, 1))])
    with _engine.get_engine().dataset(Xd, y) as ds:
        betas, icpts, objectives, winners, stats, infos = ds.solve_l0_local_l1(weights, [50] * 16, al, l1, rd, intercept=True)
        assert betas.shape == (16, 3, 16) and stats.shape == (16, 3, 1, 4)
        for r in (0, 7, 15):
            b1, i1, o1, _, s1, _ = ds.solve_l0_local_l1([weights[r]], [50], al, l1, rd, intercept=True)
            np.testing.assert_array_equal(b1[0] != 0.0, betas[r] != 0.0)
            np.testing.assert_array_equal(s1[0], stats[r])
            np.testing.assert_allclose(o1[0], objectives[r], rtol=OBJ_RTOL, atol=0)
            np.testing.assert_allclose(i1[0], icpts[r], rtol=1e-9, atol=0)
    k = dict(alphas=al, l1s=l1, ridges=rd, big_M=100.0, swaps=True)
    for r in range(16):
        ref = solve_cells(X, y, al, l1, rd, sample_weight=weights[r], fit_intercept=True)
        check_cells(ref, k, betas[r], objectives[r], winners[r], infos[r])
        _, _, _, x_mean, y_mean = gram(X, y, weights[r], True)
        for e in range(3):
            assert abs(icpts[r, e] - (y_mean - x_mean @ betas[r, e])) <= 1e-9 * abs(y_mean)
    assert len({tuple(map(tuple, betas[r] != 0.0)) for r in range(16)}) >= 2  # the row sets differ


# ---- 4. lam = 0 against the penalised entry; both routes; every refusal ---------------------------------------------------------------
def test_all_lam_zero_takes_the_decisions_of_the_penalised_entry():
    """Three starts per cell.  The same supports, swaps, sweeps and winners of EVERY problem, objectives to 1e-10 (not byte for byte:
    the multiply-adds may contract otherwise).  The premise is the penalised restatement's: no decision and no winner closer than
    1e-6 (a cell whose starts all end empty ties at exactly 0 on either side: the lowest start wins)."""
    import _l0_local_reference as plain

    from sparselm_amd import _engine

    rng = np.random.default_rng(4)
    swapped = 0
    for (X, y), rels in ((hard_law(5), (0.005, 0.01, 0.07, 0.1, 0.2)), (draw(80, 130, 6, 130), (0.05, 0.2, 0.3)),
                         (hard_law(12), (0.005, 0.01, 0.2, 0.3))):
        p, E = X.shape[1], len(rels)
        al, rd = np.array(rels) * var(y), np.zeros(E)
        starts = np.zeros((1, E, 3, p))
        starts[0, :, 1, :: max(p // 5, 1)] = 0.25
        starts[0, :, 2] = rng.uniform(-0.3, 0.3, p) * (rng.uniform(size=p) < 0.2)
        ref = plain.solve_cells(X, y, al, rd, starts=starts[0])
        for cell in ref:
            print(f"margin {cell['margin']:.3e} lead {cell['lead']:.3e} swaps {cell['swaps']} start {cell['start']}")
            assert cell["status"] == 0 and cell["margin"] >= MARGIN_MIN and cell["lead"] >= MARGIN_MIN  # the premise
        with _engine.get_engine().dataset(X, y) as ds:
            a = ds.solve_l0_local_folds([None], [0], al, rd, starts=starts)
            b = ds.solve_l0_local_l1([None], [0], al, np.zeros(E), rd, starts=starts)
        np.testing.assert_array_equal(a[0] != 0.0, b[0] != 0.0)
        np.testing.assert_array_equal(a[3], b[3])  # winners
        np.testing.assert_array_equal(a[3][0], [cell["start"] for cell in ref])
        np.testing.assert_array_equal(a[4], b[4])  # sweeps, swaps, status word, non-zeros of every problem
        np.testing.assert_allclose(a[2], b[2], rtol=OBJ_RTOL, atol=0)
        np.testing.assert_allclose(a[0], b[0], rtol=1e-9, atol=1e-12)
        swapped += int(a[4][..., 1].max() >= 1)
    assert swapped >= 2  # swaps in the compared problems


def test_both_routes_byte_for_byte_and_every_refusal():
    from sparselm_amd import _engine

    if _engine.load_binding() is None:
        pytest.fail("the compiled binding is not built")
    X, y = draw(60, 70, 5, 21)
    al, l1, rd = np.array([0.01, 0.05, 0.2]) * var(y), np.array([0.05, 0.1, 0.0]), np.array([0.0, 0.01, 0.0])
    starts = np.zeros((3, 2, 70))
    starts[:, 1, ::9] = 0.25
    a = engine_cells(X, y, al, l1, rd, starts=starts, binding=False)
    b = engine_cells(X, y, al, l1, rd, starts=starts, binding=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])
    assert np.array_equal(a[3], b[3]) and a[4] == b[4] and a[0].any()
    with _engine.get_engine().dataset(X, y) as ds:
        none = ds.solve_l0_local_l1([None], [0], al, l1, None)  # ridges = NULL: no ridge
        zero = ds.solve_l0_local_l1([None], [0], al, l1, 0.0, binding=True)
        assert none[0].tobytes() == zero[0].tobytes() and none[2].tobytes() == zero[2].tobytes()
    wide = np.random.default_rng(0).standard_normal((8, 1025))
    with _engine.get_engine().dataset(wide, np.ones(8)) as ds:
        for route in (False, True):
            with pytest.raises(NotImplementedError, match="up to 1024 columns"):
                ds.solve_l0_local_l1([None], [0], [0.1], [0.1], binding=route)
    w = np.ones(60)
    with _engine.get_engine().dataset(X, y) as ds:
        for route in (False, True):
            for bad, words in ((dict(alphas=[-1.0], l1s=[0.1]), "alphas"), (dict(alphas=[0.1], l1s=[-0.1]), "l1s"),
                               (dict(alphas=[0.1], l1s=[np.nan]), "l1s"), (dict(alphas=[0.1], l1s=[0.1], ridges=[np.inf]), "ridges"),
                               (dict(alphas=[0.1], l1s=[0.1], ridges=[-1.0]), "ridges"), (dict(alphas=[0.1], l1s=[0.1], big_M=-1.0), "big_M"),
                               (dict(alphas=[0.1], l1s=[0.1], n_cells=0), "n_cells"), (dict(alphas=[0.1], l1s=[0.1], n_starts=0), "n_starts"),
                               (dict(alphas=np.full(8193, 0.1), l1s=0.1), "problems"),
                               (dict(alphas=[0.1], l1s=[0.1], big_M=0.1, starts=starts[None, :1]), "box")):
                with pytest.raises(ValueError, match=words):
                    ds.solve_l0_local_l1([None], [0], binding=route, **bad)
            with pytest.raises(ValueError, match="count"):
                ds.solve_l0_local_l1([None] * 17, [0] * 17, [0.1], [0.1], binding=route)
            with pytest.raises(ValueError, match="row_weights"):
                ds.solve_l0_local_l1([-w], [0], [0.1], [0.1], binding=route)
        # the order: the l1 weights before the ridges, both before the row sets and the alphas
        for route in (False, True):
            with pytest.raises(ValueError, match="l1s"):
                ds.solve_l0_local_l1([None] * 17, [0] * 17, [-1.0], [-0.1], [-1.0], binding=route)
            with pytest.raises(ValueError, match="ridges"):
                ds.solve_l0_local_l1([None] * 17, [0] * 17, [-1.0], [0.1], [-1.0], binding=route)
            with pytest.raises(ValueError, match="count"):
                ds.solve_l0_local_l1([None] * 17, [0] * 17, [-1.0], [0.1], [0.0], binding=route)
            with pytest.raises(ValueError, match="alphas"):
                ds.solve_l0_local_l1([None], [0], [-1.0], [0.1], [0.0], binding=route)
        # (a NULL goes by ctypes alone: the compiled route takes arrays)
        with pytest.raises(ValueError, match="NULL"):
            ds.solve_l0_local_l1([None], [0], [0.1], None, binding=False)
        with pytest.raises(ValueError, match="NULL"):
            ds.solve_l0_local_l1([None], [0], None, [0.1], binding=False)
        ds.set_groups(np.arange(70) // 2, 35)
        for route in (False, True):
            with pytest.raises(NotImplementedError, match="groups"):
                ds.solve_l0_local_l1([None], [0], [0.1], [0.1], binding=route)


# ---- 5. against the exact search on the same device ---------------------------------------------------------------------------------
def exact_fit(X, y, alpha, eta):
    from sparselm_amd.miqp import L1L0

    est = L1L0(alpha=alpha, eta=eta, big_M=100)
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        est.fit(X, y)
    assert est.solver_info_["proven_optimal"]
    return est.solver_info_["objective"]


def test_never_below_l1l0_and_equal_on_easy_cases():
    from sparselm_amd.miqp import l1l0_local_search

    hits = 0
    for seed in (0, 1):
        X, y = hard_law(seed, p=20)
        alphas, etas = np.array([0.02, 0.1]) * var(y), [0.02, 0.1]
        path = l1l0_local_search(X, y, alphas=alphas, etas=etas)
        assert path.proven_optimal_ is False and path.converged_.all() and path.ridge_ == 0.0
        for a in range(2):
            for e in range(2):
                exact = exact_fit(X, y, alphas[a], etas[e])
                print(f"seed {seed} alpha {alphas[a]:.4g} eta {etas[e]}: local {path.objectives_[a, e]:.12e} exact {exact:.12e}")
                assert path.objectives_[a, e] >= exact - OBJ_RTOL * abs(exact)
                hits += abs(path.objectives_[a, e] - exact) <= OBJ_RTOL * abs(exact)
    print(f"{hits} of 8 hard cells at the proven optimum")
    # easy: AR(1) 0.1, signal-to-noise 20 -- the local minimum is the optimum
    for seed in (0, 1):
        X, y = hard_law(seed, n=60, p=12, rho=0.1, k=3, snr=20.0)
        alphas, etas = np.array([0.02, 0.1]) * var(y), [0.02, 0.1]
        path = l1l0_local_search(X, y, alphas=alphas, etas=etas, fit_intercept=True)
        for a in range(2):
            for e in range(2):
                exact = exact_fit_intercept(X, y, alphas[a], etas[e])
                assert abs(path.objectives_[a, e] - exact["objective"]) <= OBJ_RTOL * abs(exact["objective"]), (seed, a, e)
                np.testing.assert_array_equal(path.supports_[a, e], exact["coef"] != 0.0)
                np.testing.assert_allclose(path.coefs_[a, e], exact["coef"], rtol=0, atol=1e-7 * np.abs(exact["coef"]).max())
                assert abs(path.intercepts_[a, e] - exact["intercept"]) <= 1e-7 * max(abs(exact["intercept"]), 1.0)


def exact_fit_intercept(X, y, alpha, eta):
    from sparselm_amd.miqp import L1L0

    est = L1L0(alpha=alpha, eta=eta, big_M=100, fit_intercept=True).fit(X, y)
    assert est.solver_info_["proven_optimal"]
    return {"objective": est.solver_info_["objective"], "coef": est.coef_, "intercept": est.intercept_}


# ---- 6. rounds, swaps = False, cross-validation --------------------------------------------------------------------------------------
def test_rounds_never_raise_an_objective():
    from sparselm_amd.miqp import l1l0_local_search

    X, y = hard_law(4, p=20)
    alphas = np.geomspace(0.005, 0.3, 6) * var(y)
    etas = [0.0, 0.02, 0.1]
    one = l1l0_local_search(X, y, alphas=alphas, etas=etas, max_rounds=0)
    path = l1l0_local_search(X, y, alphas=alphas, etas=etas, ridge=0.0, max_rounds=3)
    print("rounds", path.rounds_, "\n", path.round_objectives_)
    assert one.rounds_ == 1 and 2 <= path.rounds_ <= 4 and path.round_objectives_.shape == (path.rounds_, 6, 3)
    np.testing.assert_array_equal(path.round_objectives_[0], one.objectives_)
    np.testing.assert_array_equal(path.round_objectives_[-1], path.objectives_)
    assert np.all(np.diff(path.round_objectives_, axis=0) <= 0.0)
    G, c, _, _, _ = gram(X, y)
    for a in range(6):
        for e in range(3):
            ok, why = is_l1_swap_inescapable(G, c, alphas[a], etas[e], 100.0, path.coefs_[a, e], CERT_TOL)
            assert ok, (a, e, why)
    descent = l1l0_local_search(X, y, alphas=alphas, etas=etas, max_rounds=0, solver_options={"swaps": False})
    assert not descent.swaps_.any() and one.swaps_.any() and np.all(one.objectives_ <= descent.objectives_ + 1e-12)
    ridged = l1l0_local_search(X, y, alphas=alphas[:2], etas=[0.02], ridge=0.05, max_rounds=0)
    assert ridged.ridge_ == 0.05 and not np.array_equal(ridged.coefs_, one.coefs_[:2, 1:2])


def test_l1l0_local_cv_end_to_end():
    from sklearn.model_selection import KFold

    from sparselm_amd.miqp import l1l0_local_cv, l1l0_local_search

    X, y = draw(60, 24, 4, 31)
    X, y = X + 1.0, y + 2.0
    alphas, etas = np.array([0.005, 0.05, 0.5]) * var(y), [0.01, 0.1]
    cv = KFold(4, shuffle=True, random_state=0)
    rounds = l1l0_local_cv(X, y, alphas=alphas, etas=etas, cv=cv, fit_intercept=True, max_rounds=1)
    assert rounds.solver_info_["launches"] == rounds.solver_info_["rounds"] == 2  # 1 + rounds launches, whatever the fold count
    assert np.all(np.diff(rounds.full_.round_objectives_, axis=0) <= 0.0) and rounds.solver_info_["problems"] == 5 * 6 * 4
    res = l1l0_local_cv(X, y, alphas=alphas, etas=etas, cv=cv, fit_intercept=True, max_rounds=0)
    assert res.proven_optimal_ is False and res.solver_info_["launches"] == 1 and res.solver_info_["problems"] == 5 * 6
    assert res.cell_scores_.shape == (4, 3, 2)
    for f, (tr, te) in enumerate(res.splits_):
        single = l1l0_local_search(X[tr], y[tr], alphas=alphas, etas=etas, fit_intercept=True, max_rounds=0)
        np.testing.assert_array_equal(res.paths_[f].supports_, single.supports_)
        np.testing.assert_allclose(res.paths_[f].objectives_, single.objectives_, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(res.paths_[f].coefs_, single.coefs_, rtol=0, atol=1e-8)
        rmse = np.sqrt(np.mean((y[te] - res.paths_[f].predict(X[te], 1, 0)) ** 2))
        assert abs(res.cell_scores_[f, 1, 0] + rmse) <= 1e-12
    full = l1l0_local_search(X, y, alphas=alphas, etas=etas, fit_intercept=True, max_rounds=0)
    np.testing.assert_array_equal(res.full_.supports_, full.supports_)
    for rule in ("max_score", "one_std_score"):
        found = res.search(rule)
        assert [set(q) for q in found.cv_results_["params"]] == [{"alpha", "eta"}] * 6
        a, e = divmod(found.best_index_, 2)
        np.testing.assert_array_equal(found.coef_, res.full_.coefs_[a, e])
        assert found.best_params_ == {"alpha": float(alphas[a]), "eta": float(etas[e])}
