"""The l0 local search with groups and a hierarchy on the GPU (``slm_solve_l0_local_groups``, csrc/l0_local_group_kernels.hpp)
against the numpy restatement of its rule (tests/_l0_local_groups_reference.py) and, where the columns fit, against the exact
estimators with the same ``groups`` and ``hierarchy`` on the same device.

As in tests/test_l0_local_gpu.py every comparison first asserts the PREMISE: the restatement took every decision (screen, keep or
drop, candidate lead, swap; with several starts the winner's lead) with a relative margin >= 1e-6, so that rounding -- the kernel
contracts multiply-adds -- cannot change one.  Then: identical group supports (cl(S)), column supports, swap counts and winning
starts, objectives (after the polish) to 1e-10 relative, and the independent certificate ``is_group_swap_inescapable`` on the
engine's coefficients.  Rows stay at n <= 200."""

import functools
import warnings

import numpy as np
import pytest

from _l0_local_groups_reference import close_hierarchy, group_law, is_group_swap_inescapable, solve_group_cells

pytestmark = pytest.mark.gpu

MARGIN_MIN, OBJ_RTOL, CERT_TOL = 1e-6, 1e-10, 1e-8


def thirds(p):
    """Groups of three consecutive columns (the last one holds what is left): at p >= 65 group 21 straddles columns 63 | 64."""
    return np.append(np.arange(0, p, 3), p)


@functools.lru_cache(maxsize=None)
def draw(n, p, seed, rho=0.5, noise=0.5):
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, p))
    X = Z.copy()
    for j in range(1, p):
        X[:, j] = rho * X[:, j - 1] + np.sqrt(1.0 - rho * rho) * Z[:, j]
    e = noise * rng.standard_normal(n)
    X.setflags(write=False)
    e.setflags(write=False)
    return X, e


def signal(X, e, gstart, true_groups):
    """y = the columns of ``true_groups`` with coefficients +-1, plus the noise."""
    beta = np.zeros(X.shape[1])
    for t, g in enumerate(true_groups):
        beta[gstart[g]:gstart[g + 1]] = (-1.0) ** (t + np.arange(gstart[g + 1] - gstart[g]))
    return X @ beta + e


def gid_of(gstart):
    return np.repeat(np.arange(len(gstart) - 1), np.diff(gstart)).astype(np.int32)


def engine_cells(X, y, gstart, need, alphas, etas, big_M=100.0, starts=None, swaps=True, sample_weight=None, fit_intercept=False,
                 binding=None, singleton=False):
    """One row set, the dataset's own rows (centred on the rows with an intercept, as ``l0_local_group_search`` does it)."""
    from sparselm_amd import _engine

    n = X.shape[0]
    w = None if sample_weight is None else np.asarray(sample_weight) * (n / np.sum(sample_weight))
    with _engine.get_engine().dataset(X, y, row_weight=w) as ds:
        if fit_intercept:
            ds.center()
        if not singleton:
            ds.set_groups(gid_of(gstart), len(gstart) - 1)
        b, _, o, wn, gs, stats, infos = ds.solve_l0_local_groups([None], [0], alphas, etas, need=need, big_M=big_M,
                                                                 starts=None if starts is None else np.asarray(starts)[None], swaps=swaps,
                                                                 binding=binding)
    return b[0], o[0], wn[0], gs[0], stats[0], infos[0]


def check_cells(ref, out, alphas, gstart, need, big_M=100.0, swaps=True):
    betas, objectives, winners, gsup, stats, infos = out
    closed = close_hierarchy(len(gstart) - 1, need)
    for e, cell in enumerate(ref):
        print(f"cell {e}: alpha {alphas[e]:.4g} margin {cell['margin']:.3e} lead {cell['lead']:.3e} reference objective {cell['objective']:.12e} "
              f"swaps {cell['swaps']} sweeps {cell['sweeps']} trials {cell['trials']} start {cell['start']} groups {int(cell['closed'].sum())}; "
              f"engine objective {objectives[e]:.12e} swaps {infos[e]['swaps']} sweeps {infos[e]['sweeps']} trials {infos[e]['trials']} "
              f"start {winners[e]} groups {infos[e]['n_active_groups']}")
        assert cell["status"] == 0 and cell["margin"] >= MARGIN_MIN and cell["lead"] >= MARGIN_MIN  # the premise
        assert infos[e]["converged"] and infos[e]["status"] == "fixed_point" and infos[e]["proven_optimal"] is False
        np.testing.assert_array_equal(gsup[e].astype(bool), cell["closed"])
        np.testing.assert_array_equal(betas[e] != 0.0, cell["beta"] != 0.0)
        assert infos[e]["swaps"] == cell["swaps"] and winners[e] == cell["start"] and infos[e]["trials"] == cell["trials"]
        assert stats[e, winners[e], 3] == int(cell["closed"].sum()) == infos[e]["n_active_groups"]
        scale = max(abs(cell["objective"]), alphas[e], np.finfo(float).tiny)
        assert abs(objectives[e] - cell["objective"]) <= OBJ_RTOL * scale and objectives[e] == infos[e]["objective"]
        assert infos[e]["objective"] <= infos[e]["descent_objective"] + OBJ_RTOL * scale  # the polish does not raise it
        assert np.all(np.abs(betas[e]) <= big_M)
        ok, why = is_group_swap_inescapable(cell["H"], cell["c"], alphas[e], big_M, betas[e], gstart, closed, CERT_TOL, swaps=swaps)
        assert ok, why


def compare(X, y, gstart, need, alphas, etas=None, big_M=100.0, starts=None, swaps=True, sample_weight=None, fit_intercept=False):
    alphas = np.asarray(alphas, dtype=float)
    etas = np.zeros_like(alphas) if etas is None else np.asarray(etas, dtype=float)
    ref = solve_group_cells(X, y, gstart, need, alphas, etas, big_M=big_M, starts=starts, swaps=swaps, sample_weight=sample_weight,
                            fit_intercept=fit_intercept)
    out = engine_cells(X, y, gstart, need, alphas, etas, big_M, starts, swaps, sample_weight, fit_intercept)
    check_cells(ref, out, alphas, gstart, need, big_M, swaps)
    return ref, out


def var(y):
    return float(np.var(y))


# ---- 1. singleton groups, no hierarchy: the family's search -------------------------------------------------------------------------
def test_singleton_groups_are_the_local_search():
    """p = 65, three cells: the supports, swap counts and SWEEPS of ``solve_l0_local_folds``, objectives to 1e-10."""
    from sparselm_amd import _engine

    X, e = draw(80, 65, 65)
    gstart = np.arange(66)
    y = signal(X, e, gstart, [3, 20, 41, 63, 64])
    alphas, etas = np.array([0.01, 0.05, 0.3]) * var(y), np.array([0.0, 0.02, 0.0])
    ref, (betas, objectives, _, gsup, _, infos) = compare(X, y, gstart, None, alphas, etas)
    with _engine.get_engine().dataset(X, y) as ds:
        b0, _, o0, _, _, i0 = ds.solve_l0_local_folds([None], [0], alphas, etas)
        b1, _, o1, _, g1, _, i1 = ds.solve_l0_local_groups([None], [0], alphas, etas)  # the dataset's own singleton groups
    for e_ in range(3):
        for b, o, info in ((betas, objectives, infos), (b1[0], o1[0], i1[0])):
            np.testing.assert_array_equal(b[e_] != 0.0, b0[0][e_] != 0.0)
            assert (info[e_]["swaps"], info[e_]["sweeps"]) == (i0[0][e_]["swaps"], i0[0][e_]["sweeps"])
            assert abs(o[e_] - o0[0][e_]) <= OBJ_RTOL * max(abs(o0[0][e_]), alphas[e_])
        np.testing.assert_array_equal(g1[0][e_].astype(bool), b0[0][e_] != 0.0)


# ---- 2. - 4. group shapes against the slots --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [63, 64, 65, 130])
def test_groups_of_three_across_the_slot_boundary(p):
    """63: one slot with an idle lane; 64: a last group of one column; 65 and 130: group 21 holds columns 63, 64 and 65, in two
    slots, and carries signal."""
    X, e = draw(80, p, p)
    gstart = thirds(p)
    ng = len(gstart) - 1
    y = signal(X, e, gstart, [2, min(21, ng - 1), ng // 2])
    compare(X, y, gstart, None, np.array([0.01, 0.05, 0.5]) * var(y), etas=[0.0, 0.02, 0.0])


def test_one_group_holds_all_65_columns():
    X, e = draw(120, 65, 7, rho=0.3)
    gstart = np.array([0, 65])
    y = signal(X, e, gstart, [0])
    ref, (betas, _, _, gsup, _, _) = compare(X, y, gstart, None, np.array([0.05, 50.0]) * var(y), etas=[0.01, 0.01])
    assert gsup[0][0] == 1 and np.count_nonzero(betas[0]) == 65 and gsup[1][0] == 0 and not betas[1].any()


def test_a_group_of_one_column_last():
    X, e = draw(80, 64, 64)
    gstart = thirds(64)
    assert gstart[-1] - gstart[-2] == 1
    y = 2.0 * X[:, 63] + 0.2 * e
    ref, (betas, _, _, gsup, _, _) = compare(X, y, gstart, None, [0.05 * var(y)])
    assert betas[0][63] != 0.0 and gsup[0][-1] == 1 and gsup[0].sum() == 1


# ---- 5. every slot live at 1024 columns ------------------------------------------------------------------------------------------------
def test_every_slot_live_at_1024_columns():
    """p = 1024 as 256 groups of four, n = 200: one true group in each slot of 64 columns, from zero and from a wrong start."""
    X, e = draw(200, 1024, 3, rho=0.0, noise=0.3)
    gstart = np.arange(0, 1025, 4)
    true = [16 * s + (5 * s + 3) % 16 for s in range(16)]
    y = signal(X, e, gstart, true)
    start = np.zeros((1, 1, 1024))
    start[0, 0, 8::64] = 0.5  # sixteen wrong columns, one per slot, in sixteen wrong groups
    # (two calls, not two starts of one: both reach the same support, and a tie in F to the last bit names no winner)
    for starts in (None, start):
        ref, (betas, _, _, gsup, _, _) = compare(X, y, gstart, None, [0.01 * var(y)], starts=starts)
        assert sorted(np.flatnonzero(gsup[0])) == sorted(true) and np.count_nonzero(betas[0]) == 64


# ---- 6. hierarchies -----------------------------------------------------------------------------------------------------------------
def test_a_chain_pays_for_its_closure_or_stays_out():
    """Five groups of two under a chain, the signal in the deepest alone: at a small alpha it enters and pays for all five; at an
    alpha between a fifth of its value and its value it stays out, where it would have entered without the hierarchy."""
    X, e = draw(100, 10, 21, rho=0.2)
    gstart = np.arange(0, 11, 2)
    chain = [[]] + [[g - 1] for g in range(1, 5)]
    y = signal(X, e, gstart, [4])
    alphas = np.array([0.02, 0.4]) * var(y)
    ref, (_, _, _, gsup, _, _) = compare(X, y, gstart, chain, alphas)
    assert gsup[0].all() and not gsup[1].any()
    _, (_, _, _, free, _, _) = compare(X, y, gstart, None, alphas)
    assert list(free[1]) == [0, 0, 0, 0, 1]


def test_a_diamond_a_cycle_and_a_start_that_is_not_closed():
    X, e = draw(100, 12, 22, rho=0.3)
    gstart = np.arange(0, 13, 2)                          # six groups of two
    diamond = [[], [0], [0], [1, 2], [], []]              # 3 needs 1 and 2, which both need 0
    y = signal(X, e, gstart, [3, 5])
    ref, (_, _, _, gsup, _, _) = compare(X, y, gstart, diamond, np.array([0.01, 0.1, 0.6]) * var(y))
    assert list(gsup[0][:4]) == [1, 1, 1, 1] and gsup[0][5] == 1
    cycle = [[1], [0], [], [], [], []]                    # 0 and 1 need each other: either brings both
    y2 = signal(X, e, gstart, [0, 4])
    ref, (_, _, _, gsup, _, _) = compare(X, y2, gstart, cycle, np.array([0.01, 0.1]) * var(y2))
    assert gsup[0][0] == gsup[0][1] == 1 and gsup[0][4] == 1
    # a start on group 3 alone under the diamond: F counts its closure from the first sweep on
    start = np.zeros((3, 1, 12))
    start[:, 0, 6:8] = 0.7
    compare(X, y, gstart, diamond, np.array([0.01, 0.1, 0.6]) * var(y), starts=start)


# ---- 7. against the exact estimators ----------------------------------------------------------------------------------------------------
def test_never_below_the_proven_optimum_and_equal_on_the_easy_cases():
    from sparselm_amd.miqp import L2L0, RegularizedL0, l0_local_group_search

    chain7 = [[]] + [[g - 1] for g in range(1, 7)]
    for seed in (0, 1, 2):  # the easy law of tests/test_l0_local_groups_cpu.py: the local search reaches the optimum there
        X, y, gstart = group_law(seed, rho=0.1, snr=20.0, spread=False)
        groups = gid_of(gstart)
        for hierarchy in (None, chain7):
            alphas = np.array([0.02, 0.1]) * var(y)
            path = l0_local_group_search(X, y, alphas=alphas, groups=groups, hierarchy=hierarchy)
            for a, alpha in enumerate(alphas):
                exact = RegularizedL0(groups=groups, alpha=alpha, hierarchy=hierarchy).fit(X, y)
                best = exact.solver_info_["objective"]
                assert exact.solver_info_["proven_optimal"]
                print(f"easy seed {seed} chain {hierarchy is not None} alpha {alpha:.4g}: local {path.objectives_[a, 0]:.12e} exact {best:.12e}")
                assert abs(path.objectives_[a, 0] - best) <= 1e-9 * max(abs(best), alpha)
                np.testing.assert_array_equal(path.group_supports_[a, 0], exact.active_groups_)
    chain10 = [[]] + [[g - 1] for g in range(1, 10)]
    for seed in (0, 1):  # the hard law at p = 20: never below
        X, y, gstart = group_law(seed, n_groups=10, k=3)
        groups = gid_of(gstart)
        for hierarchy in (None, chain10):
            alphas = np.array([0.02, 0.1]) * var(y)
            path = l0_local_group_search(X, y, alphas=alphas, etas=[0.0, 0.05], groups=groups, hierarchy=hierarchy)
            for a, alpha in enumerate(alphas):
                for e, eta in enumerate((0.0, 0.05)):
                    est = RegularizedL0(groups=groups, alpha=alpha, hierarchy=hierarchy) if eta == 0.0 else \
                        L2L0(groups=groups, alpha=alpha, eta=eta, hierarchy=hierarchy)
                    best = est.fit(X, y).solver_info_["objective"]
                    print(f"hard seed {seed} chain {hierarchy is not None} alpha {alpha:.4g} eta {eta}: local {path.objectives_[a, e]:.12e} "
                          f"exact {best:.12e}")
                    assert est.solver_info_["proven_optimal"] and path.objectives_[a, e] >= best - 1e-9 * max(abs(best), alpha)


# ---- 8. row sets --------------------------------------------------------------------------------------------------------------------
def test_three_folds_and_all_rows_with_an_intercept_and_weights():
    """Each row set of ONE call equals the single call on its rows (and the restatement on them)."""
    from sparselm_amd import _engine

    n, p = 90, 12
    X, e = draw(n, p, 31, rho=0.3)
    X = X + 1.5  # (off the origin: the intercept matters)
    gstart = np.arange(0, 13, 3)
    need = [[], [0], [], [2]]
    y = signal(X, e, gstart, [1, 2]) + 2.0
    w = np.random.default_rng(4).uniform(0.5, 1.5, n)
    folds = np.arange(n) % 3
    sets = [np.flatnonzero(folds != f) for f in range(3)] + [np.arange(n)]
    alphas = np.array([0.01, 0.1]) * var(y)
    row_weights, n_effs = [], []
    for rows in sets:
        m = np.zeros(n)
        m[rows] = w[rows] * (len(rows) / w[rows].sum())
        row_weights.append(m)
        n_effs.append(len(rows))
    gid = np.append(gid_of(gstart), 4).astype(np.int32)
    with _engine.get_engine().dataset(np.hstack([X, np.ones((n, 1))]), y) as ds:
        ds.set_groups(gid, 5)
        b, icpt, o, wn, gs, stats, infos = ds.solve_l0_local_groups(row_weights, n_effs, alphas, 0.0, need=need, intercept=True)
    assert b.shape == (4, 2, 12) and gs.shape == (4, 2, 4) and stats.shape == (4, 2, 1, 6)
    for r, rows in enumerate(sets):
        ref = solve_group_cells(X[rows], y[rows], gstart, need, alphas, np.zeros(2), sample_weight=w[rows], fit_intercept=True)
        check_cells(ref, (b[r], o[r], wn[r], gs[r], stats[r], infos[r]), alphas, gstart, need)
        single = engine_cells(X[rows], y[rows], gstart, need, alphas, np.zeros(2), sample_weight=w[rows], fit_intercept=True)
        for e_ in range(2):
            np.testing.assert_array_equal(single[3][e_], gs[r][e_])
            assert single[5][e_]["swaps"] == infos[r][e_]["swaps"]
            assert abs(single[1][e_] - o[r][e_]) <= OBJ_RTOL * max(abs(o[r][e_]), alphas[e_])
            wr = w[rows] / w[rows].sum()
            assert abs(icpt[r][e_] - (wr @ y[rows] - (wr @ X[rows]) @ b[r][e_])) <= 1e-9 * max(1.0, abs(icpt[r][e_]))


# ---- 9. more problems than one grid pass ------------------------------------------------------------------------------------------------
def test_more_problems_than_one_grid_pass():
    """More than 2 x CUs x 4 problems, alternating two cells with different supports under a chain: the grid-stride loop serves the
    rest, and a wave's LDS tables are set up again for every problem it takes."""
    from sparselm_amd import _engine

    X, e = draw(40, 6, 11, rho=0.2)
    gstart = np.array([0, 2, 4, 6])
    chain = [[], [0], [1]]
    y = signal(X, e, gstart, [2])
    cus = int(_engine.get_engine().device_info()["compute_units"])
    cells = min(2 * cus * 4 + 9, 8192)
    assert cells > 2 * cus * 4 or cus >= 1024
    two = np.array([0.01, 0.6]) * var(y)
    ref = solve_group_cells(X, y, gstart, chain, two, np.zeros(2))
    assert all(cell["margin"] >= MARGIN_MIN for cell in ref) and ref[0]["closed"].all() and not ref[1]["closed"].any()
    alphas = two[np.arange(cells) % 2]
    betas, objectives, winners, gsup, stats, infos = engine_cells(X, y, gstart, chain, alphas, np.zeros(cells))
    assert betas.shape == (cells, 6) and not winners.any()
    for c_ in range(cells):
        cell = ref[c_ % 2]
        assert np.array_equal(gsup[c_].astype(bool), cell["closed"]) and infos[c_]["swaps"] == cell["swaps"], c_
        assert abs(objectives[c_] - cell["objective"]) <= OBJ_RTOL * max(abs(cell["objective"]), alphas[c_]), c_


# ---- 10. the descent alone ----------------------------------------------------------------------------------------------------------
def test_with_and_without_the_swap_scan():
    """The hard law (7 groups of 2, AR(1) 0.9) on seeds where the scan accepts a swap: without a hierarchy, and under one that
    mixes a diamond and two chains."""
    mixed = [[], [0], [0], [1, 2], [], [4], [1]]
    for seed, k, need in ((2, 2, None), (34, 3, mixed)):
        X, y, gstart = group_law(seed, k=k)
        alphas = np.array([0.02, 0.05, 0.1]) * var(y)
        ref, (_, _, _, _, _, infos) = compare(X, y, gstart, need, alphas, swaps=False)
        assert all(info["swaps"] == 0 for info in infos)
        ref, (_, objectives, _, _, _, infos) = compare(X, y, gstart, need, alphas, swaps=True)
        assert sum(info["swaps"] for info in infos) >= 1  # (the comparison has checked the counts cell by cell)


# ---- 11. the engine's refusals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binding", [None, False])
def test_the_engine_refuses_in_its_own_words(binding):
    from sparselm_amd import _engine

    X, e = draw(20, 6, 1)
    y = X[:, 0] + e
    with _engine.get_engine().dataset(X, y) as ds:
        ds.set_groups(np.array([0, 1, 0, 1, 2, 2], dtype=np.int32), 3)
        with pytest.raises(NotImplementedError, match="the caller must order the columns"):
            ds.solve_l0_local_groups([None], [0], [0.1], binding=binding)
        ds.set_groups(np.array([0, 0, 1, 1, 2, 2], dtype=np.int32), 3)
        with pytest.raises(ValueError, match="need_idx\\[1\\] must name one of the 3 search groups"):
            ds.solve_l0_local_groups([None], [0], [0.1], need=[[], [0, 3], []], binding=binding)
        with pytest.raises(ValueError, match="need_ptr must start at 0 and never fall"):
            ds.solve_l0_local_groups([None], [0], [0.1], need=(np.array([0, 2, 1, 2]), np.array([0, 1])), binding=binding)
        with pytest.raises(ValueError, match="alphas\\[0\\] must be finite and >= 0"):
            ds.solve_l0_local_groups([None], [0], [-0.1], binding=binding)
        for name in ("solve_l0_local_folds", "solve_l0_local_subsets"):  # the family keeps its refusal
            with pytest.raises(NotImplementedError, match="groups"):
                getattr(ds, name)([None], [0], [1], binding=binding)
    with _engine.get_engine().dataset(np.zeros((4, 1025)), np.zeros(4)) as ds:
        with pytest.raises(NotImplementedError, match="takes up to 1024 columns"):
            ds.solve_l0_local_groups([None], [0], [0.1], binding=binding)


# ---- 12. - 13. the Python entries ---------------------------------------------------------------------------------------------------
def test_shuffled_labels_equal_the_call_on_sorted_columns():
    from sparselm_amd.miqp import l0_local_group_search

    X, y, gstart = group_law(2, n=60)
    groups = gid_of(gstart)
    hierarchy = [[]] + [[g - 1] for g in range(1, 7)]
    order = np.random.default_rng(9).permutation(14)
    alphas, etas = np.array([0.02, 0.05, 0.1]) * var(y), [0.0, 0.02]
    starts = np.zeros((1, 14))
    starts[0, 12:] = 0.3
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        plain = l0_local_group_search(X, y, alphas=alphas, etas=etas, groups=groups, hierarchy=hierarchy, fit_intercept=True, starts=starts)
        mixed = l0_local_group_search(X[:, order], y, alphas=alphas, etas=etas, groups=groups[order], hierarchy=hierarchy, fit_intercept=True,
                                      starts=starts[:, order])
    assert plain.coefs_.shape == (3, 2, 14) and plain.group_supports_.shape == (3, 2, 7) and plain.proven_optimal_ is False
    # (the same problem with the columns of a group in another order: the Gram's sums and the polish's factor round differently,
    # so supports are identical and the numbers agree to the family's 1e-10 on objectives; the coefficients of this law, AR(1) 0.9
    # with a condition number of a few hundred, to 1e-9)
    np.testing.assert_array_equal(mixed.coefs_ != 0.0, plain.coefs_[..., order] != 0.0)
    np.testing.assert_allclose(mixed.coefs_, plain.coefs_[..., order], rtol=1e-9, atol=1e-12)
    np.testing.assert_array_equal(mixed.group_supports_, plain.group_supports_)
    np.testing.assert_allclose(mixed.objectives_, plain.objectives_, rtol=OBJ_RTOL, atol=0.0)
    np.testing.assert_array_equal(mixed.swaps_, plain.swaps_)
    np.testing.assert_array_equal(plain.n_active_groups_, plain.group_supports_.sum(axis=-1))
    assert np.all(np.diff(plain.round_objectives_, axis=0) <= 0.0) and plain.trials_.shape == (3, 2)
    # the supports are closed under the chain, and the objective is the one the exact estimators report
    assert np.all(plain.group_supports_[..., :-1] >= plain.group_supports_[..., 1:])
    Xc, yc = X - X.mean(axis=0), y - y.mean()
    for a in range(3):
        for e in range(2):
            b = plain.coefs_[a, e]
            F = 0.5 * np.mean((yc - Xc @ b) ** 2) - 0.5 * np.mean(yc ** 2) + etas[e] * b @ b + alphas[a] * plain.n_active_groups_[a, e]
            assert abs(F - plain.objectives_[a, e]) <= 1e-9 * max(abs(F), alphas[a])


def test_cv_search_gives_sklearn_shaped_results():
    from sparselm_amd.miqp import L0LocalGroupCV, l0_local_group_cv, l0_local_group_search

    X, y, gstart = group_law(5, n=90, rho=0.3, snr=10.0)
    groups = gid_of(gstart)
    hierarchy = [[]] + [[g - 1] for g in range(1, 7)]
    alphas, etas = np.array([0.01, 0.05, 0.5]) * var(y), [0.0, 0.05]
    res = l0_local_group_cv(X, y, alphas=alphas, etas=etas, groups=groups, hierarchy=hierarchy, cv=3, fit_intercept=True)
    assert isinstance(res, L0LocalGroupCV) and len(res.paths_) == 3 and res.cell_scores_.shape == (3, 3, 2)
    assert res.solver_info_["launches"] == res.solver_info_["rounds"] <= 3 and res.solver_info_["proven_optimal"] is False
    assert res.full_.group_supports_.shape == (3, 2, 7)
    full = l0_local_group_search(X, y, alphas=alphas, etas=etas, groups=groups, hierarchy=hierarchy, fit_intercept=True)
    np.testing.assert_array_equal(res.full_.group_supports_, full.group_supports_)
    np.testing.assert_allclose(res.full_.objectives_, full.objectives_, rtol=1e-9)
    for method in ("max_score", "one_std_score"):
        found = res.search(method)
        cvr = found.cv_results_
        assert [set(prm) for prm in cvr["params"]] == [{"alpha", "eta"}] * 6
        for key in ("mean_test_score", "std_test_score", "rank_test_score", "split0_test_score", "split2_test_score"):
            assert len(cvr[key]) == 6
        a, e = divmod(found.best_index_, 2)
        np.testing.assert_array_equal(found.coef_, res.full_.coefs_[a, e])
        assert found.best_params_ == {"alpha": float(alphas[a]), "eta": float(etas[e])}
        assert found.predict(X).shape == (90,)
