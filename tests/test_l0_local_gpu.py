"""The l0 local search on the GPU (``slm_solve_l0_local``, csrc/l0_local_kernels.hpp) against the numpy restatement of its
rule (tests/_l0_local_reference.py) and, where the columns fit, against the exact estimators on the same device.

The restatement reports the smallest relative margin by which it took any decision (a threshold ``gain > alpha``, a swap, the
lead of an entering column over the runner-up; with several starts, the lead of the winning start's objective).  Every
comparison first asserts that this margin is >= 1e-6, so that rounding -- the kernel contracts multiply-adds and sums in
another order -- cannot change a decision; then: identical supports, swap counts and winning starts, objectives (after the
polish) to 1e-10 relative, the tolerance of tests/test_l0_gpu.py.  Every returned cell must also pass the independent
certificate ``is_swap_inescapable``.  Rows stay at n <= 200.

Against ``RegularizedL0`` / ``L2L0``: at p = 20 on the hard law (too wide for a brute force in a test, within the exact
search's 64 columns) the local objective is never below the proven optimum; on the committed cases of
tests/test_l0_local_cpu.py (that law at p = 14, where the restatement was checked against brute force) it EQUALS it."""

import functools
import warnings

import numpy as np
import pytest
from sklearn.exceptions import ConvergenceWarning

from _l0_local_reference import gram, hard_law, is_swap_inescapable, solve_cells

pytestmark = pytest.mark.gpu

MARGIN_MIN, OBJ_RTOL, CERT_TOL = 1e-6, 1e-10, 1e-8


def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def draw(n, p, k, seed, rho=0.5, noise=0.5, spread=False):
    """n x p AR(1) columns, k true columns with coefficients +-1 (``spread``: one in every block of 64 columns)."""
    rng = np.random.default_rng(seed)
    Z = rng.standard_normal((n, p))
    X = Z.copy()
    for j in range(1, p):
        X[:, j] = rho * X[:, j - 1] + np.sqrt(1.0 - rho * rho) * Z[:, j]
    beta = np.zeros(p)
    cols = 64 * np.arange(k) + rng.integers(0, 64, k) if spread else rng.choice(p, min(k, p), replace=False)
    beta[cols] = (-1.0) ** np.arange(len(cols))
    y = X @ beta + noise * rng.standard_normal(n)
    return freeze(X, y)


def engine_cells(X, y, alphas, etas, big_M=100.0, starts=None, swaps=True, sample_weight=None, fit_intercept=False, binding=None):
    from sparselm_amd import _engine

    n = X.shape[0]
    w = None if sample_weight is None else np.asarray(sample_weight) * (n / np.sum(sample_weight))
    with _engine.get_engine().dataset(X, y, row_weight=w) as ds:
        if fit_intercept:
            ds.center()
        return ds.solve_l0_local(alphas, etas, big_M=big_M, starts=starts, swaps=swaps, binding=binding)


def compare(X, y, alphas, etas=None, big_M=100.0, starts=None, swaps=True, sample_weight=None, fit_intercept=False, expect=None):
    """The comparison every test shares: the premise on the restatement's margins, then supports, swap counts, winning starts,
    objectives, the certificate.  Returns (the restatement's cells, the engine's result)."""
    alphas = np.asarray(alphas, dtype=float)
    etas = np.zeros_like(alphas) if etas is None else np.asarray(etas, dtype=float)
    ref = solve_cells(X, y, alphas, etas, big_M=big_M, starts=starts, swaps=swaps, sample_weight=sample_weight, fit_intercept=fit_intercept)
    betas, objectives, winners, infos = engine_cells(X, y, alphas, etas, big_M, starts, swaps, sample_weight, fit_intercept)
    for e, cell in enumerate(ref):
        print(f"cell {e}: alpha {alphas[e]:.4g} eta {etas[e]:.4g} margin {cell['margin']:.3e} lead {cell['lead']:.3e} reference objective "
              f"{cell['objective']:.12e} swaps {cell['swaps']} start {cell['start']} nnz {np.count_nonzero(cell['beta'])}; engine objective "
              f"{objectives[e]:.12e} swaps {infos[e]['swaps']} start {winners[e]} sweeps {infos[e]['sweeps']}")
        assert cell["status"] == 0 and cell["margin"] >= MARGIN_MIN and cell["lead"] >= MARGIN_MIN  # the premise
        assert infos[e]["converged"] and infos[e]["status"] == "fixed_point" and infos[e]["proven_optimal"] is False
        np.testing.assert_array_equal(betas[e] != 0.0, cell["beta"] != 0.0)
        assert infos[e]["swaps"] == cell["swaps"] and winners[e] == cell["start"]
        scale = max(abs(cell["objective"]), alphas[e], np.finfo(float).tiny)
        assert abs(objectives[e] - cell["objective"]) <= OBJ_RTOL * scale and objectives[e] == infos[e]["objective"]
        assert infos[e]["objective"] <= infos[e]["descent_objective"] + OBJ_RTOL * scale  # the polish does not raise it
        assert np.all(np.abs(betas[e]) <= big_M)
        ok, why = is_swap_inescapable(cell["H"], cell["c"], alphas[e], big_M, betas[e], CERT_TOL, swaps=swaps)
        assert ok, why
    if expect is not None:
        expect(ref, betas, infos)
    return ref, (betas, objectives, winners, infos)


def var(y):
    return float(np.var(y))


# ---- 1. widths: one column, the slot boundary, several slots, all sixteen -----------------------------------------------------------
def test_one_column_and_one_cell():
    X, y = draw(20, 1, 1, 0)
    compare(X, y, [0.01 * var(y)])                 # one cell: the column enters
    compare(X, y, [0.01 * var(y), 10.0 * var(y)])  # ... and an alpha that keeps it out


@pytest.mark.parametrize("p", [63, 64, 65, 130])
def test_slot_boundaries(p):
    """63: one slot with an idle lane; 64: one full slot (ld = p); 65: a second slot of one lane; 130: three slots.  The leading
    dimension of the Gram (p rounded up to 16) differs from p at 63, 65 and 130."""
    X, y = draw(80, p, 6, p)
    compare(X, y, np.array([0.01, 0.05, 0.3]) * var(y), etas=[0.0, 0.02, 0.0])
    # the last column is reached: a signal in it alone is found
    y2 = 2.0 * X[:, p - 1] + 0.1 * draw(80, p, 6, p + 1000)[1]
    ref, (betas, _, _, _) = compare(X, y2, [0.05 * var(y2)])
    assert betas[0][p - 1] != 0.0


def test_every_slot_live_at_1024_columns():
    """p = 1024, n = 200: a well-conditioned support of 16 columns, one in each slot, from zero and from a wrong start."""
    X, y = draw(200, 1024, 16, 3, rho=0.0, noise=0.3, spread=True)
    start = np.zeros((1, 1, 1024))
    start[0, 0, 5::64] = 0.5  # sixteen wrong columns, one per slot
    # (two calls, not two starts of one: both reach the same support, and a tie in F to the last bit names no winner)
    for starts in (None, start):
        _, (betas, _, _, _) = compare(X, y, [0.015 * var(y)], starts=starts)
        live = np.flatnonzero(betas[0])
        assert set(live // 64) == set(range(16)) and live.size == 16  # every slot holds an active column


# ---- 2. the problems of one launch ---------------------------------------------------------------------------------------------------
def test_more_problems_than_one_grid_pass():
    """The launch holds at most 2 x CUs workgroups of four waves: with more problems than that the grid-stride loop serves the
    rest.  Seven distinct alphas repeated, so that the restatement runs seven times."""
    from sparselm_amd import _engine

    X, y = draw(30, 6, 3, 11)
    cus = int(_engine.get_engine().device_info()["compute_units"])
    cells = min(2 * cus * 4 + 9, 8192)
    assert cells > 2 * cus * 4 or cus >= 1024
    distinct = np.array([0.001, 0.003, 0.01, 0.03, 0.1, 0.3, 3.0]) * var(y)
    ref = solve_cells(X, y, distinct, np.zeros(7))
    assert all(cell["margin"] >= MARGIN_MIN for cell in ref) and len({tuple(cell["beta"] != 0) for cell in ref}) >= 2
    alphas = distinct[np.arange(cells) % 7]
    betas, objectives, winners, infos = engine_cells(X, y, alphas, np.zeros(cells))
    assert betas.shape == (cells, 6) and not winners.any()
    for e in range(cells):
        cell = ref[e % 7]
        assert np.array_equal(betas[e] != 0.0, cell["beta"] != 0.0) and infos[e]["swaps"] == cell["swaps"], e
        assert abs(objectives[e] - cell["objective"]) <= OBJ_RTOL * max(abs(cell["objective"]), alphas[e]), e
    # the same cell gives the same bytes wherever it sits in the grid
    for e in range(7, cells):
        assert betas[e].tobytes() == betas[e % 7].tobytes(), e


def test_two_starts_the_second_wins():
    """On the hard law the search from zero misses the optimum at seed 0; a start on the optimum's support wins."""
    from _l0_reference import brute_force

    X, y = hard_law(0)
    alpha = 0.05 * var(y)
    exact = brute_force(X, y, alpha=alpha, big_M=100.0)
    starts = np.stack([np.zeros(14), exact["coef"]])[None]

    def expect(ref, betas, infos):
        assert ref[0]["start"] == 1 and ref[0]["F"][1] < ref[0]["F"][0]
        assert abs(infos[0]["objective"] - exact["objective"]) <= OBJ_RTOL * abs(exact["objective"])

    compare(X, y, [alpha], starts=starts, expect=expect)
    # the other order: the winner's index follows
    _, (_, _, winners, _) = compare(X, y, [alpha], starts=starts[:, ::-1])
    assert winners[0] == 0


# ---- 3. the box, the ridge, the ends of the alpha range ----------------------------------------------------------------------------
def test_big_m_binds_on_an_active_coordinate():
    X, y = draw(60, 20, 5, 7)

    def expect(ref, betas, infos):
        assert np.any(np.abs(betas[0]) == 0.6) and np.any((betas[0] != 0.0) & (np.abs(betas[0]) < 0.6))

    compare(X, y, [0.01 * var(y)], big_M=0.6, expect=expect)


def test_ridge_with_fewer_rows_than_columns():
    X, y = draw(15, 40, 4, 9)
    compare(X, y, np.array([0.005, 0.02, 0.02]) * var(y), etas=[0.05, 0.05, 0.5])


def test_alpha_that_empties_the_support_and_alpha_zero():
    X, y = draw(40, 12, 4, 5)
    _, (betas, objectives, _, _) = compare(X, y, [10.0 * var(y)])
    assert not betas.any() and objectives[0] == 0.0
    # alpha = 0: every column enters and the result is least squares
    _, (betas, objectives, _, _) = compare(X, y, [0.0])
    ls = np.linalg.lstsq(X, y, rcond=None)[0]
    assert np.count_nonzero(betas[0]) == 12 and np.max(np.abs(betas[0] - ls)) <= 1e-9 * np.max(np.abs(ls))


# ---- 4. the Python layer -------------------------------------------------------------------------------------------------------------
def test_swaps_false_gives_the_descents_fixed_point():
    from sparselm_amd.miqp import l0_local_search

    X, y = hard_law(12)  # (on the committed list: one swap reaches the optimum)
    alpha = 0.1 * var(y)
    ref_d, _ = compare(X, y, [alpha], swaps=False)
    ref_s, _ = compare(X, y, [alpha], swaps=True)
    assert ref_d[0]["swaps"] == 0 and ref_s[0]["swaps"] == 1 and ref_s[0]["objective"] < ref_d[0]["objective"]
    descent = l0_local_search(X, y, alphas=[alpha], max_rounds=0, solver_options={"swaps": False})
    full = l0_local_search(X, y, alphas=[alpha], max_rounds=0)
    assert descent.swaps_[0, 0] == 0 and full.swaps_[0, 0] == 1 and full.objectives_[0, 0] < descent.objectives_[0, 0]
    np.testing.assert_array_equal(descent.supports_[0, 0], ref_d[0]["beta"] != 0)
    np.testing.assert_array_equal(full.supports_[0, 0], ref_s[0]["beta"] != 0)
    assert full.proven_optimal_ is False and full.converged_.all() and full.rounds_ == 1


def test_sample_weights_and_intercept():
    from sparselm_amd.miqp import l0_local_search

    X, y = draw(50, 16, 4, 13)
    X = X + 3.0
    w = np.random.default_rng(2).uniform(0.2, 2.0, 50)
    alphas = np.array([0.01, 0.1]) * var(y)
    ref, _ = compare(X, y + 5.0, alphas, sample_weight=w, fit_intercept=True)
    path = l0_local_search(X, y + 5.0, alphas=alphas, sample_weight=w, fit_intercept=True, max_rounds=0)
    _, _, _, x_mean, y_mean = gram(X, y + 5.0, w, True)
    for a in range(2):
        np.testing.assert_array_equal(path.supports_[a, 0], ref[a]["beta"] != 0)
        assert abs(path.objectives_[a, 0] - ref[a]["objective"]) <= OBJ_RTOL * abs(ref[a]["objective"])
        assert abs(path.intercepts_[a, 0] - (y_mean - x_mean @ path.coefs_[a, 0])) <= 1e-12 * abs(y_mean)
        np.testing.assert_allclose(path.predict(X[:5], a), X[:5] @ path.coefs_[a, 0] + path.intercepts_[a, 0], rtol=0, atol=0)
        resid = X @ path.coefs_[a, 0] + path.intercepts_[a, 0] - (y + 5.0)
        loss = float((w * (50 / w.sum())) @ resid**2) / 100.0
        assert abs(path.losses_[a, 0] - loss) <= 1e-9 * loss
    # without the intercept the shifted data give another answer: the centring is not a no-op
    flat = l0_local_search(X, y + 5.0, alphas=alphas, sample_weight=w, max_rounds=0)
    assert not np.allclose(flat.coefs_, path.coefs_) and not flat.intercepts_.any()


def test_both_routes_byte_for_byte_and_refuse_1025_columns():
    from sparselm_amd import _engine

    if _engine.load_binding() is None:
        pytest.fail("the compiled binding is not built")
    X, y = draw(60, 70, 5, 21)
    alphas, etas = np.array([0.01, 0.05, 0.2]) * var(y), np.array([0.0, 0.01, 0.0])
    starts = np.zeros((3, 2, 70))
    starts[:, 1, ::9] = 0.25
    a = engine_cells(X, y, alphas, etas, starts=starts, binding=False)
    b = engine_cells(X, y, alphas, etas, starts=starts, binding=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert a[0].any()
    wide = np.random.default_rng(0).standard_normal((8, 1025))
    with _engine.get_engine().dataset(wide, np.ones(8)) as ds:
        for route in (False, True):
            with pytest.raises(NotImplementedError, match="up to 1024 columns"):
                ds.solve_l0_local([0.1], binding=route)
            with pytest.raises(NotImplementedError, match="up to 1024 columns"):
                ds.solve_l0_local([0.1], swaps=False, binding=route)
    with _engine.get_engine().dataset(X, y) as ds:
        for route in (False, True):
            for bad, words in ((dict(alphas=[-1.0]), "alphas"), (dict(alphas=[0.1], etas=[np.nan]), "etas"), (dict(alphas=[0.1], big_M=-1.0), "big_M"),
                               (dict(alphas=[0.1], n_cells=0), "n_cells"), (dict(alphas=[0.1], n_starts=0), "n_starts"),
                               (dict(alphas=np.full(8193, 0.1)), "problems"), (dict(alphas=[0.1], big_M=0.1, starts=starts[:1]), "box")):
                with pytest.raises(ValueError, match=words):
                    ds.solve_l0_local(binding=route, **bad)
        ds.set_groups(np.arange(70) // 2, 35)
        for route in (False, True):
            with pytest.raises(NotImplementedError, match="groups"):
                ds.solve_l0_local([0.1], binding=route)


# ---- 5. against the exact search on the same device ---------------------------------------------------------------------------------
def exact_fit(X, y, alpha, eta):
    from sparselm_amd.miqp import L2L0, RegularizedL0

    est = L2L0(alpha=alpha, eta=eta, big_M=100) if eta > 0.0 else RegularizedL0(alpha=alpha, big_M=100)
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        est.fit(X, y)
    assert est.solver_info_["proven_optimal"]
    return est.solver_info_["objective"]


def test_never_below_the_proven_optimum_at_20_columns():
    from sparselm_amd.miqp import l0_local_search

    hits = 0
    for seed in (0, 1, 2):
        X, y = hard_law(seed, p=20)
        alphas, etas = np.array([0.02, 0.1]) * var(y), [0.0, 0.05]
        path = l0_local_search(X, y, alphas=alphas, etas=etas)
        for a in range(2):
            for e in range(2):
                exact = exact_fit(X, y, alphas[a], etas[e])
                print(f"seed {seed} alpha {alphas[a]:.4g} eta {etas[e]}: local {path.objectives_[a, e]:.12e} exact {exact:.12e}")
                assert path.objectives_[a, e] >= exact - OBJ_RTOL * abs(exact)
                hits += abs(path.objectives_[a, e] - exact) <= OBJ_RTOL * abs(exact)
    print(f"{hits} of 12 cells at the proven optimum")


def test_equal_to_the_proven_optimum_on_the_committed_cases():
    from test_l0_local_cpu import SWAPS_REACH_OPTIMUM

    from sparselm_amd.miqp import l0_local_search

    for seed, rel in SWAPS_REACH_OPTIMUM:
        X, y = hard_law(seed)
        alpha = rel * var(y)
        path = l0_local_search(X, y, alphas=[alpha], max_rounds=0)
        exact = exact_fit(X, y, alpha, 0.0)
        assert path.swaps_[0, 0] >= 1 and abs(path.objectives_[0, 0] - exact) <= OBJ_RTOL * abs(exact), (seed, rel)


# ---- 6. rounds -------------------------------------------------------------------------------------------------------------------------
def test_rounds_never_raise_an_objective_and_improve_a_cell():
    from sparselm_amd.miqp import l0_local_search

    X, y = hard_law(4, p=20)
    alphas = np.geomspace(0.005, 0.3, 8) * var(y)
    one = l0_local_search(X, y, alphas=alphas, etas=[0.0, 0.02], max_rounds=0)
    path = l0_local_search(X, y, alphas=alphas, etas=[0.0, 0.02], max_rounds=3)
    print("rounds", path.rounds_, "\n", path.round_objectives_)
    assert one.rounds_ == 1 and 2 <= path.rounds_ <= 4 and path.round_objectives_.shape == (path.rounds_, 8, 2)
    np.testing.assert_array_equal(path.round_objectives_[0], one.objectives_)
    np.testing.assert_array_equal(path.round_objectives_[-1], path.objectives_)
    assert np.all(np.diff(path.round_objectives_, axis=0) <= 0.0)
    assert np.any(path.round_objectives_[1] < path.round_objectives_[0])  # a cell improves in round 1
    G, c, _, _, _ = gram(X, y)
    for a in range(8):
        for e in range(2):
            H = G + 2.0 * path.etas_[e] * np.eye(20)
            ok, why = is_swap_inescapable(H, c, alphas[a], 100.0, path.coefs_[a, e], CERT_TOL)
            assert ok, (a, e, why)



# ---- 7. the one body behind the single-set entry: an empty winner, a start across the slot boundary, non-finite data ---------------
def empty_and_live(X, y, starts=None):
    """Two cells, the second with an alpha no column's gain reaches: its winner is empty -- objective 0, loss yy / 2, beta 0."""
    yy = gram(X, y)[2]
    alphas = np.array([0.02, 10.0]) * var(y)
    ref, (betas, objectives, _, infos) = compare(X, y, alphas, starts=starts)
    assert ref[0]["beta"].any() and not ref[1]["beta"].any()
    assert not betas[1].any() and objectives[1] == 0.0 and infos[1]["objective"] == 0.0
    # (yy is a sum of n products on either side: they differ by rounding alone, n eps at the most)
    assert abs(infos[1]["loss"] - 0.5 * yy) <= 1e-12 * yy
    return alphas


def test_an_empty_winner_fetches_no_row_of_the_gram():
    X, y = draw(30, 6, 3, 11)
    alphas = empty_and_live(X, y)
    # the empty cell alone: no winner of the call holds a column
    betas, objectives, winners, infos = engine_cells(X, y, alphas[1:], np.zeros(1))
    assert not betas.any() and objectives[0] == 0.0 and winners[0] == 0 and infos[0]["converged"]
    assert abs(infos[0]["loss"] - 0.5 * gram(X, y)[2]) <= 1e-12 * gram(X, y)[2]


def test_an_empty_winner_from_a_start_across_the_slot_boundary():
    X, y = draw(80, 65, 6, 65)
    starts = np.zeros((2, 1, 65))
    starts[:, 0, 62:65] = 0.25  # columns 62 and 63 of the first slot, column 64 of the second
    empty_and_live(X, y, starts=starts)


def test_non_finite_data_is_refused_by_both_entries():
    """One NaN in X: the dataset is built (only y is checked there), X^T y is not finite, and both entries say so by ctypes."""
    from sparselm_amd import _engine

    X, y = draw(30, 6, 3, 11)
    X = X.copy()
    X[4, 2] = np.nan
    with _engine.get_engine().dataset(X, y) as ds:
        with pytest.raises(_engine.NonFiniteError, match="non-finite"):
            ds.solve_l0_local([0.1], binding=False)
        with pytest.raises(_engine.NonFiniteError, match="non-finite"):
            ds.solve_l0_local_folds([None], [0], [0.1], binding=False)
