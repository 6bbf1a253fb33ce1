"""The l0 local search over row sets on the GPU (``slm_solve_l0_local_folds``, csrc/l0_local_kernels.hpp) and ``l0_local_cv``.

The comparison is the one of ``tests/test_l0_local_gpu.compare``, per (row set, cell), against the numpy restatement run on
``X[rows], y[rows]`` directly (tests/_l0_local_cv_cases.py): an independent route -- rows selected and centred in numpy, no Gram
of a complement, no elimination.  Under the premise (status 0, every decision margin and lead >= 1e-6, asserted here and
recomputed by tests/test_l0_local_cv_cpu.py): identical supports, swap counts and winning starts, objectives to 1e-10, the
certificate ``is_swap_inescapable`` at 1e-8, intercepts to 1e-9 relative to max |y|.

``l0_local_cv`` end to end: every fold against ``l0_local_search`` on the fold's rows -- same supports, objectives to 1e-10.  The
coefficients are NOT byte for byte: a fold's Gram is built from the complement of its held-out rows, and centring is by
elimination of the ones column."""

import warnings

import numpy as np
import pytest
from sklearn.exceptions import ConvergenceWarning
from sklearn.model_selection import KFold, ParameterGrid

from _l0_local_cv_cases import RUNS, case, masks, reference, second_start_case
from _l0_local_reference import gram, is_swap_inescapable, solve_cells
from test_l0_local_gpu import CERT_TOL, MARGIN_MIN, OBJ_RTOL, draw, var

pytestmark = pytest.mark.gpu


def folds_cells(X, y, weights, n_effs, alphas, etas, intercept=False, binding=None, **kw):
    from sparselm_amd import _engine

    Xd = np.hstack([X, np.ones((X.shape[0], 1))]) if intercept else X
    with _engine.get_engine().dataset(Xd, y) as ds:
        return ds.solve_l0_local_folds(weights, n_effs, alphas, etas, intercept=intercept, binding=binding, **kw)


def check_against(ref, result, alphas, y, swaps=True, big_M=100.0):
    """Per (row set, cell): the premise, then supports, swap counts, winning starts, objectives, the certificate, the intercept."""
    betas, icpts, objectives, winners, stats, infos = result
    ymax = float(np.max(np.abs(y)))
    for r, cells in enumerate(ref):
        for e, cell in enumerate(cells):
            print(f"row set {r} cell {e}: margin {cell['margin']:.3e} lead {cell['lead']:.3e} reference objective {cell['objective']:.12e} swaps "
                  f"{cell['swaps']} start {cell['start']} nnz {np.count_nonzero(cell['beta'])}; engine objective {objectives[r, e]:.12e} swaps "
                  f"{infos[r][e]['swaps']} start {winners[r, e]} intercept {icpts[r, e]:.12e} against {cell['intercept']:.12e}")
            assert cell["status"] == 0 and cell["margin"] >= MARGIN_MIN and cell["lead"] >= MARGIN_MIN  # the premise
            info = infos[r][e]
            assert info["converged"] and info["status"] == "fixed_point" and info["proven_optimal"] is False
            np.testing.assert_array_equal(betas[r, e] != 0.0, cell["beta"] != 0.0)
            assert info["swaps"] == cell["swaps"] and winners[r, e] == cell["start"]
            scale = max(abs(cell["objective"]), alphas[e], np.finfo(float).tiny)
            assert abs(objectives[r, e] - cell["objective"]) <= OBJ_RTOL * scale and objectives[r, e] == info["objective"]
            assert info["objective"] <= info["descent_objective"] + OBJ_RTOL * scale  # the polish does not raise it
            assert np.all(np.abs(betas[r, e]) <= big_M)
            ok, why = is_swap_inescapable(cell["H"], cell["c"], alphas[e], big_M, betas[r, e], CERT_TOL, swaps=swaps)
            assert ok, why
            assert abs(icpts[r, e] - cell["intercept"]) <= 1e-9 * ymax
            # the four words of the winner among those of every problem
            w = stats[r, e, winners[r, e]]
            assert (w[0], w[1], w[2], w[3]) == (info["sweeps"], info["swaps"], 0, np.count_nonzero(betas[r, e]))


# ---- 1. the cases of tests/_l0_local_cv_cases.py ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,intercept", RUNS)
def test_row_sets_against_the_restatement_on_the_rows(name, intercept):
    X, y, rows, alphas, etas = case(name, intercept)
    ref = reference(name, intercept)
    # (all rows as a set of ones, so that every Gram comes from the folds' call -- and, with an intercept, as None: one by one)
    weights, n_effs = masks(X.shape[0], rows, all_rows_given=not intercept)
    result = folds_cells(X, y, weights, n_effs, alphas, etas, intercept=intercept)
    check_against(ref, result, alphas, y)
    assert result[0].shape == (len(rows), len(alphas), X.shape[1]) and result[4].shape == (len(rows), len(alphas), 1, 4)
    if not intercept:
        assert not result[1].any()


def test_1025_columns_are_taken_with_an_intercept_and_1026_refused():
    from sparselm_amd import _engine

    wide = np.random.default_rng(0).standard_normal((8, 1026))
    with _engine.get_engine().dataset(wide, np.ones(8)) as ds:
        for route in (False, True):
            with pytest.raises(NotImplementedError, match="up to 1024 columns beside the intercept's"):
                ds.solve_l0_local_folds([None], [0], [0.1], intercept=True, binding=route)
    with _engine.get_engine().dataset(wide[:, :1025], np.ones(8)) as ds:
        for route in (False, True):
            with pytest.raises(NotImplementedError, match="up to 1024 columns"):
                ds.solve_l0_local_folds([None], [0], [0.1], binding=route)


def test_more_problems_than_one_grid_pass_on_sixteen_row_sets():
    """130 cells (the two of the case, repeated) x 16 row sets = 2080 problems: more than the 2 x CUs workgroups of four waves that
    one pass of the grid holds at 256 CUs.  Equal cells of one row set give equal bytes wherever they sit."""
    from sparselm_amd import _engine

    X, y, rows, alphas, etas = case("sixteen_row_sets", False)
    ref = reference("sixteen_row_sets", False)
    cus = int(_engine.get_engine().device_info()["compute_units"])
    cells = 130
    problems = 16 * cells
    assert problems > 2 * cus * 4 or cus > 256
    weights, n_effs = masks(X.shape[0], rows)
    betas, icpts, objectives, winners, stats, infos = folds_cells(X, y, weights, n_effs, alphas[np.arange(cells) % 2], np.zeros(cells))
    assert betas.shape == (16, cells, 6) and not winners.any()
    for r in range(16):
        for e in range(cells):
            cell = ref[r][e % 2]
            assert cell["status"] == 0 and cell["margin"] >= MARGIN_MIN
            assert np.array_equal(betas[r, e] != 0.0, cell["beta"] != 0.0) and infos[r][e]["swaps"] == cell["swaps"], (r, e)
            assert abs(objectives[r, e] - cell["objective"]) <= OBJ_RTOL * max(abs(cell["objective"]), alphas[e % 2]), (r, e)
            if e >= 2:
                assert betas[r, e].tobytes() == betas[r, e % 2].tobytes() and objectives[r, e] == objectives[r, e % 2], (r, e)
                assert np.array_equal(stats[r, e], stats[r, e % 2]), (r, e)


# ---- 2. one row set is the parent's call ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("swaps", [True, False])
def test_one_null_row_set_equals_solve_l0_local_byte_for_byte(swaps):
    from sparselm_amd import _engine

    if _engine.load_binding() is None:
        pytest.fail("the compiled binding is not built")
    X, y = draw(60, 70, 5, 21)
    alphas, etas = np.array([0.01, 0.05, 0.2]) * var(y), np.array([0.0, 0.01, 0.0])
    starts = np.zeros((3, 2, 70))
    starts[:, 1, ::9] = 0.25
    with _engine.get_engine().dataset(X, y) as ds:
        for route in (False, True):
            a = ds.solve_l0_local(alphas, etas, starts=starts, swaps=swaps, binding=route)
            b = ds.solve_l0_local_folds([None], [0], alphas, etas, starts=starts[None], swaps=swaps, binding=route)
            assert a[0].any() and a[0].tobytes() == b[0][0].tobytes() and a[1].tobytes() == b[2][0].tobytes()
            assert np.array_equal(a[2], b[3][0]) and a[3] == b[5][0] and not b[1].any()
            assert b[4].shape == (1, 3, 2, 4)


def test_the_same_weights_twice_give_the_same_bytes():
    X, y, rows, alphas, etas = case("two_slots", True)
    weights, n_effs = masks(X.shape[0], rows)
    twice = ([weights[0], weights[1], weights[0].copy()], [n_effs[0], n_effs[1], n_effs[0]])
    betas, icpts, objectives, winners, stats, infos = folds_cells(X, y, *twice, alphas, etas, intercept=True)
    assert betas[0].any() and betas[0].tobytes() == betas[2].tobytes() and betas[0].tobytes() != betas[1].tobytes()
    assert icpts[0].tobytes() == icpts[2].tobytes() and objectives[0].tobytes() == objectives[2].tobytes()
    assert np.array_equal(stats[0], stats[2]) and infos[0] == infos[2]


# ---- 3. starts, weights --------------------------------------------------------------------------------------------------------------
def test_a_second_start_wins_in_one_row_set_and_loses_in_another():
    X, y, rows, alphas, starts, ref, wins = second_start_case()
    for e in range(3):
        assert sorted(set(wins[:, e])) == [0, 1]
    weights, n_effs = masks(X.shape[0], rows)
    result = folds_cells(X, y, weights, n_effs, alphas, np.zeros(3), intercept=True, starts=np.broadcast_to(starts, (4, 3, 2, 14)))
    check_against(ref, result, alphas, y)
    np.testing.assert_array_equal(result[3], wins)
    assert result[4].shape == (4, 3, 2, 4) and np.all(result[4][..., 2] == 0)  # the losers' words are there too


def test_sample_weights_that_are_not_masks_times_folds():
    X, y = draw(50, 16, 4, 13)
    X = X + 3.0
    y = y + 5.0
    w = np.random.default_rng(2).uniform(0.2, 2.0, 50)
    alphas = np.array([0.01, 0.1]) * var(y)
    rows = [tr for tr, _ in KFold(3).split(X)] + [np.arange(50)]
    weights, n_effs, ref = [], [], []
    for r in rows:
        m = np.zeros(50)
        m[r] = w[r] * (len(r) / w[r].sum())  # as l0_local_cv normalises: the set's weights sum to its row count
        weights.append(m)
        n_effs.append(len(r))
        cells = solve_cells(X[r], y[r], alphas, np.zeros(2), sample_weight=w[r], fit_intercept=True)
        _, _, _, x_mean, y_mean = gram(X[r], y[r], w[r], True)
        for cell in cells:
            cell["intercept"] = float(y_mean - x_mean @ cell["beta"])
        ref.append(cells)
    check_against(ref, folds_cells(X, y, weights, n_effs, alphas, np.zeros(2), intercept=True), alphas, y)


# ---- 4. every refusal, by both routes --------------------------------------------------------------------------------------------------
def test_every_refusal_by_both_routes():
    from sparselm_amd import _engine

    X, y = draw(60, 70, 5, 21)
    ones = np.ones(60)
    starts = np.full((1, 1, 1, 70), 0.25)
    with _engine.get_engine().dataset(X, y) as ds:
        for route in (False, True):
            for bad, words in ((dict(alphas=[-1.0]), "alphas"), (dict(alphas=[0.1], etas=[np.nan]), "etas"), (dict(alphas=[0.1], big_M=-1.0), "big_M"),
                               (dict(alphas=[0.1], n_cells=0), "n_cells"), (dict(alphas=[0.1], n_starts=0), "n_starts"),
                               (dict(alphas=np.full(8193, 0.1)), r"count \* n_cells \* n_starts"),
                               (dict(alphas=[0.1], big_M=0.1, starts=starts), "box")):
                with pytest.raises(ValueError, match=words):
                    ds.solve_l0_local_folds([None], [0], binding=route, **bad)
            with pytest.raises(ValueError, match=r"count \* n_cells \* n_starts must be at most 8192 problems \(got 3 x 2731 x 1\)"):
                ds.solve_l0_local_folds([None, ones, None], [0, 60, 0], np.full(2731, 0.1), binding=route)
            for count in (0, 17):
                with pytest.raises(ValueError, match="count must be 1 .. 16"):
                    ds.solve_l0_local_folds([None] * count, [0] * count, [0.1], binding=route)
            for value in (-1.0, np.nan, np.inf):
                w = ones.copy()
                w[7] = value
                with pytest.raises(ValueError, match=r"row_weights\[1\]\[7\]"):
                    ds.solve_l0_local_folds([None, w], [0, 60], [0.1], binding=route)
        ds.set_groups(np.r_[np.arange(69), 68], 69)  # the last column shares its group
        for route in (False, True):
            with pytest.raises(ValueError, match="the last column must be alone"):
                ds.solve_l0_local_folds([None], [0], [0.1], intercept=True, binding=route)
            with pytest.raises(NotImplementedError, match="groups"):
                ds.solve_l0_local_folds([None], [0], [0.1], binding=route)
    # a last column that no row set weighs: refused once the Grams are there (here the column is zero, so G11 = 0 in every set)
    Z = X.copy()
    Z[:, -1] = 0.0
    with _engine.get_engine().dataset(Z, y) as ds:
        for route in (False, True):
            with pytest.raises(ValueError, match="row set 0 gives the last column no weight"):
                ds.solve_l0_local_folds([None, ones], [0, 60], [0.1], intercept=True, binding=route)


# ---- 5. l0_local_cv end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("intercept", [False, True])
def test_l0_local_cv_end_to_end(intercept):
    from sparselm_amd.miqp import l0_local_cv, l0_local_search
    from sparselm_amd.model_selection import _format_results, select_best_index_onestd

    X, y = draw(60, 65, 6, 65)
    if intercept:
        X, y = X + 1.0, y + 2.0
    alphas, etas = np.array([0.01, 0.05, 0.3]) * var(y), [0.0, 0.02]
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        cv = l0_local_cv(X, y, alphas=alphas, etas=etas, cv=3, fit_intercept=intercept)
        five = l0_local_cv(X, y, alphas=alphas, etas=etas, cv=5, fit_intercept=intercept)
    assert len(cv.paths_) == 3 and len(cv.splits_) == 3 and cv.cell_scores_.shape == (3, 3, 2) and cv.proven_optimal_ is False
    for path, rows in [(cv.paths_[f], tr) for f, (tr, _) in enumerate(cv.splits_)] + [(cv.full_, np.arange(60))]:
        alone = l0_local_search(X[rows], y[rows], alphas=alphas, etas=etas, fit_intercept=intercept)
        np.testing.assert_array_equal(path.supports_, alone.supports_)
        scale = np.maximum(np.abs(alone.objectives_), alphas[:, None])
        assert np.all(np.abs(path.objectives_ - alone.objectives_) <= OBJ_RTOL * scale)
        assert np.all(np.abs(path.coefs_ - alone.coefs_) <= 1e-8 * np.max(np.abs(alone.coefs_)))
        assert np.all(np.abs(path.intercepts_ - alone.intercepts_) <= 1e-9 * np.max(np.abs(y)))
        assert np.all(np.abs(path.losses_ - alone.losses_) <= 1e-9 * np.abs(alone.losses_))
        assert path.converged_.all() and path.round_objectives_.shape == (cv.solver_info_["rounds"], 3, 2)
        assert np.all(np.diff(path.round_objectives_, axis=0) <= 0.0)  # the rounds never raise an objective
        np.testing.assert_array_equal(path.round_objectives_[-1], path.objectives_)
        if not intercept:
            assert not path.intercepts_.any()
    # held-out scores, recomputed
    for f, (_, te) in enumerate(cv.splits_):
        for a in range(3):
            for e in range(2):
                resid = y[te] - cv.paths_[f].predict(X[te], a, e)
                assert cv.cell_scores_[f, a, e] == pytest.approx(-np.sqrt(np.mean(resid**2)), rel=1e-12)
    # the grid, both rules
    res = cv.search()
    assert res.cv_results_["params"] == list(ParameterGrid({"alpha": [float(a) for a in alphas], "eta": [0.0, 0.02]}))
    assert [k for k in res.cv_results_ if k.startswith("split")] == ["split0_test_score", "split1_test_score", "split2_test_score"]
    scores = cv.cell_scores_.reshape(3, 6).T
    np.testing.assert_allclose(res.cv_results_["mean_test_score"], scores.mean(axis=1), rtol=1e-14)
    assert res.best_index_ == int(np.argmax(scores.mean(axis=1))) and res.proven_optimal_ is False
    a, e = divmod(res.best_index_, 2)
    np.testing.assert_array_equal(res.coef_, cv.full_.coefs_[a, e])
    assert res.intercept_ == cv.full_.intercepts_[a, e]
    np.testing.assert_array_equal(res.predict(X[:4]), X[:4] @ res.coef_ + res.intercept_)
    one = cv.search(opt_selection_method="one_std_score")
    want = select_best_index_onestd(_format_results(res.cv_results_["params"], scores, np.zeros_like(scores)))
    assert one.best_index_ == want
    np.testing.assert_array_equal(one.coef_, cv.full_.coefs_[divmod(want, 2)])
    # one launch per round, whatever the number of folds; the counts of every problem bound the winners'
    for got in (cv, five):
        info = got.solver_info_
        assert info["launches"] == info["rounds"] == got.full_.rounds_ and 1 <= info["rounds"] <= 3
        assert info["max_sweeps"] >= info["winner_max_sweeps"] >= 1 and info["max_swaps"] >= info["winner_max_swaps"] >= 0
        assert info["proven_optimal"] is False
    assert five.solver_info_["problems"] == 6 * 6 * 4 and cv.solver_info_["problems"] == 4 * 6 * 4 or cv.solver_info_["rounds"] == 1
    np.testing.assert_array_equal(five.full_.supports_, cv.full_.supports_)
