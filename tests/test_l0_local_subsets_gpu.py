"""Local subsets on the GPU (``slm_solve_l0_local_subsets``, ``l0_local_kernel<true>`` of csrc/l0_local_kernels.hpp),
``l0_local_subsets`` and ``l0_local_subsets_cv``.

The comparison, per (row set, cell), is against the numpy restatement of the rule (tests/_l0_local_subsets_reference.py) run
on the weighted rows directly (tests/_l0_local_subsets_cases.py).  Under the premise -- status 0 and every decision margin of
every start's run >= 1e-6, recomputed on the CPU by tests/test_l0_local_subsets_cpu.py -- the engine must give: for EVERY
problem (losing starts included) the restatement's accepted swaps, grows, drops and non-zeros; the winner's support; the
winning start where the runner-up's Q is not within 1e-6 of it (where it is, the tied starts hold one support and only the
index is left open); the polished Q to 1e-10; the certificate ``is_subset_inescapable`` at 1e-8; intercepts to 1e-9 relative to
max |y|.  A case whose premise fails is skipped; none of the committed ones does."""

import os
import warnings

import numpy as np
import pytest
from sklearn.exceptions import ConvergenceWarning
from sklearn.model_selection import ParameterGrid

from _l0_local_reference import gram, hard_law
from _l0_local_subsets_cases import NAMES, case, reference, row_sets
from _l0_local_subsets_reference import best_subset, is_subset_inescapable

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MARGIN_MIN, OBJ_RTOL, CERT_TOL = 1e-6, 1e-10, 1e-8


def engine_cells(c, binding=None, sizes=None, etas=None, starts="case"):
    from sparselm_amd import _engine

    X, y = c["X"], c["y"]
    weights, n_effs, n = row_sets(c)
    Xd = np.hstack([X, np.ones((n, 1))]) if c["intercept"] else X
    st = c["starts"] if isinstance(starts, str) else starts
    if st is not None:
        st = np.broadcast_to(st, (len(weights),) + st.shape)
    with _engine.get_engine().dataset(Xd, y) as ds:
        return ds.solve_l0_local_subsets(weights, n_effs, c["sizes"] if sizes is None else sizes, c["etas"] if etas is None else etas,
                                         intercept=c["intercept"], big_M=c["big_M"], starts=st, swaps=c["swaps"], binding=binding)


def check_against(c, ref, result):
    betas, icpts, objectives, winners, stats, infos = result
    ymax = float(np.max(np.abs(c["y"])))
    for r, cells in enumerate(ref):
        for e, cell in enumerate(cells):
            k = int(c["sizes"][e])
            info = infos[r][e]
            print(f"row set {r} cell {e} (k = {k}): margin {cell['margin']:.3e} lead {cell['lead']:.3e} reference Q {cell['objective']:.12e} "
                  f"start {cell['start']} stats {cell['stats'].tolist()}; engine Q {objectives[r, e]:.12e} start {winners[r, e]} stats "
                  f"{stats[r, e].tolist()} intercept {icpts[r, e]:.12e} against {cell['intercept']:.12e}")
            assert info["converged"] and info["status"] == "fixed_point" and info["proven_optimal"] is False
            # every problem's counts: accepted swaps, status word, non-zeros, grows, drops (the sweeps are not compared: the last
            # digits of a descent decide how many it takes to fall under the tolerance)
            np.testing.assert_array_equal(stats[r, e][:, 1:], cell["stats"][:, 1:])
            assert np.all(stats[r, e][:, 0] >= 1)
            np.testing.assert_array_equal(betas[r, e] != 0.0, cell["beta"] != 0.0)
            assert np.count_nonzero(betas[r, e]) <= k
            if cell["lead"] >= MARGIN_MIN:
                assert winners[r, e] == cell["start"]
            w = stats[r, e, winners[r, e]]
            assert (w[0], w[1], w[4], w[5]) == (info["sweeps"], info["swaps"], info["grows"], info["drops"])
            scale = max(abs(cell["objective"]), np.finfo(float).tiny)
            assert abs(objectives[r, e] - cell["objective"]) <= OBJ_RTOL * scale and objectives[r, e] == info["objective"]
            assert info["objective"] <= info["descent_objective"] + OBJ_RTOL * scale  # the polish does not raise it
            assert np.all(np.abs(betas[r, e]) <= c["big_M"])
            ok, why = is_subset_inescapable(cell["H"], cell["c"], k, c["big_M"], cell["yy"], betas[r, e], CERT_TOL, swaps=c["swaps"])
            assert ok, why
            assert abs(icpts[r, e] - cell["intercept"]) <= 1e-9 * ymax


def premise(ref):
    return all(cell["status"] == 0 and cell["margin"] >= MARGIN_MIN for cells in ref for cell in cells)


# ---- 1. every case of tests/_l0_local_subsets_cases.py against the restatement ----------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_against_the_restatement(name):
    c, ref = case(name), reference(name)
    if not premise(ref):
        pytest.skip("a decision of the restatement is closer than 1e-6 to a tie")
    result = engine_cells(c)
    check_against(c, ref, result)
    R, E, p = len(c["weights"]), len(c["sizes"]), c["X"].shape[1]
    S = 1 if c["starts"] is None else c["starts"].shape[1]
    assert result[0].shape == (R, E, p) and result[4].shape == (R, E, S, 6)
    if not c["intercept"]:
        assert not result[1].any()
    # what the case is there for
    stats = result[4]
    if name == "dead_column":
        assert np.all(stats[..., 3] == 11) and not result[0][..., 5].any()
    if name == "box":
        assert np.all(np.abs(result[0]).max(axis=-1) == c["big_M"])
    if name == "greedy":
        assert not stats[..., 1].any()
    if name == "hard_swaps":
        assert np.all(stats[..., 1] >= 1)
    if name == "second_start":
        assert np.all(result[3] == 1)
    if name in ("p63", "p64", "p65", "p130"):
        assert np.all(stats[:, :-1, 1, 5] >= 1) and stats[0, 0, 1, 5] >= 8  # the large start is shrunk ...
    if name in ("p63", "p64", "p65"):
        assert stats[0, 3, 1, 4] == 2 and stats[0, 3, 1, 5] == 0              # ... and for k = 12 grown
    if name == "p1024":
        support = np.flatnonzero(result[0][0, 1])
        assert len(set(support // 64)) == 16  # a column of every 64-block: all sixteen slots


def test_both_routes_byte_for_byte():
    from sparselm_amd import _engine

    if _engine.load_binding() is None:
        pytest.fail("the compiled binding is not built")
    for name in ("p65", "intercept"):
        a, b = engine_cells(case(name), binding=False), engine_cells(case(name), binding=True)
        assert a[0].any()
        for x, y in zip(a[:5], b[:5]):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        assert a[5] == b[5]


def test_more_problems_than_one_grid_pass_on_sixteen_row_sets():
    """130 cells (the two of the case, repeated) x 16 row sets = 2080 problems: more than the 2 x CUs workgroups of four waves
    that one pass of the grid holds at 256 CUs.  Equal cells of one row set give equal bytes wherever they sit."""
    from sparselm_amd import _engine

    c, ref = case("sixteen_sets"), reference("sixteen_sets")
    cus = int(_engine.get_engine().device_info()["compute_units"])
    cells = 130
    assert 16 * cells > 2 * cus * 4 or cus > 256
    sizes = np.asarray(c["sizes"])[np.arange(cells) % 2]
    betas, icpts, objectives, winners, stats, infos = engine_cells(c, sizes=sizes, etas=np.zeros(cells))
    assert betas.shape == (16, cells, 6) and stats.shape == (16, cells, 1, 6) and not winners.any()
    for r in range(16):
        for e in range(cells):
            cell = ref[r][e % 2]
            assert cell["status"] == 0 and cell["margin"] >= MARGIN_MIN
            assert np.array_equal(betas[r, e] != 0.0, cell["beta"] != 0.0), (r, e)
            assert abs(objectives[r, e] - cell["objective"]) <= OBJ_RTOL * abs(cell["objective"]), (r, e)
            if e >= 2:
                assert betas[r, e].tobytes() == betas[r, e % 2].tobytes() and objectives[r, e] == objectives[r, e % 2], (r, e)
                assert np.array_equal(stats[r, e], stats[r, e % 2]) and icpts[r, e] == icpts[r, e % 2], (r, e)


# ---- 2. every refusal, by both routes ---------------------------------------------------------------------------------------------
def test_every_refusal_by_both_routes():
    from sparselm_amd import _engine

    c = case("p65")
    X, y = c["X"], c["y"]
    ones = np.ones(40)
    starts = np.full((1, 1, 1, 65), 0.25)
    with _engine.get_engine().dataset(X, y) as ds:
        for route in (False, True):
            for bad, words in ((dict(sizes=[2, 0]), r"sizes\[1\] must be >= 1"), (dict(sizes=[-3]), r"sizes\[0\]"),
                               (dict(sizes=[2], etas=[np.nan]), "etas"), (dict(sizes=[2], etas=[-0.5]), "etas"),
                               (dict(sizes=[0], etas=[-0.5]), "sizes"),  # (the size is named first)
                               (dict(sizes=[2], big_M=-1.0), "big_M"), (dict(sizes=[2], n_cells=0), "n_cells"),
                               (dict(sizes=[2], n_starts=0), "n_starts"), (dict(sizes=np.full(8193, 2)), r"count \* n_cells \* n_starts"),
                               (dict(sizes=[2], big_M=0.1, starts=starts), "box")):
                with pytest.raises(ValueError, match=words):
                    ds.solve_l0_local_subsets([None], [0], binding=route, **bad)
            with pytest.raises(ValueError, match=r"count \* n_cells \* n_starts must be at most 8192 problems \(got 3 x 2731 x 1\)"):
                ds.solve_l0_local_subsets([None, ones, None], [0, 40, 0], np.full(2731, 2), binding=route)
            for count in (0, 17):
                with pytest.raises(ValueError, match="count must be 1 .. 16"):
                    ds.solve_l0_local_subsets([None] * count, [0] * count, [2], binding=route)
            for value in (-1.0, np.nan, np.inf):
                w = ones.copy()
                w[7] = value
                with pytest.raises(ValueError, match=r"row_weights\[1\]\[7\]"):
                    ds.solve_l0_local_subsets([None, w], [0, 40], [2], binding=route)
        # NULL sizes or etas: the ctypes route hands them over as they are
        with pytest.raises(ValueError, match="NULL"):
            ds.solve_l0_local_subsets([None], [0], None, [0.0])
        with pytest.raises(ValueError, match="NULL"):
            ds.solve_l0_local_subsets([None], [0], [2], None)
        ds.set_groups(np.r_[np.arange(64), 63], 64)  # the last column shares its group
        for route in (False, True):
            with pytest.raises(ValueError, match="the last column must be alone"):
                ds.solve_l0_local_subsets([None], [0], [2], intercept=True, binding=route)
            with pytest.raises(NotImplementedError, match="groups"):
                ds.solve_l0_local_subsets([None], [0], [2], binding=route)
    wide = np.random.default_rng(0).standard_normal((8, 1026))
    with _engine.get_engine().dataset(wide, np.ones(8)) as ds:
        for route in (False, True):
            with pytest.raises(NotImplementedError, match="up to 1024 columns beside the intercept's"):
                ds.solve_l0_local_subsets([None], [0], [2], intercept=True, binding=route)
    Z = X.copy()
    Z[:, -1] = 0.0
    with _engine.get_engine().dataset(Z, y) as ds:
        for route in (False, True):
            with pytest.raises(ValueError, match="row set 0 gives the last column no weight"):
                ds.solve_l0_local_subsets([None, ones], [0, 40], [2], intercept=True, binding=route)


# ---- 3. against the exact side ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.0, 0.05])
def test_never_below_and_where_the_restatement_hits_it_equal_to_the_proven_optimum(eta):
    """The hard law (p = 14): (seed, k) of ``SWAPS_REACH_OPTIMUM`` are cases where the restatement's zero start is at the
    optimum with eta = 0; with a ridge term the enumeration says where Q must be equal."""
    from sparselm_amd.miqp import BestSubsetSelection, RidgedBestSubsetSelection, l0_local_subsets

    for seed, sizes in ((20, [2, 4, 5]), (2, [3, 4]), (16, [2, 3])):
        X, y = hard_law(seed)
        res = l0_local_subsets(X, y, sizes=sizes, etas=[eta], max_rounds=0)
        G, c, _, _, _ = gram(X, y)
        for i, k in enumerate(sizes):
            est = (RidgedBestSubsetSelection(sparse_bound=k, eta=eta) if eta else BestSubsetSelection(sparse_bound=k)).fit(X, y)
            assert est.solver_info_["proven_optimal"]
            exact = est.solver_info_["objective"]
            print(f"seed {seed} k {k} eta {eta}: Q {res.objectives_[i, 0]:.12e} proven {exact:.12e}")
            assert abs(exact - best_subset(G + 2.0 * eta * np.eye(14), c, k)) <= 1e-9 * abs(exact)  # the units are the same
            assert res.objectives_[i, 0] >= exact - 1e-9 * abs(exact)
            assert res.supports_[i, 0].sum() <= k and res.proven_optimal_ is False
            if eta == 0.0 and seed in (20, 16):
                assert abs(res.objectives_[i, 0] - exact) <= 1e-9 * abs(exact)
                np.testing.assert_array_equal(res.supports_[i, 0], est.coef_ != 0.0)


def test_the_reference_data_against_the_wide_profile():
    from sparselm_amd.miqp import l0_local_subsets, l0_profile

    X = np.load(os.path.join(ROOT, "tests", "golden", "reference_examples", "corr.npy"))
    y = np.load(os.path.join(ROOT, "tests", "golden", "reference_examples", "energy.npy"))
    assert X.shape == (290, 66)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        prof = l0_profile(X, y, max_groups=3, big_M=1000, solver_options={"wide": True})
    res = l0_local_subsets(X, y, sizes=[1, 2, 3], big_M=1000)
    assert prof.proven_optimal_  # K = 3 of 66 columns: the search ends
    for i, k in enumerate((1, 2, 3)):
        exact = float(np.min(prof.values_[: k + 1]))
        print(f"290 x 66, k = {k}: Q {res.objectives_[i, 0]:.12e} proven {exact:.12e}")
        assert res.objectives_[i, 0] >= exact - 1e-9 * abs(exact)
    assert abs(res.objectives_[0, 0] - prof.values_[1]) <= 1e-9 * abs(prof.values_[1])  # one column: the arg-max of the gains IS the optimum


# ---- 4. the rounds, the cross-validation --------------------------------------------------------------------------------------------
def test_rounds_never_raise_an_objective_and_the_fixed_point_is_monotone_in_k():
    from sparselm_amd.miqp import l0_local_subsets

    X, y = hard_law(9)
    sizes = list(range(1, 9))
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        one = l0_local_subsets(X, y, sizes=sizes, etas=[0.0, 0.05], max_rounds=0)
        res = l0_local_subsets(X, y, sizes=sizes, etas=[0.0, 0.05], max_rounds=20)
    assert one.rounds_ == 1 and res.round_objectives_.shape == (res.rounds_, 8, 2) and 2 <= res.rounds_ <= 20
    np.testing.assert_array_equal(res.round_objectives_[0], one.objectives_)
    np.testing.assert_array_equal(res.round_objectives_[-1], res.objectives_)
    assert np.all(np.diff(res.round_objectives_, axis=0) <= 0.0)
    assert res.rounds_ == 2 or np.any(res.round_objectives_[-2] != res.round_objectives_[0])  # a chain improved something, or nothing could
    assert np.array_equal(res.round_objectives_[-1], res.round_objectives_[-2])                # it ended because no cell improved
    assert np.all(np.diff(res.objectives_, axis=0) <= 1e-12 * np.abs(res.objectives_[:-1]))    # non-increasing in k for each eta
    assert np.all(res.supports_.sum(axis=2) <= np.array(sizes)[:, None]) and res.converged_.all()
    G, c, _, _, _ = gram(X, y)
    for i, k in enumerate(sizes[:5]):
        exact = best_subset(G, c, k)
        assert res.objectives_[i, 0] >= exact - 1e-9 * abs(exact)
    for name in ("swaps_", "sweeps_", "grows_", "drops_", "losses_", "intercepts_"):
        assert getattr(res, name).shape == (8, 2)
    np.testing.assert_allclose(res.losses_[:, 0], [np.mean((y - res.predict(X, i)) ** 2) / 2 for i in range(8)], rtol=1e-9)


@pytest.mark.parametrize("intercept", [False, True])
def test_l0_local_subsets_cv_end_to_end(intercept):
    from sparselm_amd.miqp import l0_local_subsets, l0_local_subsets_cv

    c = case("p65")
    X, y = (c["X"] + 1.0, c["y"] + 2.0) if intercept else (c["X"], c["y"])
    sizes, etas = [1, 2, 4], [0.0, 0.02]
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        cv = l0_local_subsets_cv(X, y, sizes=sizes, etas=etas, cv=3, fit_intercept=intercept)
        five = l0_local_subsets_cv(X, y, sizes=sizes, etas=etas, cv=5, fit_intercept=intercept)
    assert len(cv.paths_) == 3 and cv.cell_scores_.shape == (3, 3, 2) and cv.proven_optimal_ is False
    for path, rows in [(cv.paths_[f], tr) for f, (tr, _) in enumerate(cv.splits_)] + [(cv.full_, np.arange(40))]:
        alone = l0_local_subsets(X[rows], y[rows], sizes=sizes, etas=etas, fit_intercept=intercept)
        np.testing.assert_array_equal(path.supports_, alone.supports_)
        assert np.all(np.abs(path.objectives_ - alone.objectives_) <= OBJ_RTOL * np.abs(alone.objectives_))
        assert np.all(np.abs(path.intercepts_ - alone.intercepts_) <= 1e-9 * np.max(np.abs(y)))
        assert path.converged_.all() and path.round_objectives_.shape == (cv.solver_info_["rounds"], 3, 2)
        assert np.all(np.diff(path.round_objectives_, axis=0) <= 0.0)
        if not intercept:
            assert not path.intercepts_.any()
    for f, (_, te) in enumerate(cv.splits_):
        for a in range(3):
            for e in range(2):
                resid = y[te] - cv.paths_[f].predict(X[te], a, e)
                assert cv.cell_scores_[f, a, e] == pytest.approx(-np.sqrt(np.mean(resid**2)), rel=1e-12)
    res = cv.search()
    assert res.cv_results_["params"] == list(ParameterGrid({"sparse_bound": sizes, "eta": etas}))
    scores = cv.cell_scores_.transpose(0, 2, 1).reshape(3, 6).T
    np.testing.assert_allclose(res.cv_results_["mean_test_score"], scores.mean(axis=1), rtol=1e-14)
    assert res.best_index_ == int(np.argmax(scores.mean(axis=1))) and res.proven_optimal_ is False
    e, k = divmod(res.best_index_, 3)
    np.testing.assert_array_equal(res.coef_, cv.full_.coefs_[k, e])
    assert res.intercept_ == cv.full_.intercepts_[k, e]
    # one launch per round, whatever the number of folds
    for got in (cv, five):
        info = got.solver_info_
        assert info["launches"] == info["rounds"] == got.full_.rounds_ and 1 <= info["rounds"] <= 3 and info["proven_optimal"] is False
    assert cv.solver_info_["problems"] in (4 * 6, 4 * 6 * 4) and five.solver_info_["problems"] in (6 * 6, 6 * 6 * 4)
