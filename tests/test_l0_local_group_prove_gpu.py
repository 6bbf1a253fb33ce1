"""The local proof with groups on the GPU (``slm_solve_l0_local_group_nodes``, ``slm_solve_l0_local_group_prove``;
``l0_local_group_node_kernel`` in csrc/l0_local_group_node_kernels.hpp).

1. The group node kernel equals the rule: on the device's own Gram (downloaded) ``u``, sweeps, status, lower, primal and upper of
   every node of every shared batch equal the numpy restatement BIT FOR BIT -- the restatement that
   tests/test_l0_local_group_prove_cpu.py shows to equal the host twin bit for bit -- at 2, 63, 64, 65, 130 and 1024 columns, with
   groups that straddle lanes 63 / 64, one group of 70 columns and a rank-deficient 12 x 20 design in groups of four; and the
   bound agrees with ``node_lower_bound`` by plain numpy products at the kernel's own ``u``.
2. The group hard law: proven at the brute-force optimum, with ``nodes_``, ``rounds_``, bounds and coefficients equal to the
   restatement's tree exactly.  3. Singleton groups without a hierarchy equal ``l0_local_prove`` field for field.  4. The committed
   290 x 66 data in 22 groups of three under a chain at eta = 0.01 against the exact grouped estimator.  5. A 120 x 160 draw in
   40 groups of four whose certificate numpy checks.  6. ``max_nodes = 3``, an intercept, weights, ``path=``, ``big_M = 0``, ``alpha = 0``."""

import os
import warnings

import numpy as np
import pytest
from sklearn.exceptions import ConvergenceWarning

from _l0_local_bound_reference import certificate_tolerance
from _l0_local_group_prove_cases import cases, run_rule
from _l0_local_group_prove_reference import brute_force, group_words, node_lower_bound, objective, tree
from _l0_local_groups_reference import close_hierarchy, group_law

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REL_GAP = 1e-6
ALPHAS, ETAS, BIG_M = (1e-3, 0.1, 0.5), (0.0, 0.02, 1.0), 100.0


def gid_of(gstart):
    return np.repeat(np.arange(len(gstart) - 1), np.diff(gstart))


def chain(ng):
    return [[]] + [[g - 1] for g in range(1, ng)]


# ---- 1. the group node kernel equals the rule -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases()))
def test_the_group_node_kernel_equals_the_rule(name):
    from sparselm_amd import _engine

    k = cases()[name]
    p, gstart = k["X"].shape[1], k["gstart"]
    ng = len(gstart) - 1
    closed = close_hierarchy(ng, k["need"])
    cell = [n[0] for n in k["nodes"]]
    in_words = np.stack([group_words(n[1]) for n in k["nodes"]])
    out_words = np.stack([group_words(n[2]) for n in k["nodes"]])
    parent = np.array([n[3] for n in k["nodes"]])
    starts = np.stack([np.zeros(p) if n[4] is None else n[4] for n in k["nodes"]])  # (a zero start is no start)
    with _engine.get_engine().dataset(k["X"], k["y"]) as ds:
        ds.set_groups(gid_of(gstart), ng)
        lower, primal, upper, u, stats, rc = ds.solve_l0_local_group_nodes(k["alphas"], k["etas"], cell, in_words, out_words, need=k["need"],
                                                                           big_M=k["big_M"], parent_lower=parent, starts=starts,
                                                                           max_sweeps=k["max_sweeps"], gap_tol=k["gap_tol"])
        G, c, _ = ds.covariance_download(0)
    ref = run_rule(G, c, k)  # the rule on the device's own Gram
    for i, ((ce, gin, gout, par, _), run) in enumerate(zip(k["nodes"], ref)):
        alpha, eta = float(k["alphas"][ce]), float(k["etas"][ce])
        print(f"{name} node {i}: cell {ce} IN {int(gin.sum())} OUT {int(gout.sum())}: rule sweeps {run['sweeps']} status {run['status']} lower "
              f"{run['lower']:.15e} upper {run['upper']:.15e}; kernel sweeps {stats[i, 0]} status {stats[i, 1]} lower {lower[i]:.15e} upper "
              f"{upper[i]:.15e} max |u - u_rule| {np.max(np.abs(u[i] - run['u'])):.2e}")
        assert stats[i, 0] == run["sweeps"] and stats[i, 1] == run["status"]
        np.testing.assert_array_equal(u[i], run["u"])  # change for change: the same bits
        assert lower[i] == run["lower"] and primal[i] == run["primal"] and upper[i] == run["upper"]
        # the certificate at the kernel's own u, by plain numpy products
        at_u = max(node_lower_bound(G, c, alpha, eta, k["big_M"], gstart, gin, gout, u[i]),
                   node_lower_bound(G, c, alpha, eta, k["big_M"], gstart, gin, gout, np.zeros(p)), par)
        assert abs(lower[i] - at_u) <= certificate_tolerance(G, alpha, u[i], lower[i])
        assert abs(upper[i] - objective(G, c, alpha, eta, u[i], gstart, closed)) <= certificate_tolerance(G, alpha, u[i], upper[i])
        assert np.all(np.abs(u[i]) <= k["big_M"]) and not u[i][np.repeat(gout, np.diff(gstart))].any()
    assert rc == (_engine.SLM_ERR_NOT_CONVERGED if stats[:, 1].any() else _engine.SLM_OK)  # (with every output valid either way)
    if name.startswith("rank_deficient"):
        assert G[7, 7] == 0.0 and not u[:, 7].any()  # a failed pivot inside an IN group: u stays 0, its h(c_7) is counted (above)
    if name == "one_sweep":
        assert (stats[:, 0] == 1).all()


# ---- 2. the group hard law ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chained", [False, True])
@pytest.mark.parametrize("seed", range(3))
def test_the_hard_law_is_proven_and_the_tree_is_the_restatements(seed, chained):
    """``l0_local_group_prove`` as it is called -- width 32, the incumbents of an ``L0LocalGroupPath`` -- against brute force and
    against the restatement's tree with the path's coefficients as its incumbents on the device's own Gram.  A sweep cap of 25
    keeps the restatement quick; an unclosed node's bound is valid and is split further, on both sides alike."""
    from sparselm_amd import _engine
    from sparselm_amd.miqp import l0_local_group_prove, l0_local_group_search

    X, y, gstart = group_law(seed)
    ng = len(gstart) - 1
    need = chain(ng) if chained else None
    closed = close_hierarchy(ng, need)
    cells = [(alpha, eta) for alpha in ALPHAS for eta in ETAS]
    with _engine.get_engine().dataset(X, y) as ds:
        ds.covariance()
        G, c, _ = ds.covariance_download(0)
    path = l0_local_group_search(X, y, alphas=ALPHAS, etas=ETAS, groups=gid_of(gstart), hierarchy=need, big_M=BIG_M)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        res = l0_local_group_prove(X, y, alphas=ALPHAS, etas=ETAS, groups=gid_of(gstart), hierarchy=need, big_M=BIG_M, path=path, rel_gap=REL_GAP,
                                   max_nodes=400, max_sweeps=25)
    ref, launches = tree(G, c, cells, BIG_M, gstart, need=need, incumbents=path.coefs_.reshape(9, -1), rel_gap=REL_GAP, max_nodes=400, width=32,
                         max_sweeps=25)
    print(f"seed {seed} chain {chained}: nodes {res.nodes_.ravel().tolist()} rounds {res.rounds_.ravel().tolist()} launches {launches}")
    assert res.nodes_.ravel().tolist() == [cell["nodes"] for cell in ref] and res.rounds_.ravel().tolist() == [cell["rounds"] for cell in ref]
    assert (res.status_.ravel() == "optimal").tolist() == [cell["status"] == 0 for cell in ref]
    np.testing.assert_array_equal(res.objectives_.ravel(), [cell["objective"] for cell in ref])
    np.testing.assert_array_equal(res.lower_bounds_.ravel(), [cell["lower_bound"] for cell in ref])
    np.testing.assert_array_equal(res.coefs_.reshape(9, -1), np.array([cell["beta"] for cell in ref]))
    for a, alpha in enumerate(ALPHAS):
        for e, eta in enumerate(ETAS):
            best = brute_force(G, c, alpha, eta, BIG_M, gstart, closed)
            scale = max(abs(best), alpha)
            print(f"  alpha {alpha} eta {eta}: F* {best:.9e} proof {res.objectives_[a, e]:.9e} bound {res.lower_bounds_[a, e]:.9e} search "
                  f"{path.objectives_[a, e]:.9e} nodes {res.nodes_[a, e]} {res.status_[a, e]}")
            assert res.lower_bounds_[a, e] <= best + 1e-9 * scale and res.objectives_[a, e] >= best - 1e-9 * scale
            if eta > 0.0:  # (eta = 0 under the loose box need only report an honest gap)
                assert res.proven_optimal_[a, e] and abs(res.objectives_[a, e] - best) <= 2.0 * REL_GAP * scale and res.gaps_[a, e] <= REL_GAP
            assert res.n_active_groups_[a, e] == np.count_nonzero(res.group_supports_[a, e])
            assert abs(objective(G, c, alpha, eta, res.coefs_[a, e], gstart, closed) - res.objectives_[a, e]) <= 1e-10 * scale


# ---- 3. singleton groups, no hierarchy: l0_local_prove ---------------------------------------------------------------------------------
def test_singleton_groups_equal_the_column_proof_field_for_field():
    from _l0_local_bound_reference import hard_problem
    from sparselm_amd.miqp import l0_local_group_prove, l0_local_group_search, l0_local_prove, l0_local_search

    X, y, _, _ = hard_problem(1)
    for M in (0.7, 100.0):
        col_path = l0_local_search(X, y, alphas=ALPHAS, etas=ETAS, big_M=M)
        grp_path = l0_local_group_search(X, y, alphas=ALPHAS, etas=ETAS, big_M=M)
        grp_path.coefs_, grp_path.group_supports_ = col_path.coefs_, col_path.coefs_ != 0.0  # the same incumbents under the group path's type
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", ConvergenceWarning)
            col = l0_local_prove(X, y, alphas=ALPHAS, etas=ETAS, big_M=M, path=col_path, max_nodes=4096, max_sweeps=60, return_certificate=True)
            grp = l0_local_group_prove(X, y, alphas=ALPHAS, etas=ETAS, big_M=M, path=grp_path, max_nodes=4096, max_sweeps=60, return_certificate=True)
        for field in ("coefs_", "intercepts_", "objectives_", "lower_bounds_", "gaps_", "nodes_", "rounds_", "status_", "proven_optimal_"):
            np.testing.assert_array_equal(getattr(grp, field), getattr(col, field), err_msg=field)
        for key in ("cell", "in_", "out_", "u", "lower"):
            np.testing.assert_array_equal(grp.certificate_[key], col.certificate_[key], err_msg=key)
        np.testing.assert_array_equal(grp.group_supports_, grp.coefs_ != 0.0)


# ---- 4. the committed data against the exact grouped estimator ---------------------------------------------------------------------------
def test_the_reference_data_in_groups_of_three_under_a_chain():
    """290 x 66 in 22 groups of three, group g needing g - 1, at eta = 0.01: the exact search with the same groups and hierarchy
    (``L2L0``, which is ``RegularizedL0`` with the ridge term; wide, 66 columns) says what the optimum is."""
    from sparselm_amd.miqp import L2L0, l0_local_group_prove

    X = np.load(os.path.join(ROOT, "tests", "golden", "reference_examples", "corr.npy"))
    y = np.load(os.path.join(ROOT, "tests", "golden", "reference_examples", "energy.npy"))
    assert X.shape == (290, 66)
    groups, hierarchy = np.arange(66) // 3, chain(22)
    alphas, eta = np.array([0.01, 0.1]) * float(np.var(y)), 0.01
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        res = l0_local_group_prove(X, y, alphas=alphas, etas=[eta], groups=groups, hierarchy=hierarchy, big_M=100, fit_intercept=True,
                                   rel_gap=REL_GAP, max_nodes=4000)
    for a, alpha in enumerate(alphas):
        est = L2L0(groups=groups, alpha=alpha, eta=eta, hierarchy=hierarchy, big_M=100, fit_intercept=True, solver_options={"wide": True})
        with warnings.catch_warnings():
            warnings.simplefilter("error", ConvergenceWarning)
            est.fit(X, y)
        exact = est.solver_info_["objective"]
        print(f"290 x 66 grouped alpha {alpha:.4g}: proof {res.objectives_[a, 0]:.10e} exact {exact:.10e} bound {res.lower_bounds_[a, 0]:.10e} nodes "
              f"{res.nodes_[a, 0]} rounds {res.rounds_[a, 0]} {res.status_[a, 0]}")
        assert est.solver_info_["proven_optimal"]
        scale = max(abs(exact), alpha)
        assert res.lower_bounds_[a, 0] <= exact + 1e-9 * scale and res.objectives_[a, 0] >= exact - 1e-9 * scale
        assert res.proven_optimal_[a, 0] and abs(res.objectives_[a, 0] - exact) <= 2.0 * REL_GAP * scale
        np.testing.assert_array_equal(res.group_supports_[a, 0], est.active_groups_)
        assert abs(res.intercepts_[a, 0] - est.intercept_) <= 1e-6 * max(1.0, abs(est.intercept_))


# ---- 5. wider than any exact entry ---------------------------------------------------------------------------------------------------
def grouped_draw():
    """120 x 160 in 40 groups of four: AR(1) 0.5 columns, 3 true groups, SNR 4, default_rng(0)."""
    rng = np.random.default_rng(0)
    n, p = 120, 160
    Z = rng.standard_normal((n, p))
    X = Z.copy()
    for j in range(1, p):
        X[:, j] = 0.5 * X[:, j - 1] + np.sqrt(0.75) * Z[:, j]
    beta = np.zeros(p)
    for g in rng.choice(40, 3, replace=False):
        beta[4 * g:4 * g + 4] = (-1.0) ** np.arange(4)
    signal = X @ beta
    y = signal + np.sqrt(np.var(signal) / 4.0) * rng.standard_normal(n)
    return X, y


def test_a_grouped_proof_at_160_columns_with_a_certificate_numpy_checks():
    from sparselm_amd import _engine
    from sparselm_amd.miqp import l0_local_group_prove, l0_local_group_search

    X, y = grouped_draw()
    yy = float(y @ y) / len(y)
    groups, gstart = np.arange(160) // 4, np.arange(0, 161, 4)
    closed = close_hierarchy(40, None)
    alphas, eta, M = np.array([0.01, 0.05, 0.2]) * yy, 0.1, 100.0
    path = l0_local_group_search(X, y, alphas=alphas, etas=[eta], groups=groups, big_M=M)
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        res = l0_local_group_prove(X, y, alphas=alphas, etas=[eta], groups=groups, big_M=M, rel_gap=REL_GAP, max_nodes=4000, return_certificate=True)
    with _engine.get_engine().dataset(X, y) as ds:
        ds.covariance()
        G, c, _ = ds.covariance_download(0)
    cert = res.certificate_
    print(f"120 x 160 grouped: nodes {res.nodes_[:, 0].tolist()} rounds {res.rounds_[:, 0].tolist()} leaves {len(cert['lower'])} gaps {res.gaps_[:, 0]}")
    assert res.proven_optimal_.all() and cert["in_"].shape[1] == 40
    for a, alpha in enumerate(alphas):
        best = res.objectives_[a, 0]
        scale = max(abs(best), alpha)
        assert res.lower_bounds_[a, 0] <= best <= path.objectives_[a, 0] + 1e-12 * scale
        assert abs(objective(G, c, alpha, eta, res.coefs_[a, 0], gstart, closed) - best) <= 1e-10 * scale
        mine = (cert["cell"][:, 0] == a) & (cert["cell"][:, 1] == 0)
        gin, gout = cert["in_"][mine], cert["out_"][mine]
        # without a hierarchy the leaves partition all group supports: their 2^-depth sum to 1 and no two overlap
        depth = gin.sum(axis=1) + gout.sum(axis=1)
        apart = (gin.astype(int) @ gout.T.astype(int) + gout.astype(int) @ gin.T.astype(int)) > 0
        assert float(np.sum(np.ldexp(1.0, -depth))) == 1.0 and int((~apart).sum()) == int(mine.sum())
        assert 2 * int(mine.sum()) - 1 == res.nodes_[a, 0]
        cut = best - REL_GAP * scale
        for lf_in, lf_out, u, lower in zip(gin, gout, cert["u"][mine], cert["lower"][mine]):
            at_u = max(node_lower_bound(G, c, alpha, eta, M, gstart, lf_in, lf_out, u),
                       node_lower_bound(G, c, alpha, eta, M, gstart, lf_in, lf_out, np.zeros(160)))
            assert at_u >= cut - certificate_tolerance(G, alpha, u, cut)
            assert lower >= cut


# ---- 6. the node limit and the surface ----------------------------------------------------------------------------------------------------
def test_the_node_limit_an_intercept_weights_a_given_path_and_the_edges():
    from sparselm_amd import _engine
    from sparselm_amd.miqp import L0LocalGroupProof, l0_local_group_prove, l0_local_group_search

    X, y, gstart = group_law(1)
    groups, need = gid_of(gstart), chain(7)
    y = y + 3.0
    w = np.random.default_rng(2).uniform(0.5, 2.0, len(y))
    alphas, etas = [0.0, 0.05], [0.01]
    kw = dict(alphas=alphas, etas=etas, groups=groups, hierarchy=need, big_M=100, fit_intercept=True, sample_weight=w)
    path = l0_local_group_search(X, y, **kw)
    given = l0_local_group_prove(X, y, path=path, max_nodes=4096, **kw)
    own = l0_local_group_prove(X, y, max_nodes=4096, **kw)
    assert isinstance(given, L0LocalGroupProof) and given.proven_optimal_.all() and own.proven_optimal_.all()
    np.testing.assert_array_equal(given.objectives_, own.objectives_)  # path=None runs the same search on the same handle
    np.testing.assert_array_equal(given.nodes_, own.nodes_)
    assert (given.objectives_ <= path.objectives_ + 1e-12).all() and (given.lower_bounds_ <= given.objectives_).all()
    assert given.coefs_.shape == (2, 1, 14) and given.group_supports_.shape == (2, 1, 7)
    # alpha = 0: nothing is paid for a group, the ridge regression on all columns is the optimum
    wn = w / w.sum()
    xm, ym = wn @ X, wn @ y
    Xc, yc = X - xm, y - ym
    G, c = Xc.T @ (wn[:, None] * Xc), Xc.T @ (wn * yc)
    b = np.linalg.solve(G + 0.02 * np.eye(14), c)
    exact = 0.5 * b @ (G + 0.02 * np.eye(14)) @ b - c @ b
    assert abs(given.objectives_[0, 0] - exact) <= 2.0 * REL_GAP * abs(exact)
    assert abs(given.intercepts_[0, 0] - (ym - xm @ given.coefs_[0, 0])) <= 1e-9
    # the columns in another order: the caller's order comes back
    order = np.random.default_rng(3).permutation(14)
    mixed = l0_local_group_prove(X[:, order], y, max_nodes=4096, **dict(kw, groups=groups[order]))
    np.testing.assert_array_equal(mixed.coefs_ != 0.0, given.coefs_[..., order] != 0.0)
    np.testing.assert_allclose(mixed.objectives_, given.objectives_, rtol=1e-9, atol=1e-12)
    # a node limit of 3: a proven bound all the same
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        short = l0_local_group_prove(X, y, alphas=ALPHAS, etas=[0.0], groups=groups, hierarchy=need, big_M=100, max_nodes=3)
        full = l0_local_group_prove(X, y, alphas=ALPHAS, etas=[0.0], groups=groups, hierarchy=need, big_M=100, max_nodes=4096)
    assert (short.nodes_ <= 3).all() and np.array_equal(short.status_ == "node_limit", ~short.proven_optimal_)
    assert (short.lower_bounds_ <= full.objectives_ + 1e-9).all() and (short.objectives_ >= full.lower_bounds_ - 1e-9).all()
    assert (~short.proven_optimal_).any() == any(issubclass(s.category, ConvergenceWarning) for s in seen)
    # big_M = 0: no launch, everything zero, proven
    zero = l0_local_group_prove(X, y, alphas=[0.1], groups=groups, hierarchy=need, big_M=0)
    assert zero.proven_optimal_.all() and not zero.coefs_.any() and zero.objectives_[0, 0] == 0.0 and zero.lower_bounds_[0, 0] == 0.0
    assert zero.nodes_[0, 0] == 0 and zero.rounds_[0, 0] == 0 and not zero.group_supports_.any()
    # the engine refuses by class: masks that are not closed, a group beyond the groups, groups out of order
    none = np.zeros((1, 16), dtype=np.uint64)
    with _engine.get_engine().dataset(X, y) as ds:
        ds.set_groups(groups, 7)
        top = none.copy()
        top[0, 0] = 1 << 6
        with pytest.raises(ValueError, match="is not closed under the hierarchy"):
            ds.solve_l0_local_group_nodes([0.1], [0.0], [0], top, none, need=need)
        far = none.copy()
        far[0, 0] = 1 << 7
        with pytest.raises(ValueError, match="fixes a group beyond the 7 groups"):
            ds.solve_l0_local_group_nodes([0.1], [0.0], [0], far, none, need=need)
        with pytest.raises(ValueError, match="both IN and OUT"):
            ds.solve_l0_local_group_nodes([0.1], [0.0], [0], top, top, need=need)
        with pytest.raises(ValueError, match="rel_gap must lie in"):
            ds.solve_l0_local_group_prove([0.1], need=need, rel_gap=2.0)
        ds.set_groups(np.arange(14) % 7, 7)
        with pytest.raises(NotImplementedError, match="contiguous and ascending"):
            ds.solve_l0_local_group_prove([0.1])
