"""The local proof on the GPU (``slm_solve_l0_local_nodes``, ``slm_solve_l0_local_prove``; ``l0_local_node_kernel`` in
csrc/l0_local_node_kernels.hpp).

1. The node kernel equals the host twin: on the device's own Gram (downloaded) ``u``, sweeps, status, lower, primal and upper of
   every node of every shared batch equal the numpy restatement of the rule BIT FOR BIT -- the restatement that
   tests/test_l0_local_prove_cpu.py shows to equal the host twin bit for bit -- and the bound agrees with ``node_lower_bound`` by
   plain numpy products at the kernel's own ``u``.
2. ``l0_local_prove`` on the hard law's 54 cells: proven optimal at the brute-force optimum; ``nodes_``, ``rounds_``, the
   coefficients and the bounds equal the restatement's tree run on the device's Gram, exactly.
3. The committed 290 x 66 data against the exact ``RegularizedL0`` / ``L2L0`` (wide).  4. A 120 x 160 draw, wider than any exact
   entry takes: proven, with a certificate that numpy alone checks.  5. A node limit of 3.  6. The surface."""

import functools
import os
import warnings

import numpy as np
import pytest
from sklearn.exceptions import ConvergenceWarning

from _l0_local_bound_reference import ALPHAS, BIG_MS, ETAS, brute_force, certificate_tolerance, hard_problem
from _l0_local_prove_cases import cases, run_rule
from _l0_local_reference import gram
from _l0_local_prove_reference import leaves_cover, node_lower_bound, objective, to_words, tree

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
REL_GAP = 1e-6


# ---- 1. the node kernel equals the host twin ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases()))
def test_the_node_kernel_equals_the_twin(name):
    from sparselm_amd import _engine

    k = cases()[name]
    p = k["X"].shape[1]
    cell = [n[0] for n in k["nodes"]]
    in_words = np.stack([to_words(n[1]) for n in k["nodes"]])
    out_words = np.stack([to_words(n[2]) for n in k["nodes"]])
    parent = np.array([n[3] for n in k["nodes"]])
    starts = np.stack([np.zeros(p) if n[4] is None else n[4] for n in k["nodes"]])  # (a zero start is no start)
    with _engine.get_engine().dataset(k["X"], k["y"]) as ds:
        lower, primal, upper, u, stats, rc = ds.solve_l0_local_nodes(k["alphas"], k["etas"], cell, in_words, out_words, big_M=k["big_M"],
                                                                     parent_lower=parent, starts=starts, max_sweeps=k["max_sweeps"],
                                                                     gap_tol=k["gap_tol"])
        G, c, _ = ds.covariance_download(0)
    ref = run_rule(G, c, k)  # the rule on the device's own Gram
    for i, ((ce, in_, out_, par, _), run) in enumerate(zip(k["nodes"], ref)):
        alpha, eta = float(k["alphas"][ce]), float(k["etas"][ce])
        print(f"{name} node {i}: cell {ce} IN {int(in_.sum())} OUT {int(out_.sum())}: rule sweeps {run['sweeps']} status {run['status']} changes "
              f"{run['changes']} lower {run['lower']:.15e} upper {run['upper']:.15e}; kernel sweeps {stats[i, 0]} status {stats[i, 1]} lower "
              f"{lower[i]:.15e} upper {upper[i]:.15e} max |u - u_rule| {np.max(np.abs(u[i] - run['u'])):.2e}")
        assert stats[i, 0] == run["sweeps"] and stats[i, 1] == run["status"]
        np.testing.assert_array_equal(u[i], run["u"])  # change for change: the same bits
        assert lower[i] == run["lower"] and primal[i] == run["primal"] and upper[i] == run["upper"]
        # the certificate at the kernel's own u, by plain numpy products
        at_u = max(node_lower_bound(G, c, alpha, eta, k["big_M"], in_, out_, u[i]),
                   node_lower_bound(G, c, alpha, eta, k["big_M"], in_, out_, np.zeros(p)), par)
        assert abs(lower[i] - at_u) <= certificate_tolerance(G, alpha, u[i], lower[i])
        assert abs(upper[i] - objective(G, c, alpha, eta, u[i])) <= certificate_tolerance(G, alpha, u[i], upper[i])
        assert np.all(np.abs(u[i]) <= k["big_M"]) and not u[i][out_].any()
    assert rc == (_engine.SLM_ERR_NOT_CONVERGED if stats[:, 1].any() else _engine.SLM_OK)  # (with every output valid either way)
    if name.startswith("rank_deficient"):
        assert G[7, 7] == 0.0 and not u[:, 7].any()  # IN on the zero column: u stays 0, its term h(c_7) - alpha is counted (above)


def test_no_start_and_no_parent_bound():
    """``starts=None`` and ``parent_lower=None``: the kernel's two branches without the optional arrays, bit for bit."""
    from sparselm_amd import _engine

    k = dict(cases()["slots65"])
    k["nodes"] = [(ce, in_, out_, -np.inf, None) for ce, in_, out_, _, _ in k["nodes"]]
    with _engine.get_engine().dataset(k["X"], k["y"]) as ds:
        lower, primal, upper, u, stats, _ = ds.solve_l0_local_nodes(k["alphas"], k["etas"], [n[0] for n in k["nodes"]],
                                                                    np.stack([to_words(n[1]) for n in k["nodes"]]),
                                                                    np.stack([to_words(n[2]) for n in k["nodes"]]), big_M=k["big_M"],
                                                                    parent_lower=None, starts=None, max_sweeps=k["max_sweeps"], gap_tol=k["gap_tol"])
        G, c, _ = ds.covariance_download(0)
        with pytest.raises(ValueError, match="neither a number nor -infinity"):
            ds.solve_l0_local_nodes(k["alphas"], k["etas"], [0], np.zeros((1, 16), dtype=np.uint64), np.zeros((1, 16), dtype=np.uint64),
                                    parent_lower=[np.nan])
    for i, run in enumerate(run_rule(G, c, k)):
        assert stats[i, 0] == run["sweeps"] and stats[i, 1] == run["status"]
        np.testing.assert_array_equal(u[i], run["u"])
        assert lower[i] == run["own_lower"] == run["lower"] and primal[i] == run["primal"] and upper[i] == run["upper"]


# ---- 2. the hard law ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hard_proof(seed, M, **kw):
    from sparselm_amd.miqp import l0_local_prove

    X, y, _, _ = hard_problem(seed)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        res = l0_local_prove(X, y, alphas=ALPHAS, etas=ETAS, big_M=M, rel_gap=REL_GAP, **dict(kw))
    return res, any(issubclass(w.category, ConvergenceWarning) for w in seen)


@pytest.mark.parametrize("M", BIG_MS)
@pytest.mark.parametrize("seed", range(3))
def test_the_hard_law_is_proven_at_the_brute_force_optimum(seed, M):
    res, warned = hard_proof(seed, M, max_nodes=4096)
    assert not warned and res.proven_optimal_.all() and (res.status_ == "optimal").all()  # the full tree has 2047 nodes
    for a, alpha in enumerate(ALPHAS):
        for e, eta in enumerate(ETAS):
            best = brute_force(seed, alpha, eta, M)
            scale = max(abs(best), alpha)
            print(f"seed {seed} M {M} alpha {alpha} eta {eta}: F* {best:.9e} proof {res.objectives_[a, e]:.9e} bound {res.lower_bounds_[a, e]:.9e} "
                  f"nodes {res.nodes_[a, e]} rounds {res.rounds_[a, e]}")
            assert abs(res.objectives_[a, e] - best) <= 2.0 * REL_GAP * scale  # no cell excluded
            assert res.lower_bounds_[a, e] <= best + 1e-9 * scale
            assert res.gaps_[a, e] <= REL_GAP


@pytest.mark.parametrize("seed", range(3))
def test_the_tree_equals_the_restatement_node_for_node(seed):
    """The engine's tree and the restatement's on the device's own Gram: nodes, rounds, coefficients and bounds, exactly.  Both
    boxes, all 18 cells of the seed; width 1, no incumbent, and a sweep cap of 25 a node, which keeps the restatement quick and
    sends some nodes back unclosed -- valid bounds that are split further, on both sides alike."""
    from sparselm_amd import _engine

    X, y, _, _ = hard_problem(seed)
    cells = [(alpha, eta) for alpha in ALPHAS for eta in ETAS]
    al, et = np.array([c[0] for c in cells]), np.array([c[1] for c in cells])
    for M in BIG_MS:
        with _engine.get_engine().dataset(X, y) as ds:
            out = ds.solve_l0_local_prove(al, et, big_M=M, rel_gap=REL_GAP, max_nodes=4096, width=1, max_sweeps=25, leaf_capacity=1 << 14)
            G, c, _ = ds.covariance_download(0)
        ref, launches = tree(G, c, cells, M, rel_gap=REL_GAP, max_nodes=4096, width=1, max_sweeps=25)
        print(f"seed {seed} M {M}: nodes {out['nodes'].tolist()} rounds {out['rounds'].tolist()} launches {len(launches)}")
        for e, cell in enumerate(ref):
            assert out["nodes"][e] == cell["nodes"] and out["rounds"][e] == cell["rounds"] and out["status"][e] == cell["status"]
            assert out["objective"][e] == cell["objective"] and out["lower_bound"][e] == cell["lower_bound"]
            np.testing.assert_array_equal(out["beta"][e], cell["beta"])
            assert int((out["leaves"]["cell"] == e).sum()) == len(cell["leaves"])
        assert out["leaves"]["count"] == sum(len(cell["leaves"]) for cell in ref)


@pytest.mark.parametrize("seed", range(3))
def test_the_public_call_equals_the_restatement_node_for_node(seed):
    """``l0_local_prove`` as it is called -- width 32, the incumbents of an ``L0LocalPath``, the cells of a grid sharing every launch --
    against the restatement's tree with ``path.coefs_`` as its incumbents, on the device's own Gram: ``nodes_``, ``rounds_``, the
    coefficients and the bounds, exactly.  Both boxes, all 18 cells of the seed; the sweep cap of 25 keeps the restatement quick."""
    from sparselm_amd import _engine
    from sparselm_amd.miqp import l0_local_prove, l0_local_search

    X, y, _, _ = hard_problem(seed)
    cells = [(alpha, eta) for alpha in ALPHAS for eta in ETAS]
    with _engine.get_engine().dataset(X, y) as ds:
        ds.covariance()
        G, c, _ = ds.covariance_download(0)
    for M in BIG_MS:
        path = l0_local_search(X, y, alphas=ALPHAS, etas=ETAS, big_M=M)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", ConvergenceWarning)
            res = l0_local_prove(X, y, alphas=ALPHAS, etas=ETAS, big_M=M, path=path, rel_gap=REL_GAP, max_nodes=4096, max_sweeps=25)
        ref, launches = tree(G, c, cells, M, incumbents=path.coefs_.reshape(9, -1), rel_gap=REL_GAP, max_nodes=4096, width=32, max_sweeps=25)
        print(f"seed {seed} M {M}: nodes {res.nodes_.ravel().tolist()} rounds {res.rounds_.ravel().tolist()} launches {launches}")
        assert res.nodes_.ravel().tolist() == [cell["nodes"] for cell in ref] and res.rounds_.ravel().tolist() == [cell["rounds"] for cell in ref]
        assert (res.status_.ravel() == "optimal").tolist() == [cell["status"] == 0 for cell in ref]
        np.testing.assert_array_equal(res.objectives_.ravel(), [cell["objective"] for cell in ref])
        np.testing.assert_array_equal(res.lower_bounds_.ravel(), [cell["lower_bound"] for cell in ref])
        np.testing.assert_array_equal(res.coefs_.reshape(9, -1), np.array([cell["beta"] for cell in ref]))


# ---- 3. the committed data against the exact search ---------------------------------------------------------------------------------
def test_the_reference_data_is_proven_at_the_exact_optimum():
    from sparselm_amd.miqp import L2L0, RegularizedL0, l0_local_prove

    X = np.load(os.path.join(ROOT, "tests", "golden", "reference_examples", "corr.npy"))
    y = np.load(os.path.join(ROOT, "tests", "golden", "reference_examples", "energy.npy"))
    assert X.shape == (290, 66)
    alphas, etas = np.array([0.01, 0.1]) * float(np.var(y)), [0.0, 0.01]
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        res = l0_local_prove(X, y, alphas=alphas, etas=etas, big_M=100, fit_intercept=True, rel_gap=REL_GAP, max_nodes=4000)
    assert res.proven_optimal_.all()
    for a, alpha in enumerate(alphas):
        for e, eta in enumerate(etas):
            opts = {"wide": True}
            est = (L2L0(alpha=alpha, eta=eta, big_M=100, fit_intercept=True, solver_options=opts) if eta > 0.0
                   else RegularizedL0(alpha=alpha, big_M=100, fit_intercept=True, solver_options=opts))
            with warnings.catch_warnings():
                warnings.simplefilter("error", ConvergenceWarning)
                est.fit(X, y)
            exact = est.solver_info_["objective"]  # (the units of L0LocalPath.objectives_: tests/test_l0_local_gpu.py compares them so)
            print(f"290 x 66 alpha {alpha:.4g} eta {eta}: proof {res.objectives_[a, e]:.10e} exact {exact:.10e} bound {res.lower_bounds_[a, e]:.10e} "
                  f"nodes {res.nodes_[a, e]} rounds {res.rounds_[a, e]}")
            assert est.solver_info_["proven_optimal"]
            assert abs(res.objectives_[a, e] - exact) <= 2.0 * REL_GAP * max(abs(exact), alpha)
            assert abs(res.intercepts_[a, e] - est.intercept_) <= 1e-6 * max(1.0, abs(est.intercept_))


# ---- 4. wider than any exact entry ---------------------------------------------------------------------------------------------------
def wide_draw():
    """120 x 160: AR(1) 0.5 columns, 6 true columns, SNR 4, default_rng(0)."""
    rng = np.random.default_rng(0)
    n, p = 120, 160
    Z = rng.standard_normal((n, p))
    X = Z.copy()
    for j in range(1, p):
        X[:, j] = 0.5 * X[:, j - 1] + np.sqrt(0.75) * Z[:, j]
    beta = np.zeros(p)
    beta[rng.choice(p, 6, replace=False)] = (-1.0) ** np.arange(6)
    signal = X @ beta
    y = signal + np.sqrt(np.var(signal) / 4.0) * rng.standard_normal(n)
    return X, y


def test_a_proof_at_160_columns_with_a_certificate_numpy_checks():
    from sparselm_amd import _engine
    from sparselm_amd.miqp import l0_local_prove, l0_local_search

    X, y = wide_draw()
    yy = float(y @ y) / len(y)
    alphas, eta, M = np.array([0.005, 0.02, 0.1]) * yy, 0.1, 100.0
    path = l0_local_search(X, y, alphas=alphas, etas=[eta], big_M=M)
    with warnings.catch_warnings():
        warnings.simplefilter("error", ConvergenceWarning)
        res = l0_local_prove(X, y, alphas=alphas, etas=[eta], big_M=M, rel_gap=REL_GAP, max_nodes=4000, return_certificate=True)
    with _engine.get_engine().dataset(X, y) as ds:
        ds.covariance()
        G, c, _ = ds.covariance_download(0)
    cert = res.certificate_
    print(f"120 x 160: nodes {res.nodes_[:, 0].tolist()} rounds {res.rounds_[:, 0].tolist()} leaves {len(cert['lower'])} gaps {res.gaps_[:, 0]}")
    assert res.proven_optimal_.all()
    for a, alpha in enumerate(alphas):
        best = res.objectives_[a, 0]
        scale = max(abs(best), alpha)
        assert res.lower_bounds_[a, 0] <= best <= path.objectives_[a, 0]
        assert abs(objective(G, c, alpha, eta, res.coefs_[a, 0]) - best) <= 1e-10 * scale
        mine = (cert["cell"][:, 0] == a) & (cert["cell"][:, 1] == 0)
        total, overlapping = leaves_cover(cert["in_"][mine], cert["out_"][mine])
        assert total == 1.0 and overlapping == 0  # the leaves partition the space of supports
        assert 2 * int(mine.sum()) - 1 == res.nodes_[a, 0]
        cut = best - REL_GAP * scale
        for in_, out_, u, lower in zip(cert["in_"][mine], cert["out_"][mine], cert["u"][mine], cert["lower"][mine]):
            at_u = max(node_lower_bound(G, c, alpha, eta, M, in_, out_, u), node_lower_bound(G, c, alpha, eta, M, in_, out_, np.zeros(160)))
            assert at_u >= cut - certificate_tolerance(G, alpha, u, cut)
            assert lower >= cut


# ---- 5. the node limit ------------------------------------------------------------------------------------------------------------------
def test_three_nodes_end_at_the_limit_with_a_proven_bound():
    from sparselm_amd.miqp import l0_local_bound

    seed, M = 0, 100.0
    X, y, _, _ = hard_problem(seed)
    res, warned = hard_proof(seed, M, max_nodes=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", ConvergenceWarning)
        root = l0_local_bound(X, y, alphas=ALPHAS, etas=ETAS, big_M=M, gap_tol=REL_GAP / 100.0)
    assert warned and (res.status_ == "node_limit").any() and not res.proven_optimal_.all()
    assert np.array_equal(res.status_ == "node_limit", ~res.proven_optimal_) and (res.nodes_ <= 3).all()
    for a, alpha in enumerate(ALPHAS):
        for e, eta in enumerate(ETAS):
            best = brute_force(seed, alpha, eta, M)
            print(f"alpha {alpha} eta {eta}: F* {best:.9e} bound {res.lower_bounds_[a, e]:.9e} root {root.lower_bounds_[a, e]:.9e} "
                  f"objective {res.objectives_[a, e]:.9e} {res.status_[a, e]}")
            assert res.lower_bounds_[a, e] <= best + 1e-9 * max(abs(best), alpha)
            assert res.lower_bounds_[a, e] >= root.lower_bounds_[a, e]  # a child's bound is never below its parent's
            assert res.objectives_[a, e] >= best - 1e-9 * max(abs(best), alpha)


# ---- 6. the surface ---------------------------------------------------------------------------------------------------------------------
def test_intercept_weights_a_given_path_and_the_edges():
    from sparselm_amd.miqp import l0_local_prove, l0_local_search

    X, y, _, _ = hard_problem(1)
    y = y + 3.0
    w = np.random.default_rng(2).uniform(0.5, 2.0, len(y))
    alphas, etas = [0.0, 0.05], [0.01]
    path = l0_local_search(X, y, alphas=alphas, etas=etas, big_M=100, fit_intercept=True, sample_weight=w)
    given = l0_local_prove(X, y, alphas=alphas, etas=etas, big_M=100, fit_intercept=True, sample_weight=w, path=path, max_nodes=4096)
    own = l0_local_prove(X, y, alphas=alphas, etas=etas, big_M=100, fit_intercept=True, sample_weight=w, max_nodes=4096)
    assert given.proven_optimal_.all() and own.proven_optimal_.all()
    np.testing.assert_array_equal(given.objectives_, own.objectives_)  # path=None runs the same search on the same handle
    np.testing.assert_array_equal(given.nodes_, own.nodes_)
    assert (given.objectives_ <= path.objectives_).all() and (given.lower_bounds_ <= given.objectives_).all()
    # alpha = 0: nothing is paid for a column, the ridge regression on all columns is the optimum
    G, c, _, mean, y_mean = gram(X, y, sample_weight=w, fit_intercept=True)
    b = np.linalg.solve(G + 2.0 * 0.01 * np.eye(10), c)
    exact = 0.5 * b @ (G + 0.02 * np.eye(10)) @ b - c @ b
    assert abs(given.objectives_[0, 0] - exact) <= 2.0 * REL_GAP * abs(exact)
    assert abs(given.intercepts_[0, 0] - (y_mean - mean @ given.coefs_[0, 0])) <= 1e-9
    # big_M = 0: no launch, everything zero, proven
    zero = l0_local_prove(X, y, alphas=[0.1], big_M=0)
    assert zero.proven_optimal_.all() and not zero.coefs_.any() and zero.objectives_[0, 0] == 0.0 and zero.lower_bounds_[0, 0] == 0.0
    assert zero.nodes_[0, 0] == 0 and zero.rounds_[0, 0] == 0


def test_the_engine_refuses_by_class():
    from sparselm_amd import _engine

    X, y, _, _ = hard_problem(0)
    none = np.zeros((1, 16), dtype=np.uint64)
    with _engine.get_engine().dataset(X, y) as ds:
        with pytest.raises(ValueError, match="rel_gap must lie in"):
            ds.solve_l0_local_prove([0.1], rel_gap=2.0)
        with pytest.raises(ValueError, match="max_nodes must be >= 1"):
            ds.solve_l0_local_prove([0.1], max_nodes=0)
        with pytest.raises(ValueError, match="width must be >= 1"):
            ds.solve_l0_local_prove([0.1], width=0)
        with pytest.raises(ValueError, match="outside the box"):
            ds.solve_l0_local_prove([0.1], big_M=1.0, incumbents=np.full((1, 10), 2.0))
        with pytest.raises(ValueError, match="not a cell of the call"):
            ds.solve_l0_local_nodes([0.1], [0.0], [1], none, none)
        both = none.copy()
        both[0, 0] = 1
        with pytest.raises(ValueError, match="both IN and OUT"):
            ds.solve_l0_local_nodes([0.1], [0.0], [0], both, both)
        ds.set_groups(np.arange(10) // 2, 5)
        with pytest.raises(NotImplementedError, match="groups"):
            ds.solve_l0_local_prove([0.1])
        with pytest.raises(NotImplementedError, match="groups"):
            ds.solve_l0_local_nodes([0.1], [0.0], [0], none, none)
