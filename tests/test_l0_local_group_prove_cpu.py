"""The local proof with groups without a GPU: the mathematics (the group penalty's conjugate against a dense numerical supremum,
the node inequality against a brute force over a node's closed supports), the restated tree on the group hard law against brute
force with its certificate, the host twin against the restatement bit for bit under AddressSanitizer and
UndefinedBehaviorSanitizer too (tests/l0_local_group_prove_host_test.cpp, a stand-alone program), the refusals with their
messages, and the public surface."""

import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _l0_local_group_prove_cases import cases, run_rule
from _l0_local_group_prove_reference import (brute_force, closed_supports, h_of, leaves_cover, node_brute_force, node_lower_bound, node_rule,
                                             phi_g_conj, phi_g_scan, tree)
from _l0_local_groups_reference import close_hierarchy, group_law

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "sparse-lm_amd", "csrc")
REL_GAP = 1e-6
ALPHAS, ETAS, BIG_M = (1e-3, 0.1, 0.5), (0.0, 0.02, 1.0), 100.0
SWEEPS = 40  # a node's sweep cap in the restated trees: it keeps them quick; an unclosed node's bound is valid and is split further


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open an engine fails the test: validation errors have to come first."""
    from sparselm_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were validated")

    monkeypatch.setattr(_engine, "get_engine", boom)


def law(seed):
    X, y, gstart = group_law(seed)
    n = len(y)
    return X.T @ X / n, X.T @ y / n, gstart


def chain(ng):
    return [[]] + [[g - 1] for g in range(1, ng)]


# ---- 1. the mathematics -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta, M, alpha", [(0.05, 0.8, 0.3), (0.05, 100.0, 0.3), (0.0, 2.0, 0.3)])  # a binding M, a loose M, eta = 0
def test_the_conjugate_against_a_dense_numerical_supremum(eta, M, alpha):
    """phi_g*(t) = max(0, h(t_1) + h(t_2) - alpha) for 2-column groups, against sup over a grid of b of t.b - phi_g(b) with phi_g by
    its own scan of z.  The grid's supremum falls short of the true one by at most (|t|_1 + phi_g's slope) times half a step; the
    box is cut at 4 where M is loose (the maximiser |t_j| / (2 eta) lies inside)."""
    top = min(M, 4.0)
    grid = np.linspace(-top, top, 161)
    step = grid[1] - grid[0]
    rng = np.random.default_rng(0)
    worst = 0.0
    for t in rng.uniform(-0.35, 0.35, (6, 2)):
        sup = 0.0
        for b1 in grid:
            for b2 in grid:
                sup = max(sup, t[0] * b1 + t[1] * b2 - phi_g_scan(np.array([b1, b2]), alpha, eta, M, points=2001))
        closed = phi_g_conj(t, alpha, eta, M)
        slope = np.abs(t).sum() + 2.0 * (2.0 * eta * top + alpha / top)
        worst = max(worst, abs(sup - closed))
        assert sup <= closed + 1e-9 and closed - sup <= slope * step
    print(f"eta {eta} M {M} alpha {alpha}: largest |sup - closed form| {worst:.2e}")


def test_the_three_regimes_of_the_penalty_equal_its_scan():
    from _l0_local_group_prove_reference import _values  # the rule's closed pieces: P - (quadratic) at a FREE group of three

    rng = np.random.default_rng(1)
    gstart = np.array([0, 3])
    for eta, M, alpha in [(0.05, 0.8, 0.3), (0.05, 100.0, 0.3), (0.0, 2.0, 0.3), (1.0, 100.0, 0.01), (0.02, 1.0, 0.5)]:
        for _ in range(20):
            b = rng.uniform(-M, M, 3) * rng.choice([1e-3, 0.1, 1.0]) * (rng.random(3) < 0.8)
            lam, tauc = 0.0, 0.0  # (not read: the group has three columns)
            P, _, _ = _values(b[None, :], np.zeros((1, 3)), np.zeros(3), np.array([alpha]), np.array([eta]), np.array([lam]), np.array([tauc]), M,
                              gstart, np.zeros((1, 1), dtype=int), np.zeros(1))
            scan = phi_g_scan(b, alpha, eta, M)
            assert abs(P[0] - scan) <= 1e-6 * max(scan, 1e-12) + 1e-12, (eta, M, alpha, b, P[0], scan)


@pytest.mark.parametrize("chained", [False, True])
def test_the_node_inequality_against_a_brute_force_over_the_node(chained):
    G, c, gstart = law(0)
    G, c, gstart = G[:8, :8], c[:8], gstart[:5]  # four groups of two
    ng = 4
    need = chain(ng) if chained else None
    closed = close_hierarchy(ng, need)
    rng = np.random.default_rng(5)
    sup = closed_supports(ng, closed)
    assert len(sup) == (5 if chained else 16)
    for eta in (0.0, 0.02, 1.0):
        for alpha in (1e-3, 0.1, 0.5):
            for _ in range(4):
                if chained:
                    gin, gout = np.arange(ng) < rng.integers(0, 3), np.arange(ng) >= ng - rng.integers(0, 3)
                else:
                    state = rng.integers(0, 3, ng)
                    gin, gout = state == 1, state == 2
                best = node_brute_force(G, c, alpha, eta, BIG_M, gstart, closed, gin, gout)
                for scale in (0.0, 0.1, 1.0):  # random u
                    u = rng.standard_normal(8) * scale
                    u[np.repeat(gout, 2)] = 0.0
                    assert node_lower_bound(G, c, alpha, eta, BIG_M, gstart, gin, gout, u) <= best + 1e-10 * max(abs(best), alpha)
                r = node_rule(G, c, BIG_M, gstart, closed, [alpha], [eta], gin[None], gout[None], max_sweeps=2000, gap_tol=1e-9)  # descended u
                low = node_lower_bound(G, c, alpha, eta, BIG_M, gstart, gin, gout, r["u"][0])
                assert low <= best + 1e-10 * max(abs(best), alpha) and abs(r["lower"][0] - max(low, node_lower_bound(
                    G, c, alpha, eta, BIG_M, gstart, gin, gout, np.zeros(8)))) <= 1e-10 * max(abs(low), alpha)
                assert r["upper"][0] >= brute_force(G, c, alpha, eta, BIG_M, gstart, closed) - 1e-10 * max(abs(best), alpha)
                assert r["status"][0] == 0 and r["primal"][0] - r["lower"][0] <= 1.0001e-9 * max(abs(r["primal"][0]), alpha) + 1e-15


def test_a_zero_group_moves_iff_its_conjugate_is_positive():
    """Condition 3: two columns that each stay below alpha alone and pass it together move; scaled below, they stay."""
    G = np.array([[1.0, 0.0], [0.0, 1.0]])
    eta, alpha = 0.5, 0.3
    for t, moves in ((0.6, True), (0.5, False)):  # h(t) = t^2 / 2: 0.18 + 0.18 > 0.3; 0.125 + 0.125 < 0.3
        c = np.array([t, -t])
        assert (float(np.sum(h_of(c, eta, BIG_M))) > alpha) == moves and h_of(c, eta, BIG_M)[0] < alpha
        r = node_rule(G, c, BIG_M, np.array([0, 2]), [[]], [alpha], [eta], np.zeros((1, 1), dtype=bool), np.zeros((1, 1), dtype=bool))
        assert bool(r["u"][0].any()) == moves and r["status"][0] == 0


# ---- 2. the restated tree on the group hard law -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hard_tree(seed, chained):
    G, c, gstart = law(seed)
    cells = [(alpha, eta) for alpha in ALPHAS for eta in ETAS]
    need = chain(len(gstart) - 1) if chained else None
    return tree(G, c, cells, BIG_M, gstart, need=need, rel_gap=REL_GAP, max_nodes=200, width=4, max_sweeps=SWEEPS)


# the restatement's own node counts, as observed (alpha-major, eta-minor): not targets, a record that a change of the rule shows in
NODES = {(0, False): [51, 5, 3, 47, 11, 1, 19, 7, 1], (0, True): [7, 3, 5, 9, 7, 1, 7, 5, 1],
         (1, False): [37, 9, 3, 27, 3, 1, 15, 1, 1], (1, True): [7, 3, 5, 11, 3, 1, 3, 1, 1],
         (2, False): [81, 17, 3, 39, 7, 1, 15, 3, 1], (2, True): [11, 5, 5, 9, 7, 1, 3, 3, 1]}


@pytest.mark.parametrize("chained", [False, True])
@pytest.mark.parametrize("seed", range(3))
def test_the_tree_on_the_group_hard_law(seed, chained):
    G, c, gstart = law(seed)
    ng = len(gstart) - 1
    closed = close_hierarchy(ng, chain(ng) if chained else None)
    out, launches = hard_tree(seed, chained)
    print(f"seed {seed} chain {chained}: nodes {[cell['nodes'] for cell in out]} launches {launches}")
    if (seed, chained) in NODES:
        assert [cell["nodes"] for cell in out] == NODES[(seed, chained)]
    e = 0
    for alpha in ALPHAS:
        for eta in ETAS:
            cell, best = out[e], brute_force(G, c, alpha, eta, BIG_M, gstart, closed)
            e += 1
            scale = max(abs(best), alpha)
            print(f"  alpha {alpha} eta {eta}: F* {best:.9e} objective {cell['objective']:.9e} bound {cell['lower_bound']:.9e} nodes {cell['nodes']} "
                  f"status {cell['status']}")
            assert cell["lower_bound"] <= best + 1e-9 * scale and cell["objective"] >= best - 1e-9 * scale  # honest either way
            if eta > 0.0:
                assert cell["status"] == 0 and abs(cell["objective"] - best) <= 2.0 * REL_GAP * scale
                assert cell["objective"] - cell["lower_bound"] <= REL_GAP * max(abs(cell["objective"]), alpha)
            # the certificate: the leaves partition the closed supports, and every leaf's bound re-evaluates
            gin, gout = np.array([lf[0] for lf in cell["leaves"]]), np.array([lf[1] for lf in cell["leaves"]])
            if cell["status"] == 0:
                assert (leaves_cover(gin, gout, closed) == 1).all()
            for lf_in, lf_out, u, lower in cell["leaves"]:
                at_u = max(node_lower_bound(G, c, alpha, eta, BIG_M, gstart, lf_in, lf_out, u),
                           node_lower_bound(G, c, alpha, eta, BIG_M, gstart, lf_in, lf_out, np.zeros(len(c))))
                assert at_u <= lower + 1e-10 * max(abs(lower), alpha)  # (lower may hold an ancestor's bound, never less than its own)
                assert lower <= node_brute_force(G, c, alpha, eta, BIG_M, gstart, closed, lf_in, lf_out) + 1e-9 * scale


# ---- 3. the host twin -----------------------------------------------------------------------------------------------------------------
def _csr(need, ng):
    lists = [[] for _ in range(ng)] if need is None else need
    return np.concatenate([[0], np.cumsum([len(v) for v in lists])]), np.array([h for v in lists for h in v], dtype=float)


@functools.lru_cache(maxsize=None)
def exported():
    """``(the file's doubles, nodes, tree cells)``: every node of every shared case with the restatement's answer (the 1024-column
    case aside: the GPU test runs it), a singleton case for the column twin's bits, then trees of the hard law."""
    parts, nodes, tree_cells = [], 0, 0

    def put(*values):
        for v in values:
            parts.append(np.atleast_1d(np.asarray(v, dtype=np.float64)).ravel())

    def put_groups(gstart, need):
        ng = len(gstart) - 1
        ptr, idx = _csr(need, ng)
        put(ng, gstart, ptr, idx)

    todo = {name: k for name, k in cases().items() if not name.startswith("p1024")}
    single = dict(cases()["rank_deficient_fours"])
    single["gstart"] = np.arange(21)
    flat = lambda m: np.repeat(m, 4)  # noqa: E731  (a group's state for each of its four columns)
    single["nodes"] = [(ce, flat(gi), flat(go), par, st) for ce, gi, go, par, st in single["nodes"]]
    todo["singletons"] = single
    put(len(todo))
    for name, k in todo.items():
        n = len(k["y"])
        G, c = k["X"].T @ k["X"] / n, k["X"].T @ k["y"] / n
        runs = run_rule(G, c, k)
        put(len(c), len(k["alphas"]), k["big_M"], k["max_sweeps"], k["gap_tol"], len(runs))
        put_groups(k["gstart"], k["need"])
        put(G, c, np.stack([k["alphas"], k["etas"]], axis=1))
        for (cell, gin, gout, parent, start), run in zip(k["nodes"], runs):
            put(cell, int(start is not None), parent, gin, gout)
            if start is not None:
                put(start)
            put(run["sweeps"], run["status"], run["lower"], run["primal"], run["upper"], run["u"])
            nodes += 1
    trees = []
    cells = [(alpha, eta) for alpha in ALPHAS for eta in ETAS]
    for seed, chained in ((0, False), (0, True)):
        G, c, gstart = law(seed)
        trees.append((G, c, gstart, chain(7) if chained else None, 200, 4, SWEEPS, None, hard_tree(seed, chained)[0]))
    G, c, gstart = law(1)
    inc = np.zeros((9, 14))
    inc[:, 2:4] = (-0.3, 0.2)  # (group 1: under the chain its closure counts two groups)
    trees.append((G, c, gstart, chain(7), 9, 32, 25, inc, tree(G, c, cells, BIG_M, gstart, need=chain(7), incumbents=inc, rel_gap=REL_GAP,
                                                                 max_nodes=9, width=32, max_sweeps=25)[0]))
    put(len(trees))
    for G, c, gstart, need, max_nodes, width, max_sweeps, inc, out in trees:
        put(len(c), len(cells), BIG_M, REL_GAP, max_nodes, width, max_sweeps, int(inc is not None))
        put_groups(gstart, need)
        put(G, c, np.array(cells))
        if inc is not None:
            put(inc)
        for cell in out:
            put(cell["nodes"], cell["rounds"], cell["status"], cell["objective"], cell["lower_bound"], len(cell["leaves"]), cell["beta"])
            tree_cells += 1
    return np.concatenate(parts), nodes, tree_cells


@pytest.mark.parametrize("sanitize", [False, True])
def test_l0_local_group_prove_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l0_local_group_prove_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    # (-ffp-contract=off: the twin's bits must not depend on whether this host has fused multiply-adds; the header says so too)
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags,
                            os.path.join(ROOT, "tests", "l0_local_group_prove_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    blob, nodes, tree_cells = exported()
    blob.tofile(str(tmp_path / "cases.bin"))
    assert nodes >= 6 * (len(cases()) - 1) and tree_cells == 27
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "l0_local_group_prove_host_test: ok" in run.stdout and f"exported: {nodes} nodes, {tree_cells} tree cells" in run.stdout


# ---- 4. the refusals ------------------------------------------------------------------------------------------------------------------
def test_every_refusal_has_its_message_before_a_device():
    with open(os.path.join(CSRC, "engine_l0.hip")) as fh:
        unit = fh.read()
    with open(os.path.join(CSRC, "l0_host.hpp")) as fh:
        host = fh.read()
    with open(os.path.join(ROOT, "include", "slm_engine.h")) as fh:
        header = fh.read()
    shared = unit[unit.index("int l0_gp_refuse("):]
    shared = shared[: shared.index("\n}\n")]
    words = {"L0_GP_ORDER": ("SLM_ERR_UNSUPPORTED", "contiguous and ascending in column order"),
             "L0_GP_NEED_PTR": ("SLM_ERR_BAD_ARG", "need_ptr must start at 0 and never fall"),
             "L0_GP_NEED_IDX": ("SLM_ERR_BAD_ARG", "need_idx[%lld] must name one of the %d groups"),
             "L0_GP_RANGE": ("SLM_ERR_BAD_ARG", "fixes a group beyond the %d groups"),
             "L0_GP_UNCLOSED": ("SLM_ERR_BAD_ARG", "is not closed under the hierarchy"),
             "L0_GP_SHARDED": ("SLM_ERR_UNSUPPORTED", "not built for row-sharded datasets")}
    enum = host[host.index("enum L0GpKind"):]
    enum = enum[: enum.index("};")]
    assert re.findall(r"\b(L0_GP_[A-Z_]+)\b", enum[enum.index("{"):]) == ["L0_GP_OK", "L0_GP_FIRST"] + list(words)
    at = []
    for name, (code, text) in words.items():
        case = shared[shared.index(f"case {name}:"):]
        case = case[: case.index(";")]
        assert code in case and text in case.replace('"\n                  "', ""), name
        at.append(shared.index(f"case {name}:"))
    assert at == sorted(at)
    for impl, check in (("solve_l0_local_group_nodes_impl", "l0_group_nodes_check("), ("solve_l0_local_group_prove_impl", "l0_group_prove_check(")):
        body = unit[unit.index(f"int {impl}("):]
        body = body[: body.index("\n}\n")]
        assert "hipSetDevice" not in body and "hipMalloc" not in body and "run.open(" not in body  # the device is opened behind the checks
        assert body.index(check) < body.index("l0_gp_refuse(") < body.index("own.build(") < body.index("_impl(ds,", 10)
    for entry in ("slm_solve_l0_local_group_nodes", "slm_solve_l0_local_group_prove"):
        assert f'extern "C" int {entry}(' in unit and f"int {entry}(slm_dataset* ds" in header
    # the older entries still refuse groups, in their words
    assert 'case L0_ND_GROUPS: return fail(SLM_ERR_UNSUPPORTED, "the l0 local proof is not built for groups' in unit
    assert 'case L0_PV_GROUPS: return fail(SLM_ERR_UNSUPPORTED, "the l0 local proof is not built for groups' in unit


def test_python_refuses_before_a_device(no_device):
    from sparselm_amd.miqp import l0_local_group_prove
    from sparselm_amd.model._l0_local import L0LocalPath
    from sparselm_amd.model._l0_local_groups import L0LocalGroupPath

    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((20, 6)), rng.standard_normal(20)
    groups = [0, 0, 1, 1, 2, 2]
    with pytest.raises(ValueError, match="alphas must be finite and >= 0"):
        l0_local_group_prove(X, y, alphas=[0.1, -1.0], groups=groups)
    for bad in (1e-11, 1.5, np.nan, True):
        with pytest.raises(ValueError, match=r"rel_gap must be a number in \[1e-10, 1\]"):
            l0_local_group_prove(X, y, alphas=[0.1], groups=groups, rel_gap=bad)
    with pytest.raises(ValueError, match="max_nodes must be an integer >= 1"):
        l0_local_group_prove(X, y, alphas=[0.1], groups=groups, max_nodes=0)
    with pytest.raises(ValueError, match="width must be an integer >= 1"):
        l0_local_group_prove(X, y, alphas=[0.1], groups=groups, width=0)
    with pytest.raises(ValueError, match="max_sweeps must be an integer >= 1"):
        l0_local_group_prove(X, y, alphas=[0.1], groups=groups, max_sweeps=0)
    with pytest.raises(ValueError, match="unknown solver_options"):
        l0_local_group_prove(X, y, alphas=[0.1], groups=groups, solver_options={"swaps": True})
    z = np.zeros((1, 1))
    plain = L0LocalPath([0.1], [0.0], np.zeros((1, 1, 6)), z, z, z, 1, z[None], z, z, z)
    with pytest.raises(ValueError, match="path must be an L0LocalGroupPath"):
        l0_local_group_prove(X, y, alphas=[0.1], groups=groups, path=plain)

    def path_of(alphas, coefs, supports):
        return L0LocalGroupPath(alphas, [0.0], coefs, z, z, z, 1, z[None], z, z, z, group_supports=supports, trials=z)

    with pytest.raises(ValueError, match="different .alpha, eta. grids"):
        l0_local_group_prove(X, y, alphas=[0.1], groups=groups, path=path_of([0.3], np.zeros((1, 1, 6)), np.zeros((1, 1, 3))))
    coefs = np.zeros((1, 1, 6))
    coefs[0, 0, 4] = 0.5  # group 2, which needs 1 and 0 under the chain
    with pytest.raises(ValueError, match="different groups or hierarchies"):
        l0_local_group_prove(X, y, alphas=[0.1], groups=groups, hierarchy=[[], [0], [1]], path=path_of([0.1], coefs, [[[False, False, True]]]))
    with pytest.raises(ValueError, match="different groups or hierarchies"):
        l0_local_group_prove(X, y, alphas=[0.1], groups=groups, path=path_of([0.1], coefs, [[[False, True]]]))
    with pytest.raises(ValueError, match="inside the box"):
        l0_local_group_prove(X, y, alphas=[0.1], groups=groups, big_M=0.1, path=path_of([0.1], coefs, [[[False, False, True]]]))
    with pytest.raises(NotImplementedError, match="takes up to 1024 columns"):
        l0_local_group_prove(np.zeros((3, 1025)), np.zeros(3), alphas=[0.1])
    with pytest.raises(ValueError, match="more than the 8192 cells"):
        l0_local_group_prove(X, y, alphas=np.linspace(0.1, 1.0, 100), etas=np.linspace(0.0, 1.0, 82), groups=groups)


# ---- the public surface -----------------------------------------------------------------------------------------------------------------
def test_exports_signature_and_the_abi():
    import inspect

    import sparselm_amd.miqp as miqp
    from sparselm_amd import _engine
    from sparselm_amd.model._l0_local_prove import L0LocalProof

    assert issubclass(miqp.L0LocalGroupProof, L0LocalProof)
    sig = inspect.signature(miqp.l0_local_group_prove)
    assert list(sig.parameters) == ["X", "y", "alphas", "groups", "hierarchy", "etas", "big_M", "fit_intercept", "sample_weight", "path", "rel_gap",
                                    "max_nodes", "width", "max_sweeps", "return_certificate", "solver_options"]
    defaults = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults == dict(groups=None, hierarchy=None, etas=(0.0,), big_M=100, fit_intercept=False, sample_weight=None, path=None, rel_gap=1e-6,
                            max_nodes=20000, width=32, max_sweeps=None, return_certificate=False, solver_options=None)
    assert "l0_local_group_prove" not in miqp.__all__
    for entry in ("slm_solve_l0_local_group_nodes", "slm_solve_l0_local_group_prove"):
        assert entry in _engine.ABI_SYMBOLS
    assert hasattr(_engine.Dataset, "solve_l0_local_group_nodes") and hasattr(_engine.Dataset, "solve_l0_local_group_prove")


def test_the_kernel_follows_the_family_discipline():
    with open(os.path.join(CSRC, "l0_local_group_node_kernels.hpp")) as fh:
        kernel = fh.read()
    body = kernel[kernel.index("void l0_local_group_node_kernel("):]
    assert "#pragma clang fp contract(off)" in body[:200] and "l0_ls_axpy(" in body and "atomicAdd" not in kernel
    assert "__shared__ double us_s[L0_WAVES][L0_LS_PMAX], hs_s[L0_WAVES][L0_LS_PMAX]" in body  # per-wave tables, 64 KB a workgroup
    for shared in ("l0_gn_coord(", "l0_gn_jump(", "l0_gn_bstar(", "l0_lb_coord(", "l0_node_coord(", "l0_gn_group_phi(", "l0_gn_group_conj("):
        assert shared in kernel  # the one definition of every number, l0_host.hpp's
