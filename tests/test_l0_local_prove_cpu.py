"""The local proof without a GPU: the node inequality on the numpy reference alone (brute force over the node's supports), the
restated tree against brute force on the hard law's 54 cells (proven optimal, at most 511 nodes a cell at width 1), the
certificate's covering and leaf-bound checks, the host twin and its tree against the restatement bit for bit -- under
AddressSanitizer and UndefinedBehaviorSanitizer too (tests/l0_local_prove_host_test.cpp, a stand-alone program) -- the refusals
with their messages, and the public surface."""

import functools
import inspect
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from _l0_local_bound_reference import ALPHAS, BIG_MS, ETAS, brute_force, certificate_tolerance, hard_problem, rule
from _l0_local_prove_cases import cases, reference
from _l0_local_prove_reference import (branch, from_words, leaves_cover, node_lower_bound, node_rule, objective, polish_on, prove_value,
                                       to_words, tree)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "sparse-lm_amd", "csrc")
REL_GAP = 1e-6
HARD = [(seed, M) for seed in range(3) for M in BIG_MS]


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to open an engine fails the test: validation errors have to come first."""
    from sparselm_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were validated")

    monkeypatch.setattr(_engine, "get_engine", boom)


def hard_cells():
    return [(alpha, eta) for eta in ETAS for alpha in ALPHAS]


@functools.lru_cache(maxsize=None)
def hard_tree(seed, M):
    """The restated tree on the nine (eta, alpha) cells of hard_law(seed) under the box M: width 1, no incumbent beyond 0.
    Computed once per process and left unchanged."""
    _, _, G, c = hard_problem(seed)
    return tree(G, c, hard_cells(), M, rel_gap=REL_GAP, max_nodes=4096, width=1)


# ---- 1. the inequality ------------------------------------------------------------------------------------------------------------
def _node_optimum(G, c, alpha, eta, M, in_, out_):
    """min F over the node by brute force: every support between nothing and the columns that are not OUT, the IN columns
    paying alpha whether zero or not."""
    from _l0_local_bound_reference import _box_qp

    p = len(c)
    free = [j for j in range(p) if not in_[j] and not out_[j]]
    fixed = [j for j in range(p) if in_[j]]
    best = np.inf
    for k in range(len(free) + 1):
        for S in itertools.combinations(free, k):
            cols = np.array(sorted(fixed + list(S)), dtype=int)
            q = 0.0 if cols.size == 0 else _box_qp(G[np.ix_(cols, cols)] + (2.0 * eta + 1e-13) * np.eye(cols.size), c[cols], M)
            best = min(best, q + alpha * cols.size)
    return best


def test_the_node_bound_is_a_bound_on_small_nodes():
    _, _, G, c = hard_problem(0, n=30, p=7)
    rng = np.random.default_rng(3)
    tight = 0
    for eta, M, alpha in ((0.0, 100.0, 0.1), (0.01, 0.7, 1e-3), (1.0, 100.0, 0.5), (0.01, 100.0, 0.1)):
        for _ in range(6):
            s = rng.choice(3, size=7, p=[0.5, 0.25, 0.25])
            in_, out_ = s == 1, s == 2
            best = _node_optimum(G, c, alpha, eta, M, in_, out_)
            r = node_rule(G, c, alpha, eta, M, in_, out_, max_sweeps=2000, gap_tol=1e-10)
            slack = 1e-9 * max(abs(best), alpha)
            assert r["lower"] <= best + slack
            for u in (np.zeros(7), r["u"], rng.standard_normal(7) * 0.3):
                v = u * ~out_
                assert node_lower_bound(G, c, alpha, eta, M, in_, out_, v) <= best + slack
            assert np.all(r["u"][out_] == 0.0) and np.all(np.abs(r["u"]) <= M)
            assert abs(r["upper"] - objective(G, c, alpha, eta, r["u"])) <= 1e-12 * max(abs(r["upper"]), alpha)
            tight += (best - r["lower"]) <= 0.05 * max(abs(best), alpha)
    assert tight >= 6  # (with a ridge or a binding box a node's bound is within a few per cent)


def test_the_rule_certifies_itself_on_every_case():
    """The restatement's own bound against node_lower_bound at its u, and that the cases do what they are there for."""
    for name, k in cases().items():
        G, c, runs = reference(name)
        p = len(c)
        assert len(runs) >= 8
        cells_used = set()
        for (cell, in_, out_, parent, start), run in zip(k["nodes"], runs):
            alpha, eta = float(k["alphas"][cell]), float(k["etas"][cell])
            cells_used.add(cell)
            at_u = max(node_lower_bound(G, c, alpha, eta, k["big_M"], in_, out_, run["u"]),
                       node_lower_bound(G, c, alpha, eta, k["big_M"], in_, out_, np.zeros(p)))
            assert abs(run["own_lower"] - at_u) <= certificate_tolerance(G, alpha, run["u"], run["own_lower"]), name
            assert run["lower"] == max(run["own_lower"], parent)
            assert np.all(run["u"][out_] == 0.0) and np.all(np.abs(run["u"]) <= k["big_M"]) and run["sweeps"] <= k["max_sweeps"]
            assert abs(run["upper"] - objective(G, c, alpha, eta, run["u"])) <= certificate_tolerance(G, alpha, run["u"], run["upper"])
            if not in_.any() and not out_.any():  # with empty masks the node is the bound's cell, bit for bit
                b = rule(G, c, alpha, eta, k["big_M"], start=start, max_sweeps=k["max_sweeps"], gap_tol=k["gap_tol"])
                assert b["lower"] == run["own_lower"] and b["primal"] == run["primal"] and np.array_equal(b["u"], run["u"])
                assert b["sweeps"] == run["sweeps"] and b["status"] == run["status"]
        masks = [(i.tobytes(), o.tobytes()) for _, i, o, _, _ in k["nodes"]]
        none, every = np.zeros(p, dtype=bool).tobytes(), np.ones(p, dtype=bool).tobytes()
        assert (none, none) in masks and (none, every) in masks and (every, none) in masks
        if p > 64:
            assert any(i[63] and o[64] for _, i, o, _, _ in k["nodes"]) and any(o[63] and i[64] for _, i, o, _, _ in k["nodes"])
        if name.startswith("rank_deficient"):
            assert G[7, 7] == 0.0 and any(i[7] and not i.all() for _, i, o, _, _ in k["nodes"]) and all(r["u"][7] == 0.0 for r in runs)
        if name == "slots65_one_sweep":
            assert all(r["sweeps"] == 1 for r in runs)
        if name != "p1":
            assert len(cells_used) == len(k["alphas"]) > 1  # nodes of different cells in one batch
    assert {float(e) for k in cases().values() for e in k["etas"]} >= {0.0, 0.02, 1.0}
    assert {k["big_M"] for k in cases().values()} == {0.6, 100.0}


def test_masks_round_trip_and_the_polish_is_the_minimiser():
    rng = np.random.default_rng(0)
    flags = rng.random(130) < 0.4
    w = to_words(flags)
    assert w.shape == (16,) and np.array_equal(from_words(w, 130), flags)
    assert (int(w[0]) >> 5) & 1 == int(flags[5]) and (int(w[1]) >> 0) & 1 == int(flags[64])
    _, _, G, c = hard_problem(1)
    for eta, M in ((0.0, 100.0), (0.01, 0.7)):
        cols = [1, 4, 6]
        quad, beta = polish_on(G, c, eta, M, cols, rng.standard_normal(10) * np.isin(np.arange(10), cols))
        from _l0_local_bound_reference import _box_qp

        exact = _box_qp(G[np.ix_(cols, cols)] + 2.0 * eta * np.eye(3), c[cols], M)
        assert abs(quad - exact) <= 1e-10 * abs(exact) and np.all(np.abs(beta) <= M) and set(np.flatnonzero(beta)) <= set(cols)
        assert abs(prove_value(G, c, 0.1, eta, beta) - (quad + 0.3)) <= 1e-12


def test_the_branching_rule():
    G, c = np.eye(4), np.array([0.1, -0.9, 0.5, 0.2])
    none = np.zeros(4, dtype=bool)
    assert branch(G, c, 1.0, none, none, np.array([0.2, 0.45, -0.55, 1.0])) == 1  # |z - 1/2| = 0.05 twice: the lowest index
    assert branch(G, c, 1.0, none, none, np.array([0.0, 1.0, -2.0, 0.0])) == 2    # every z is 0 or 1: the largest |u_j|
    assert branch(G, c, 1.0, none, none, np.zeros(4)) == 1                        # all zero: the largest |t_j| = |c_j|
    assert branch(G, c, 0.0, none, none, np.array([0.0, 0.3, 0.0, 0.0])) == 1     # tauc = 0: z = 1 where u != 0
    taken = np.array([False, True, True, False])
    assert branch(G, c, 1.0, taken, none, np.array([0.0, 0.5, 0.5, 0.0])) == 3    # only FREE columns: the largest |t_j| among them
    assert branch(G, c, 1.0, taken, ~taken, np.zeros(4)) == -1


# ---- 2. the tree on the hard law ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, M", HARD)
def test_the_tree_proves_the_hard_law(seed, M):
    """All 54 cells (nine per case): proven optimal under max_nodes = 4096 at the brute-force optimum, at most 511 nodes a cell
    at width 1 without an incumbent, and the certificate covers the space with every leaf's bound at or above the cut."""
    _, _, G, c = hard_problem(seed)
    out, launches = hard_tree(seed, M)
    for (alpha, eta), cell in zip(hard_cells(), out):
        best = brute_force(seed, alpha, eta, M)
        scale = max(abs(best), alpha)
        print(f"seed {seed} M {M} eta {eta} alpha {alpha}: F* {best:.9e} tree {cell['objective']:.9e} bound {cell['lower_bound']:.9e} "
              f"nodes {cell['nodes']} rounds {cell['rounds']}")
        assert cell["status"] == 0
        assert abs(cell["objective"] - best) <= 2.0 * REL_GAP * scale
        assert cell["lower_bound"] <= best + 1e-9 * scale
        assert cell["nodes"] <= 511  # a quarter of the full tree's 2047
        assert abs(objective(G, c, alpha, eta, cell["beta"]) - cell["objective"]) <= 1e-12 * scale
        in_ = np.array([leaf[0] for leaf in cell["leaves"]])
        out_ = np.array([leaf[1] for leaf in cell["leaves"]])
        total, overlapping = leaves_cover(in_, out_)
        assert total == 1.0 and overlapping == 0
        assert 2 * len(cell["leaves"]) - 1 == cell["nodes"]  # a binary tree: every bound evaluation is a leaf or was split
        cut = cell["objective"] - REL_GAP * max(abs(cell["objective"]), alpha)
        for li, lo, u, lower in cell["leaves"]:
            at_u = max(node_lower_bound(G, c, alpha, eta, M, li, lo, u), node_lower_bound(G, c, alpha, eta, M, li, lo, np.zeros(len(c))))
            assert at_u >= cut - certificate_tolerance(G, alpha, u, cut)
            assert lower >= cut
    assert max(launches) <= 18 and launches[0] == 9  # width 1: two children a cell a round


def test_a_wider_round_and_an_incumbent_grow_a_valid_tree():
    """width 32 with the optimum's neighbour as the incumbent, and a node limit of 3: the bound stays proven."""
    _, _, G, c = hard_problem(2)
    cells, M = hard_cells(), 0.7
    inc = np.zeros((9, 10))
    inc[:, 0] = 0.2
    out, launches = tree(G, c, cells, M, incumbents=inc, rel_gap=REL_GAP, max_nodes=4096, width=32)
    few, _ = tree(G, c, cells, M, rel_gap=REL_GAP, max_nodes=3, width=32)
    for (alpha, eta), cell, short, narrow in zip(cells, out, few, hard_tree(2, M)[0]):
        best = brute_force(2, alpha, eta, M)
        assert cell["status"] == 0 and abs(cell["objective"] - best) <= 2.0 * REL_GAP * max(abs(best), alpha)
        assert abs(cell["objective"] - narrow["objective"]) <= 2.0 * REL_GAP * max(abs(best), alpha)
        assert short["nodes"] <= 3 and short["lower_bound"] <= best + 1e-9 * max(abs(best), alpha) and short["lower_bound"] <= short["objective"]
        assert short["status"] in (0, 1) and (short["status"] == 1 or short["objective"] - short["lower_bound"] <= REL_GAP * max(abs(best), alpha))
    assert max(launches) <= 2 * 32 * 9


# ---- 3. the host twin -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exported():
    """``(the file's doubles, nodes, tree cells)``: every node of every shared case with the restatement's answer, then the hard
    law's six trees and a wide one with an incumbent -- the twin must give the same bits.  Built once per process."""
    parts, nodes, tree_cells = [], 0, 0

    def put(*values):
        for v in values:
            parts.append(np.atleast_1d(np.asarray(v, dtype=np.float64)).ravel())

    put(len(cases()))
    for name, k in cases().items():
        G, c, runs = reference(name)
        put(len(c), len(k["alphas"]), k["big_M"], k["max_sweeps"], k["gap_tol"], len(runs), G, c, np.stack([k["alphas"], k["etas"]], axis=1))
        for (cell, in_, out_, parent, start), run in zip(k["nodes"], runs):
            put(cell, int(start is not None), parent, in_, out_)
            if start is not None:
                put(start)
            put(run["sweeps"], run["status"], run["lower"], run["primal"], run["upper"], run["u"])
            nodes += 1
    trees = []
    for seed, M in HARD:
        _, _, G, c = hard_problem(seed)
        trees.append((G, c, hard_cells(), M, 4096, 1, 10000, None, hard_tree(seed, M)[0]))
    _, _, G, c = hard_problem(1)
    inc = np.zeros((9, 10))
    inc[:, 2] = -0.3
    trees.append((G, c, hard_cells(), 0.7, 9, 32, 25, inc, tree(G, c, hard_cells(), 0.7, incumbents=inc, rel_gap=REL_GAP, max_nodes=9, width=32,
                                                              max_sweeps=25)[0]))
    put(len(trees))
    for G, c, cells, M, max_nodes, width, max_sweeps, inc, out in trees:
        put(len(c), len(cells), M, REL_GAP, max_nodes, width, max_sweeps, int(inc is not None), G, c, np.array(cells))
        if inc is not None:
            put(inc)
        for cell in out:
            put(cell["nodes"], cell["rounds"], cell["status"], cell["objective"], cell["lower_bound"], len(cell["leaves"]), cell["beta"])
            tree_cells += 1
    return np.concatenate(parts), nodes, tree_cells


@pytest.mark.parametrize("sanitize", [False, True])
def test_l0_local_prove_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l0_local_prove_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    # (-ffp-contract=off: the twin's bits must not depend on whether this host has fused multiply-adds; the header says so too)
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags,
                            os.path.join(ROOT, "tests", "l0_local_prove_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    blob, nodes, tree_cells = exported()
    blob.tofile(str(tmp_path / "cases.bin"))
    assert nodes >= 8 * len(cases()) and tree_cells == 63
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "l0_local_prove_host_test: ok" in run.stdout and f"exported: {nodes} nodes, {tree_cells} tree cells" in run.stdout


# ---- 4. the refusals ------------------------------------------------------------------------------------------------------------
def _refusals(unit, host, impl, check_call, enum_name, check_name, ok, table):
    body = unit[unit.index(f"int {impl}("):]
    body = body[: body.index("\n}\n")]
    assert "hipSetDevice" not in body and "hipMalloc" not in body  # the device is opened by L0NodeRunner::open alone ...
    assert body.index(check_call) < body.index("run.open(")       # ... and every refusal comes before it
    enum = host[host.index(f"enum {enum_name}"):]
    enum = enum[: enum.index("};")]
    order = [re.search(rf"\b{name}\b", enum).start() for name in table]
    assert order == sorted(order)  # the order of the check is the order of the enum, and of this table
    names = re.findall(r"\b(L0_[A-Z]+_[A-Z_]+)\b", enum[enum.index("{"):])
    assert names == [ok] + list(table)  # and the table leaves no refusal out
    cases_at = []
    for name, (code, words) in table.items():
        line = body[body.index(f"case {name}:"):]
        line = line[: line.index("\n")]
        assert code in line and words in line, name
        cases_at.append(body.index(f"case {name}:"))
    assert cases_at == sorted(cases_at)
    check = host[host.index(f"inline {enum_name} {check_name}("):]
    check = check[: check.index(f"return {ok};")]
    at = [check.index(f"return {name};") for name in table]
    assert at == sorted(at)


def test_every_refusal_has_its_message_before_a_device():
    with open(os.path.join(CSRC, "engine_l0.hip")) as fh:
        unit = fh.read()
    with open(os.path.join(CSRC, "l0_host.hpp")) as fh:
        host = fh.read()
    for entry in ("slm_solve_l0_local_nodes", "slm_solve_l0_local_prove"):
        assert f'extern "C" int {entry}(' in unit
    runner = unit[unit.index("struct L0NodeRunner"):]
    assert runner.index("hipSetDevice") < runner.index("l0_local_hold_grams(")  # the only place of the two entries that opens the device
    common = {
        "BIG_M": ("SLM_ERR_BAD_ARG", "big_M must be >= 0"),
        "ALPHA": ("SLM_ERR_BAD_ARG", "alphas[%lld] must be finite and >= 0"),
        "ETA": ("SLM_ERR_BAD_ARG", "etas[%lld] must be finite and >= 0"),
    }
    head = {"NULL": ("SLM_ERR_BAD_ARG", "NULL argument"), "CELLS": ("SLM_ERR_BAD_ARG", "n_cells must be >= 1"),
            "PROBLEMS": ("SLM_ERR_BAD_ARG", "n_cells must be at most %d cells")}
    tail = {"GROUPS": ("SLM_ERR_UNSUPPORTED", "the l0 local proof is not built for groups"),
            "SHARDED": ("SLM_ERR_UNSUPPORTED", "the l0 local proof is not built for row-sharded datasets")}
    width = {"WIDTH": ("SLM_ERR_UNSUPPORTED", "the l0 local proof takes up to %d columns")}
    prove = {**head, **common, "REL_GAP": ("SLM_ERR_BAD_ARG", "rel_gap must lie in [1e-10, 1]"),
             "MAX_NODES": ("SLM_ERR_BAD_ARG", "max_nodes must be >= 1"), "TREE_WIDTH": ("SLM_ERR_BAD_ARG", "width must be >= 1"), **width,
             "INCUMBENT": ("SLM_ERR_BAD_ARG", "incumbents[%lld] is outside the box"), **tail}
    nodes = {**head, "NODES": ("SLM_ERR_BAD_ARG", "n_nodes must be >= 1"), "BATCH": ("SLM_ERR_BAD_ARG", "n_nodes must be at most %d nodes"),
             **common, "GAP_TOL": ("SLM_ERR_BAD_ARG", "gap_tol must be >= 0"), **width,
             "CELL": ("SLM_ERR_BAD_ARG", "cell[%lld] is not a cell of the call"), "MASK": ("SLM_ERR_BAD_ARG", "both IN and OUT"),
             "PARENT": ("SLM_ERR_BAD_ARG", "parent_lower[%lld] is neither a number nor -infinity"),
             "START": ("SLM_ERR_BAD_ARG", "starts[%lld] is not a finite number"), **tail}
    _refusals(unit, host, "solve_l0_local_prove_impl", "l0_prove_check(", "L0PvRefusal", "l0_prove_check", "L0_PV_OK",
              {f"L0_PV_{k}": v for k, v in prove.items()})
    _refusals(unit, host, "solve_l0_local_nodes_impl", "l0_nodes_check(", "L0NdRefusal", "l0_nodes_check", "L0_ND_OK",
              {f"L0_ND_{k}": v for k, v in nodes.items()})
    body = unit[unit.index("int solve_l0_local_prove_impl("):]
    assert body.index("big_M == 0.0") < body.index("run.open(")  # everything zero, proven, without a launch
    # the older entry and its check are as they were
    assert "enum L0LbRefusal { L0_LB_OK = 0, L0_LB_NULL, L0_LB_CELLS, L0_LB_PROBLEMS, L0_LB_BIG_M, L0_LB_ALPHA, L0_LB_ETA, L0_LB_GAP_TOL" in host


def test_python_refuses_before_a_device(no_device):
    from sparselm_amd.miqp import l0_local_prove
    from sparselm_amd.model._l0_local import L0LocalPath

    rng = np.random.default_rng(0)
    X, y = rng.standard_normal((20, 5)), rng.standard_normal(20)
    with pytest.raises(ValueError, match="alphas must be finite and >= 0"):
        l0_local_prove(X, y, alphas=[0.1, -1.0])
    with pytest.raises(ValueError, match="etas must be finite and >= 0"):
        l0_local_prove(X, y, alphas=[0.1], etas=[np.nan])
    with pytest.raises(ValueError, match="non-empty"):
        l0_local_prove(X, y, alphas=[])
    for bad in (1e-11, 1.5, -1.0, np.nan, True):
        with pytest.raises(ValueError, match=r"rel_gap must be a number in \[1e-10, 1\]"):
            l0_local_prove(X, y, alphas=[0.1], rel_gap=bad)
    with pytest.raises(ValueError, match="max_nodes must be an integer >= 1"):
        l0_local_prove(X, y, alphas=[0.1], max_nodes=0)
    with pytest.raises(ValueError, match="width must be an integer >= 1"):
        l0_local_prove(X, y, alphas=[0.1], width=0)
    with pytest.raises(ValueError, match="max_sweeps must be an integer >= 1"):
        l0_local_prove(X, y, alphas=[0.1], max_sweeps=0)
    with pytest.raises(ValueError, match="unknown solver_options"):
        l0_local_prove(X, y, alphas=[0.1], solver_options={"swaps": True})
    with pytest.raises(ValueError, match="path must be an L0LocalPath"):
        l0_local_prove(X, y, alphas=[0.1], path=np.zeros((1, 1, 5)))
    z = np.zeros((1, 1))
    for other in (L0LocalPath([0.3], [0.0], np.zeros((1, 1, 5)), z, z, z, 1, z[None], z, z, z),
                  L0LocalPath([0.1], [0.0, 1.0], np.zeros((1, 2, 5)), z, z, z, 1, z[None], z, z, z),
                  L0LocalPath([0.1], [0.0], np.zeros((1, 1, 4)), z, z, z, 1, z[None], z, z, z)):
        with pytest.raises(ValueError, match="different"):
            l0_local_prove(X, y, alphas=[0.1], path=other)
    outside = L0LocalPath([0.1], [0.0], np.full((1, 1, 5), 2.0), z, z, z, 1, z[None], z, z, z)
    with pytest.raises(ValueError, match="inside the box"):
        l0_local_prove(X, y, alphas=[0.1], big_M=1.0, path=outside)
    with pytest.raises(NotImplementedError, match="takes up to 1024 columns"):
        l0_local_prove(np.zeros((3, 1025)), np.zeros(3), alphas=[0.1])
    with pytest.raises(ValueError, match="more than the 8192 cells"):
        l0_local_prove(X, y, alphas=np.linspace(0.1, 1.0, 100), etas=np.linspace(0.0, 1.0, 82))
    with pytest.raises((ValueError, TypeError)):
        l0_local_prove(X, y, alphas=[0.1], big_M=-1.0)


# ---- the public surface ---------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_under_abi_24():
    from sparselm_amd import _engine

    assert _engine.ABI_VERSION == 24
    with open(os.path.join(ROOT, "include", "slm_engine.h")) as fh:
        header = fh.read()
    assert "#define SLM_ABI_VERSION 24" in header
    wanted = {
        "slm_solve_l0_local_nodes": ("slm_dataset* ds", "int32_t n_cells", "const double* alphas", "const double* etas", "double big_M",
                                     "int32_t n_nodes", "const int32_t* cell", "const uint64_t* in_mask", "const uint64_t* out_mask",
                                     "const double* parent_lower", "const double* starts", "int32_t max_sweeps", "double gap_tol",
                                     "double* lower_out", "double* primal_out", "double* upper_out", "double* u_out", "int32_t* stat_out",
                                     "slm_point_info* info"),
        "slm_solve_l0_local_prove": ("slm_dataset* ds", "int32_t n_cells", "const double* alphas", "const double* etas", "double big_M",
                                     "const double* incumbents", "double rel_gap", "int32_t max_nodes", "int32_t width", "int32_t max_sweeps",
                                     "int64_t leaf_capacity", "double* beta_out", "double* objective_out", "double* lower_out",
                                     "int32_t* nodes_out", "int32_t* rounds_out", "int32_t* status_out", "int32_t* leaf_cell", "uint64_t* leaf_in",
                                     "uint64_t* leaf_out", "double* leaf_u", "double* leaf_lower", "int64_t* leaf_count", "slm_point_info* info"),
    }
    for entry, args in wanted.items():
        assert entry in _engine.ABI_SYMBOLS and f"int {entry}(" in header
        decl = re.sub(r"/\*.*?\*/", "", header[header.index(f"int {entry}("):], flags=re.S)
        decl = " ".join(decl[: decl.index(";")].split())
        at = [decl.index(arg) for arg in args]
        assert at == sorted(at) and decl.count(",") == len(args) - 1  # every argument, in this order, and no other
        assert len(getattr(_engine.load_library(), entry).argtypes) == len(args)
    comment = header[: header.index("int slm_solve_l0_local_prove(")]
    comment = comment[comment.rindex("/*"):]
    for words in ("PROVEN OPTIMAL", "WHERE THE TREE CLOSES", "mode = 13", "Refusals", "Not here", "big_M = 0"):
        assert words in comment, words
    assert hasattr(_engine.Dataset, "solve_l0_local_nodes") and hasattr(_engine.Dataset, "solve_l0_local_prove")
    assert "slm_solve_l0_local_bound" in _engine.ABI_SYMBOLS and len(_engine.load_library().slm_solve_l0_local_bound.argtypes) == 13


def test_exports_signature_and_the_result():
    import sparselm_amd.miqp as miqp
    from sparselm_amd.model import _l0_local, _l0_local_bound, _l0_local_prove

    assert _l0_local_prove.__all__ == ["l0_local_prove", "L0LocalProof"]
    for name in _l0_local_prove.__all__:
        assert getattr(miqp, name) is getattr(_l0_local_prove, name) and name not in miqp.__all__
    assert miqp.__all__ == ["BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L1L0", "L2L0"]
    assert _l0_local_bound.__all__ == ["l0_local_bound", "L0LocalBound"] and _l0_local.__all__ == ["l0_local_search", "L0LocalPath"]
    params = inspect.signature(miqp.l0_local_prove).parameters
    assert list(params) == ["X", "y", "alphas", "etas", "big_M", "fit_intercept", "sample_weight", "path", "rel_gap", "max_nodes", "width",
                            "max_sweeps", "return_certificate", "solver_options"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in params.items() if k not in ("X", "y"))
    assert [params[k].default for k in list(params)[3:]] == [(0.0,), 100, False, None, None, 1e-6, 20000, 32, None, False, None]
    for doc in (_l0_local_prove.__doc__, miqp.l0_local_prove.__doc__):
        assert "closes" in doc and "ridge" in doc and "eta = 0" in doc and "p > n" in doc
    assert "l0_local_prove" in _l0_local.__doc__ and "l0_local_prove" in miqp.__doc__
    proof = miqp.L0LocalProof([0.1, 0.2], [0.0], np.zeros((2, 1, 3)), [[0.0], [0.0]], [[-1.0], [-0.5]], [[-1.0], [-0.9]], [[5], [7]], [[3], [4]],
                              np.array([["optimal"], ["node_limit"]], dtype=object))
    for name in ("alphas_", "etas_", "coefs_", "intercepts_", "objectives_", "lower_bounds_", "gaps_", "proven_optimal_", "nodes_", "rounds_",
                 "status_", "certificate_"):
        assert hasattr(proof, name), name
    assert proof.proven_optimal_.dtype == bool and proof.proven_optimal_.tolist() == [[True], [False]]
    np.testing.assert_allclose(proof.gaps_, [[0.0], [0.8]])
    assert proof.certificate_ is None


def test_the_kernel_the_twin_and_the_documents():
    with open(os.path.join(CSRC, "l0_local_node_kernels.hpp")) as fh:
        kernel = fh.read()
    with open(os.path.join(CSRC, "l0_host.hpp")) as fh:
        host = fh.read()
    assert "asm" not in kernel and "atomicAdd" not in kernel and "__shared__" not in kernel and "__syncthreads" not in kernel
    assert "l0_local_body.inc" not in kernel and "void l0_local_node_kernel(L0NdArgs a)" in kernel
    assert kernel.count("l0_ls_axpy(t, G, ld, p, ns, lane, 0.0,") == 2  # the filed Gram through the family's helper, ridge argument 0
    for shared in ("l0_node_coord(", "l0_node_phi(", "l0_node_conj(", "l0_node_combine(", "l0_lb_changed(", "l0_lb_closed("):
        assert shared in kernel
    for shared in ("constexpr double l0_node_coord(", "constexpr double l0_node_phi(", "constexpr double l0_node_conj(",
                   "constexpr double l0_node_h(", "constexpr L0NodeValues l0_node_combine("):
        assert shared in host
    assert "inline L0NodeResult l0_node_solve(" in host and "inline int l0_prove_tree(" in host
    section = host[host.index("// ---- local proof"):]
    assert section.index("#pragma GCC optimize(\"fp-contract=off\")") < section.index("l0_node_solve(")
    with open(os.path.join(CSRC, "engine_l0.hip")) as fh:
        unit = fh.read()
    assert unit.count("l0_prove_tree(") == 1 and "l0_ls_polish_on(" in section  # one body: the engine passes the launch to the host's tree
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        design = fh.read()
    assert "**Local proof**" in design and "profiles/l0_local_prove.txt" in design
    section = design[design.index("**Local proof**"):]
    for words in ("L_node(u)", "closest to 1/2", "does not close", "eta = 0", "*Not built:*"):
        assert words in section, words
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert "l0_local_prove" in fh.read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "l0_local_prove.txt"))
    assert os.path.exists(os.path.join(ROOT, "tools", "l0_local_prove_timing.py"))
