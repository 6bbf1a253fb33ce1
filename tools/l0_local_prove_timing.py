"""Measurements of the local proof (``l0_local_prove``, ``slm_solve_l0_local_prove``) for ``profiles/l0_local_prove.txt``.

1. Whole calls on the reference's 290 x 66 data and on a 120 x 160 draw at 1 / 16 / 64 cells, beside the host twin on one core
   (``tools/l0_local_prove_host_bench.cpp``: ``l0_prove_tree`` with ``l0_node_solve``, compiled here with g++ -O2
   -ffp-contract=off) and, at 66 columns, beside the exact ``RegularizedL0`` / ``L2L0`` fits with ``wide``; nodes, rounds and nodes
   per launch of every run.
2. A 400 x 1024 run with eta > 0: what is proven, and what gap is left at the node limit.
3. The hard law (30 x 10, AR(1) 0.9), 54 cells: nodes to a proof at width 1 without an incumbent and as the call is made, against
   the brute-force optimum.
4. ``--parent-tree``: ``slm_solve_l0_local_bound`` and ``slm_solve_l0_local`` against a built checkout of the parent commit, fresh
   processes alternating; the criterion is "inside the parent's own min .. max".

No timing is a pass criterion; the file states what was found, losses included.  Usage: ``python tools/l0_local_prove_timing.py
[--repeats 3] [--parent-tree DIR] [--out FILE]``.
"""

import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time
import warnings

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage -c csrc/engine_l0.hip, on this commit and on its parent
RESOURCES = [
    "resource lines (the build's own remarks):",
    "    l0_local_node_kernel           256 VGPRs +  12 AGPRs, 135 SGPR spills, no scratch, no LDS, one wave per SIMD",
    "    l0_local_bound_kernel          255 VGPRs +   2 AGPRs,  92 SGPR spills, no scratch, no LDS   (the parent's, figure for figure)",
    "    l0_local_kernel<false>         256 VGPRs +  74 AGPRs, 164 SGPR spills, no scratch, no LDS   (the parent's)",
    "    l0_local_kernel<true>          256 VGPRs + 171 AGPRs, 222 SGPR spills, no scratch, no LDS   (the parent's)",
    "    l0_local_l1_kernel             256 VGPRs +  78 AGPRs, 174 SGPR spills, no scratch, no LDS   (the parent's)",
    "    l0_local_group_kernel          256 VGPRs + 196 AGPRs, 207 SGPR spills, no scratch, 65536 B LDS   (the parent's)",
    "    (the remarks of the two builds were compared line by line: every one of the 107 kernels of the parent's engine_l0.hip, the five",
    "     older local kernels among them, keeps every figure of the parent's build; the node kernel is the one new entry)",
]
MAX_NODES = 4000
REL_GAP = 1e-6


def wide_draw():
    """120 x 160: AR(1) 0.5 columns, 6 true columns, SNR 4, default_rng(0) -- the draw of tests/test_l0_local_prove_gpu.py."""
    rng = np.random.default_rng(0)
    n, p = 120, 160
    Z = rng.standard_normal((n, p))
    X = Z.copy()
    for j in range(1, p):
        X[:, j] = 0.5 * X[:, j - 1] + np.sqrt(0.75) * Z[:, j]
    beta = np.zeros(p)
    beta[rng.choice(p, 6, replace=False)] = (-1.0) ** np.arange(6)
    signal = X @ beta
    return X, signal + np.sqrt(np.var(signal) / 4.0) * rng.standard_normal(n)


def shapes():
    d = os.path.join(ROOT, "tests", "golden", "reference_examples")
    Xr, yr = np.load(os.path.join(d, "corr.npy")), np.load(os.path.join(d, "energy.npy"))
    rng = np.random.default_rng(1024)
    Xw = rng.standard_normal((400, 1024))
    bw = np.zeros(1024)
    bw[rng.choice(1024, 24, replace=False)] = (-1.0) ** np.arange(24)
    return (Xr, yr), wide_draw(), (Xw, Xw @ bw + 0.5 * rng.standard_normal(400))


def child(tree):
    """One process of the parent comparison: whole calls of the two older entries on the package of ``tree``."""
    sys.path.insert(0, os.path.join(tree, "sparse-lm_amd"))
    from sparselm_amd.miqp import l0_local_bound, l0_local_search

    (Xr, yr), _, (Xw, yw) = shapes()
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, X, y, icpt, eta in (("290 x 66", Xr, yr, True, 1e-3), ("400 x 1024", Xw, yw, False, 0.05)):
            for cells in (16, 64):
                al = np.geomspace(0.3, 0.003, cells) * float(np.var(y))
                for what, fn in (("bound", lambda: l0_local_bound(X, y, alphas=al, etas=[eta], big_M=100.0, fit_intercept=icpt, max_sweeps=2000)),
                                 ("search", lambda: l0_local_search(X, y, alphas=al, etas=[eta], big_M=100.0, fit_intercept=icpt, max_rounds=0))):
                    fn()
                    ts = []
                    for _ in range(3):
                        t0 = time.perf_counter()
                        fn()
                        ts.append((time.perf_counter() - t0) * 1e3)
                    out[f"{what} | {name} | {cells}"] = ts
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l0_local_prove.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child", default=None, help="internal: time the older entries on the package of this checkout and print JSON")
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    repeats = max(1, args.repeats)
    sys.path[:0] = [os.path.join(ROOT, "sparse-lm_amd"), os.path.join(ROOT, "tests")]

    from sparselm_amd import _engine
    from sparselm_amd.miqp import L2L0, RegularizedL0, l0_local_prove, l0_local_search

    dev = _engine.get_engine().device_info()
    lines = [f"the local proof (l0_local_prove, slm_solve_l0_local_prove) on {dev['name'].strip() or 'device'}, {dev['compute_units']} compute units",
             f"(wall time of whole calls, each ending in a synchronise; every shape warmed first; {repeats} repeats, medians with min .. max)",
             *RESOURCES, ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def say(line):
        lines.append(line)
        print(line, flush=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def clock(fn):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            out = fn()
            return out, (time.perf_counter() - t0) * 1e3

    def fmt(ms):
        return f"{np.median(ms):9.2f} ({min(ms):.2f} .. {max(ms):.2f})"

    (Xr, yr), (Xd, yd), (Xw, yw) = shapes()
    exe = os.path.join(tempfile.mkdtemp(), "l0_local_prove_host_bench")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off",
                    os.path.join(ROOT, "tools", "l0_local_prove_host_bench.cpp"), "-o", exe], check=True)

    def host(X, y, cell_alphas, cell_etas, big_M, centre, incumbents, width=32, max_nodes=MAX_NODES):
        n, p = X.shape
        Xc, yc = (X - X.mean(axis=0), y - y.mean()) if centre else (X, y)
        G, c = Xc.T @ Xc / n, Xc.T @ yc / n
        path_in = exe + ".in"
        with open(path_in, "wb") as fh:
            fh.write(struct.pack("<7q2d", p, p, len(cell_alphas), max_nodes, width, 10000, 1, big_M, REL_GAP))
            for a in (G, c, np.asarray(cell_alphas, dtype=np.float64), np.asarray(cell_etas, dtype=np.float64), incumbents):
                fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        out = subprocess.run([exe, path_in], check=True, capture_output=True, text=True).stdout.splitlines()
        return float(out[0].split()[3]), out[0]

    # ---- 1. whole calls beside the twin and the exact fits --------------------------------------------------------------------------------
    say(f"1. ONE l0_local_prove call (rel_gap {REL_GAP:g}, max_nodes {MAX_NODES}, width 32, the incumbents from an L0LocalPath computed before the")
    say("   clock starts: path=) beside l0_prove_tree with l0_node_solve on ONE core (once per row; the host time is the tree alone on a Gram it is")
    say("   handed, a call's includes the upload, the Gram, its download for the tree and every round's copies).  alphas: a geometric grid from")
    say("   0.1 var y down to 0.01 var y (one cell: 0.03 var y).  nodes / launch: all bound evaluations of the call over its launches.")
    for X, y, icpt, etas, what in ((Xr, yr, True, (0.0, 0.01), "the reference's 290 x 66 data, fit_intercept, big_M = 100"),
                                   (Xd, yd, False, (0.1,), "the 120 x 160 draw (AR(1) 0.5, 6 true columns, SNR 4), big_M = 100")):
        for eta in etas:
            say(f"   {what}, eta = {eta:g}")
            say(f"{'cells':>6s} {'prove ms: median (min .. max)':>34s} {'host twin ms':>13s} {'prove/host':>11s} {'proven':>9s} {'nodes':>8s} "
                f"{'most a cell':>12s} {'rounds':>7s} {'nodes/launch':>13s}   the host's line")
            for cells in (1, 16, 64):
                al = np.geomspace(0.1, 0.01, cells) * float(np.var(y)) if cells > 1 else np.array([0.03 * float(np.var(y))])
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    path = l0_local_search(X, y, alphas=al, etas=[eta], big_M=100.0, fit_intercept=icpt)
                prove = lambda: l0_local_prove(X, y, alphas=al, etas=[eta], big_M=100.0, fit_intercept=icpt, path=path, rel_gap=REL_GAP,  # noqa: E731
                                               max_nodes=MAX_NODES)
                clock(prove)
                tp, res = [], None
                for _ in range(repeats):
                    res, ms = clock(prove)
                    tp.append(ms)
                th, line = host(X, y, al, np.full(cells, eta), 100.0, icpt, path.coefs_[:, 0])
                ratio = float(np.median(tp) / th)
                launches = int(res.rounds_.max())
                say(f"{cells:6d} {fmt(tp):>34s} {th:13.2f} {ratio:11.3f} {int(res.proven_optimal_.sum()):4d} / {cells:<3d} {int(res.nodes_.sum()):8d} "
                    f"{int(res.nodes_.max()):12d} {launches:7d} {res.nodes_.sum() / launches:13.1f}   {line}"
                    + ("  -- the call LOSES to one core" if ratio >= 1.0 else ""))
            if X is Xr:
                al = np.array([0.01, 0.1]) * float(np.var(y))
                path = l0_local_search(X, y, alphas=al, etas=[eta], big_M=100.0, fit_intercept=True)
                res, ms = clock(lambda: l0_local_prove(X, y, alphas=al, etas=[eta], big_M=100.0, fit_intercept=True, path=path, max_nodes=MAX_NODES))
                for a, alpha in enumerate(al):
                    opts = {"wide": True, "max_nodes": 1 << 24}
                    est = (L2L0(alpha=alpha, eta=eta, big_M=100, fit_intercept=True, solver_options=opts) if eta > 0.0
                           else RegularizedL0(alpha=alpha, big_M=100, fit_intercept=True, solver_options=opts))
                    clock(lambda: est.fit(X, y))
                    _, t_ex = clock(lambda: est.fit(X, y))
                    info = est.solver_info_
                    say(f"    alpha / var y = {alpha / np.var(y):.2g}: proof {res.objectives_[a, 0]:.10e} bound {res.lower_bounds_[a, 0]:.10e} nodes "
                        f"{res.nodes_[a, 0]} rounds {res.rounds_[a, 0]} {res.status_[a, 0]}; exact (wide) {info['objective']:.10e} "
                        f"{'proven' if info['proven_optimal'] else 'NOT proven'} in {t_ex:.1f} ms; local search {path.objectives_[a, 0]:.10e}")
                say(f"    (the two-cell proof call: {ms:.1f} ms)")
    say("")

    # ---- 2. 400 x 1024 ----------------------------------------------------------------------------------------------------------------------
    say("2. Synthetic 400 x 1024 (24 true columns, noise 0.5), big_M = 100, eta = 0.05, four alphas, max_nodes = 400: what is proven and what gap")
    say("   is left at the node limit, beside the root bound's gap (l0_local_bound's value is the root's).")
    al = np.array([0.3, 0.1, 0.03, 0.01]) * float(np.var(yw))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        path = l0_local_search(Xw, yw, alphas=al, etas=[0.05], big_M=100.0)
        root = l0_local_prove(Xw, yw, alphas=al, etas=[0.05], big_M=100.0, path=path, max_nodes=1)
    prove = lambda: l0_local_prove(Xw, yw, alphas=al, etas=[0.05], big_M=100.0, path=path, rel_gap=REL_GAP, max_nodes=400)  # noqa: E731
    clock(prove)
    tp, res = [], None
    for _ in range(repeats):
        res, ms = clock(prove)
        tp.append(ms)
    say(f"    the call: {fmt(tp)} ms, {int(res.rounds_.max())} launches, {int(res.nodes_.sum())} nodes")
    for a, alpha in enumerate(al):
        say(f"    alpha / var y = {alpha / np.var(yw):.2g}: {res.status_[a, 0]:>10s}, nodes {res.nodes_[a, 0]:4d}, objective {res.objectives_[a, 0]:.8e}, "
            f"proven gap {res.gaps_[a, 0]:.3e} (the root alone: {root.gaps_[a, 0]:.3e}), non-zeros {int(np.count_nonzero(res.coefs_[a, 0]))}")
    say("")

    # ---- 3. the hard law: nodes to a proof ------------------------------------------------------------------------------------------------
    from _l0_local_bound_reference import ALPHAS, BIG_MS, ETAS, brute_force, hard_problem

    say("3. NODES TO A PROOF.  The hard law (30 x 10, AR(1) 0.9), seeds 0 .. 2, alpha in {1e-3, 0.1, 0.5}, max_nodes = 4096 (the full tree has 2047")
    say("   nodes): slm_solve_l0_local_prove at width 1 WITHOUT an incumbent beyond 0, and l0_local_prove as it is called (width 32, the local")
    say("   search's incumbents); 9 cells per row.  off: the largest |objective - F*| / max(|F*|, alpha) against the brute force over all supports.")
    say(f"{'eta':>6s} {'big_M':>6s} {'proven':>8s} {'most nodes, width 1':>20s} {'all nodes':>10s} {'proven':>8s} {'most nodes, default':>20s} {'all nodes':>10s} {'off':>9s}")
    rows, cells_hl = {}, [(a, e) for a in ALPHAS for e in ETAS]
    for seed in range(3):
        X, y, _, _ = hard_problem(seed)
        for M in BIG_MS:
            with _engine.get_engine().dataset(X, y) as ds:
                one = ds.solve_l0_local_prove([c[0] for c in cells_hl], [c[1] for c in cells_hl], big_M=M, rel_gap=REL_GAP, max_nodes=4096, width=1)
            res, _ = clock(lambda: l0_local_prove(X, y, alphas=ALPHAS, etas=ETAS, big_M=M, rel_gap=REL_GAP, max_nodes=4096))
            for i, (alpha, eta) in enumerate(cells_hl):
                best = brute_force(seed, alpha, eta, M)
                off = max(abs(one["objective"][i] - best), abs(res.objectives_.ravel()[i] - best)) / max(abs(best), alpha)
                rows.setdefault((eta, M), []).append((int(one["status"][i]) == 0, int(one["nodes"][i]), bool(res.proven_optimal_.ravel()[i]),
                                                      int(res.nodes_.ravel()[i]), off))
    for (eta, M), r in sorted(rows.items()):
        say(f"{eta:6g} {M:6g} {sum(x[0] for x in r):3d} / {len(r):<2d} {max(x[1] for x in r):20d} {sum(x[1] for x in r):10d} {sum(x[2] for x in r):3d} / {len(r):<2d} "
            f"{max(x[3] for x in r):20d} {sum(x[3] for x in r):10d} {max(x[4] for x in r):9.1e}")
    every = [x for r in rows.values() for x in r]
    say(f"   all {len(every)} cells: proven {sum(x[0] for x in every)} / {sum(x[2] for x in every)}, most nodes a cell {max(x[1] for x in every)} at width 1 "
        f"without an incumbent, {max(x[3] for x in every)} as called")
    say("")

    # ---- 4. the older entries against the parent commit -----------------------------------------------------------------------------------
    if args.parent_tree:
        say("4. slm_solve_l0_local_bound and slm_solve_l0_local (their kernels' resource lines are the parent's) through l0_local_bound and")
        say(f"   l0_local_search (max_rounds = 0) on the parent commit and on this one: whole calls, fresh processes alternating parent, change, {repeats}")
        say("   times; each warms a shape and times it 3 times.  Criterion: the change's median inside the parent's own min .. max.")
        runs = {"parent": {}, "change": {}}
        for _ in range(repeats):
            for which, tree in (("parent", args.parent_tree), ("change", ROOT)):
                got = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree], check=True, capture_output=True, text=True,
                                     timeout=600).stdout
                for key, ts in json.loads(got.strip().splitlines()[-1]).items():
                    runs[which].setdefault(key, []).extend(ts)
        say(f"{'entry | n x p | cells':>28s} {'parent ms: median (min .. max)':>36s} {'change ms: median (min .. max)':>36s} {'inside':>7s}")
        for key in runs["parent"]:
            a, b = runs["parent"][key], runs["change"][key]
            med = float(np.median(b))
            verdict = "yes" if min(a) <= med <= max(a) else ("BELOW" if med < min(a) else "ABOVE")
            say(f"{key:>28s} {fmt(a):>36s} {fmt(b):>36s} {verdict:>7s}")
        say("")
    say("NOT measured: the node kernel alone (no event bracket: the whole call is what a caller pays); sample weights; eta = 0 beyond 66 columns")
    say("(the tree does not close there); more than 64 cells; widths other than 32; devices with fewer compute units.")


if __name__ == "__main__":
    main()
