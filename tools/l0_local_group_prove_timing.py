"""Measurements of the local proof with groups (``l0_local_group_prove``, ``slm_solve_l0_local_group_prove``) for
``profiles/l0_local_group_prove.txt``.

1. Whole calls on the reference's 290 x 66 data (22 groups of three under a chain), on a 120 x 160 draw (40 groups of four) and on a
   400 x 1024 draw (256 groups of four), beside the host twin on one core (``tools/l0_local_group_prove_host_bench.cpp``:
   ``l0_prove_tree`` with a group map and ``l0_group_node_solve``, compiled here with g++ -O2 -ffp-contract=off) and, at 66 columns,
   beside the exact ``L2L0`` fit with the same groups and hierarchy (``wide``).
2. ``--parent-tree``: ``slm_solve_l0_local_prove``, ``slm_solve_l0_local_bound`` and ``slm_solve_l0_local_groups`` against a built
   checkout of the parent commit, fresh processes alternating; the criterion is "inside the parent's own min .. max".

No timing is a pass criterion; the file states what was found, losses included.  Usage: ``python tools/l0_local_group_prove_timing.py
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
    "    l0_local_group_node_kernel     256 VGPRs + 212 AGPRs, 471 SGPR spills, no scratch, 65536 B LDS, one wave per SIMD",
    "    l0_local_node_kernel           256 VGPRs +  12 AGPRs, 135 SGPR spills, no scratch, no LDS   (the parent's, figure for figure)",
    "    l0_local_bound_kernel          255 VGPRs +   2 AGPRs,  92 SGPR spills, no scratch, no LDS   (the parent's)",
    "    l0_local_group_kernel          256 VGPRs + 196 AGPRs, 207 SGPR spills, no scratch, 65536 B LDS   (the parent's)",
]
REL_GAP = 1e-6
HOST_LIMIT = 150  # seconds the host twin gets for one row


def shapes():
    """(name, X, y, groups, hierarchy, eta, fit_intercept, max_nodes) of the three runs."""
    d = os.path.join(ROOT, "tests", "golden", "reference_examples")
    Xr, yr = np.load(os.path.join(d, "corr.npy")), np.load(os.path.join(d, "energy.npy"))
    rng = np.random.default_rng(0)
    Z = rng.standard_normal((120, 160))
    Xd = Z.copy()
    for j in range(1, 160):
        Xd[:, j] = 0.5 * Xd[:, j - 1] + np.sqrt(0.75) * Z[:, j]
    bd = np.zeros(160)
    for g in rng.choice(40, 3, replace=False):
        bd[4 * g:4 * g + 4] = (-1.0) ** np.arange(4)
    sd = Xd @ bd
    yd = sd + np.sqrt(np.var(sd) / 4.0) * rng.standard_normal(120)
    rng = np.random.default_rng(1024)
    Xw = rng.standard_normal((400, 1024))
    bw = np.zeros(1024)
    for g in rng.choice(256, 6, replace=False):
        bw[4 * g:4 * g + 4] = (-1.0) ** np.arange(4)
    yw = Xw @ bw + 0.5 * rng.standard_normal(400)
    chain = [[]] + [[g - 1] for g in range(1, 22)]
    return [("290 x 66, 22 groups of three under a chain, fit_intercept", Xr, yr, np.arange(66) // 3, chain, 0.01, True, 4000),
            ("120 x 160, 40 groups of four", Xd, yd, np.arange(160) // 4, None, 0.1, False, 4000),
            ("400 x 1024, 256 groups of four", Xw, yw, np.arange(1024) // 4, None, 0.05, False, 400)]


def child(tree):
    """One process of the parent comparison: whole calls of three older entries on the package of ``tree``."""
    sys.path.insert(0, os.path.join(tree, "sparse-lm_amd"))
    from sparselm_amd.miqp import l0_local_bound, l0_local_group_search, l0_local_prove

    (_, Xr, yr, gr, hr, _, _, _), (_, Xd, yd, _, _, _, _, _), _ = shapes()
    al = np.geomspace(0.1, 0.01, 16) * float(np.var(yr))
    ad = np.geomspace(0.1, 0.01, 16) * float(np.var(yd))
    runs = {"prove | 120 x 160 | 16": lambda: l0_local_prove(Xd, yd, alphas=ad, etas=[0.1], big_M=100.0, max_nodes=4000),
            "bound | 290 x 66 | 16": lambda: l0_local_bound(Xr, yr, alphas=al, etas=[1e-3], big_M=100.0, fit_intercept=True, max_sweeps=2000),
            "groups | 290 x 66 | 16": lambda: l0_local_group_search(Xr, yr, alphas=al, etas=[0.01], groups=gr, hierarchy=hr, big_M=100.0,
                                                                    fit_intercept=True)}
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for key, fn in runs.items():
            fn()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            out[key] = ts
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l0_local_group_prove.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--child", default=None, help="internal: time the older entries on the package of this checkout and print JSON")
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    repeats = max(1, args.repeats)
    sys.path[:0] = [os.path.join(ROOT, "sparse-lm_amd")]

    from sparselm_amd import _engine
    from sparselm_amd.miqp import L2L0, l0_local_group_prove, l0_local_group_search

    dev = _engine.get_engine().device_info()
    lines = [f"the local proof with groups (l0_local_group_prove, slm_solve_l0_local_group_prove) on {dev['name'].strip() or 'device'}, "
             f"{dev['compute_units']} compute units",
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

    exe = os.path.join(tempfile.mkdtemp(), "l0_local_group_prove_host_bench")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off",
                    os.path.join(ROOT, "tools", "l0_local_group_prove_host_bench.cpp"), "-o", exe], check=True)

    def host(X, y, groups, hierarchy, cell_alphas, cell_etas, centre, incumbents, max_nodes):
        n, p = X.shape
        Xc, yc = (X - X.mean(axis=0), y - y.mean()) if centre else (X, y)
        G, c = Xc.T @ Xc / n, Xc.T @ yc / n
        ng = int(groups.max()) + 1
        gstart = np.searchsorted(groups, np.arange(ng + 1))
        lists = [[] for _ in range(ng)] if hierarchy is None else hierarchy
        ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])])
        idx = np.array([h for v in lists for h in v], dtype=np.int64)
        path_in = exe + ".in"
        with open(path_in, "wb") as fh:
            fh.write(struct.pack("<8q2d", p, len(cell_alphas), max_nodes, 32, 10000, 1, ng, len(idx), 100.0, REL_GAP))
            for a in (gstart, ptr, idx):
                fh.write(np.ascontiguousarray(a, dtype=np.int64).tobytes())
            for a in (G, c, np.asarray(cell_alphas, dtype=np.float64), np.asarray(cell_etas, dtype=np.float64), incumbents):
                fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        try:
            out = subprocess.run([exe, path_in], check=True, capture_output=True, text=True, timeout=HOST_LIMIT).stdout.splitlines()
        except subprocess.TimeoutExpired:
            return float("nan"), f"(the host twin was stopped after {HOST_LIMIT} s)"
        return float(out[0].split()[3]), out[0]

    say(f"1. ONE l0_local_group_prove call (rel_gap {REL_GAP:g}, width 32, big_M = 100, the incumbents from an L0LocalGroupPath computed before")
    say("   the clock starts: path=) beside l0_prove_tree with l0_group_node_solve on ONE core (once per row; the host time is the tree alone on a")
    say("   Gram it is handed, a call's includes the upload, the Gram, its download for the tree and every round's copies).  alphas: a geometric")
    say("   grid from 0.1 var y down to 0.01 var y (one cell: 0.03 var y).")
    for name, X, y, groups, hierarchy, eta, icpt, max_nodes in shapes():
        say(f"   {name}, eta = {eta:g}, max_nodes = {max_nodes}")
        say(f"{'cells':>6s} {'prove ms: median (min .. max)':>34s} {'host twin ms':>13s} {'prove/host':>11s} {'proven':>9s} {'nodes':>8s} "
            f"{'most a cell':>12s} {'rounds':>7s} {'worst gap':>10s}   the host's line")
        for cells in (1, 16):
            al = np.geomspace(0.1, 0.01, cells) * float(np.var(y)) if cells > 1 else np.array([0.03 * float(np.var(y))])
            kw = dict(alphas=al, etas=[eta], groups=groups, hierarchy=hierarchy, big_M=100.0, fit_intercept=icpt)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                path = l0_local_group_search(X, y, **kw)
            prove = lambda: l0_local_group_prove(X, y, path=path, rel_gap=REL_GAP, max_nodes=max_nodes, **kw)  # noqa: E731
            clock(prove)
            tp, res = [], None
            for _ in range(repeats):
                res, ms = clock(prove)
                tp.append(ms)
            th, line = host(X, y, groups, hierarchy, al, np.full(cells, eta), icpt, path.coefs_[:, 0], max_nodes)
            ratio = float(np.median(tp) / th)
            say(f"{cells:6d} {fmt(tp):>34s} {th:13.2f} {ratio:11.3f} {int(res.proven_optimal_.sum()):4d} / {cells:<3d} {int(res.nodes_.sum()):8d} "
                f"{int(res.nodes_.max()):12d} {int(res.rounds_.max()):7d} {float(res.gaps_.max()):10.2e}   {line}"
                + ("  -- the call LOSES to one core" if ratio >= 1.0 else ""))
        if X.shape[1] == 66:
            al = np.array([0.01, 0.1]) * float(np.var(y))
            kw = dict(alphas=al, etas=[eta], groups=groups, hierarchy=hierarchy, big_M=100.0, fit_intercept=True)
            path = l0_local_group_search(X, y, **kw)
            res, ms = clock(lambda: l0_local_group_prove(X, y, path=path, max_nodes=max_nodes, **kw))
            for a, alpha in enumerate(al):
                est = L2L0(groups=groups, alpha=alpha, eta=eta, hierarchy=hierarchy, big_M=100, fit_intercept=True,
                           solver_options={"wide": True, "max_nodes": 1 << 24})
                clock(lambda: est.fit(X, y))
                _, t_ex = clock(lambda: est.fit(X, y))
                info = est.solver_info_
                say(f"    alpha / var y = {alpha / np.var(y):.2g}: proof {res.objectives_[a, 0]:.10e} bound {res.lower_bounds_[a, 0]:.10e} nodes "
                    f"{res.nodes_[a, 0]} rounds {res.rounds_[a, 0]} {res.status_[a, 0]}; exact (wide) {info['objective']:.10e} "
                    f"{'proven' if info['proven_optimal'] else 'NOT proven'} in {t_ex:.1f} ms; group search {path.objectives_[a, 0]:.10e}")
            say(f"    (the two-cell proof call: {ms:.1f} ms)")
    say("")

    if args.parent_tree:
        say("2. slm_solve_l0_local_prove, slm_solve_l0_local_bound and slm_solve_l0_local_groups (their kernels' resource lines are the parent's)")
        say(f"   through l0_local_prove, l0_local_bound and l0_local_group_search on the parent commit and on this one: whole calls, fresh processes")
        say(f"   alternating parent, change, {repeats} times; each warms a shape and times it 3 times.  Criterion: the change's median inside the")
        say("   parent's own min .. max.")
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
    say("NOT measured: the group node kernel alone (no event bracket: the whole call is what a caller pays); sample weights; eta = 0 (the tree")
    say("does not close under a loose box); more than 16 cells; widths other than 32; devices with fewer compute units.")


if __name__ == "__main__":
    main()
