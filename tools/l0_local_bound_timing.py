"""Measurements of the local bound (``l0_local_bound``, ``slm_solve_l0_local_bound``) for ``profiles/l0_local_bound.txt``.

1. One call beside ``l0_local_search`` (round 0 alone) on the same grids and beside its own host twin ``l0_bound_solve`` on one core
   (``tools/l0_local_bound_host_bench.cpp``, compiled here with g++ -O2 -ffp-contract=off): the reference's 290 x 66 data and synthetic 400 x 1024, at
   1 / 16 / 64 / 256 cells.
2. The relative gap of the bound to the brute-force optimum per (eta, big_M) on the hard law (30 x 10, AR(1) 0.9): where the bound is
   tight and where it is not, losses included.
3. On 290 x 66: the gap between ``l0_local_search`` and the bound next to the proven optimum of ``RegularizedL0`` at the alphas of
   ``profiles/l0_local.txt``.
4. ``--parent-tree``: ``slm_solve_l0_local`` against a built checkout of the parent commit, fresh processes alternating.

No timing is a pass criterion; the file states what was found.  Usage: ``python tools/l0_local_bound_timing.py [--repeats 5]
[--parent-tree DIR] [--out FILE]``.
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
sys.path[:0] = [os.path.join(ROOT, "sparse-lm_amd"), os.path.join(ROOT, "tests")]

# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage -c csrc/engine_l0.hip, on this commit and on its parent
RESOURCES = [
    "resource lines (the build's own remarks):",
    "    l0_local_bound_kernel          255 VGPRs +   2 AGPRs,  92 SGPR spills, no scratch, no LDS, one wave per SIMD",
    "    l0_local_kernel<false>         256 VGPRs +  74 AGPRs, 164 SGPR spills, no scratch, no LDS   (the parent's, figure for figure)",
    "    l0_local_kernel<true>          256 VGPRs + 171 AGPRs, 222 SGPR spills, no scratch, no LDS   (the parent's)",
    "    l0_local_l1_kernel             256 VGPRs +  78 AGPRs, 174 SGPR spills, no scratch, no LDS   (the parent's)",
    "    l0_local_group_kernel          256 VGPRs + 196 AGPRs, 207 SGPR spills, no scratch, 65536 B LDS   (the parent's)",
    "    (every one of the 106 kernels of the parent's engine_l0.hip, these four among them, keeps every figure of the parent's build)",
]
SWEEPS = 2000  # the cap of the timed calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l0_local_bound.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    args = ap.parse_args()
    repeats = max(1, args.repeats)

    from sparselm_amd import _engine
    from sparselm_amd.miqp import RegularizedL0, l0_local_bound, l0_local_search

    dev = _engine.get_engine().device_info()
    lines = [f"the local bound (l0_local_bound, slm_solve_l0_local_bound) on {dev['name'].strip() or 'device'}, {dev['compute_units']} compute units",
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
        return f"{np.median(ms):9.3f} ({min(ms):.3f} .. {max(ms):.3f})"

    d = os.path.join(ROOT, "tests", "golden", "reference_examples")
    Xr, yr = np.load(os.path.join(d, "corr.npy")), np.load(os.path.join(d, "energy.npy"))
    rng = np.random.default_rng(1024)
    Xw = rng.standard_normal((400, 1024))
    bw = np.zeros(1024)
    bw[rng.choice(1024, 24, replace=False)] = (-1.0) ** np.arange(24)
    yw = Xw @ bw + 0.5 * rng.standard_normal(400)

    # ---- 1. one call beside l0_local_search and beside the host twin ------------------------------------------------------------------
    exe = os.path.join(tempfile.mkdtemp(), "l0_local_bound_host_bench")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tools", "l0_local_bound_host_bench.cpp"), "-o", exe],
                   check=True)

    def host(X, y, cell_alphas, cell_etas, big_M, centre):
        n, p = X.shape
        Xc, yc = (X - X.mean(axis=0), y - y.mean()) if centre else (X, y)
        G, c = Xc.T @ Xc / n, Xc.T @ yc / n
        path_in = exe + ".in"
        with open(path_in, "wb") as fh:
            fh.write(struct.pack("<4q2d", p, p, len(cell_alphas), SWEEPS, big_M, 1e-9))
            for a in (G, c, np.asarray(cell_alphas, dtype=np.float64), np.asarray(cell_etas, dtype=np.float64)):
                fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        ts_, out = [], None
        for _ in range(repeats):
            out = subprocess.run([exe, path_in], check=True, capture_output=True, text=True).stdout.splitlines()
            ts_.append(float(out[0].split()[3]))
        return ts_, out[0], np.array([float(v) for v in out[1].split()[1:]])

    say(f"1. ONE l0_local_bound call (zero start, gap_tol 1e-9, max_sweeps {SWEEPS}) beside ONE l0_local_search call on the same grid (round 0 alone:")
    say("   max_rounds = 0) and beside l0_bound_solve on one core (the host time is the rule alone on a Gram it is handed; a call's includes the")
    say("   upload, the Gram and the read-back).  alphas: a geometric grid from 0.3 var y down to 0.003 var y, one eta per row.")
    for X, y, icpt, big_M, etas, what in ((Xr, yr, True, 100.0, (0.0, 1e-3), "the reference's 290 x 66 data, fit_intercept, big_M = 100"),
                                          (Xw, yw, False, 100.0, (0.05,), "synthetic 400 x 1024 (24 true columns, noise 0.5), big_M = 100")):
        for eta in etas:
            say(f"   {what}, eta = {eta:g}")
            say(f"{'cells':>6s} {'bound ms: median (min .. max)':>34s} {'search ms':>34s} {'host twin ms':>34s} {'bound/host':>11s}   the host's counts; "
                "max |bound - host| / max(|bound|, alpha); cells left open")
            for cells in (1, 16, 64, 256):
                al = np.geomspace(0.3, 0.003, cells) * float(np.var(y)) if cells > 1 else np.array([0.03 * float(np.var(y))])
                bound = lambda: l0_local_bound(X, y, alphas=al, etas=[eta], big_M=big_M, fit_intercept=icpt, max_sweeps=SWEEPS)  # noqa: E731
                search = lambda: l0_local_search(X, y, alphas=al, etas=[eta], big_M=big_M, fit_intercept=icpt, max_rounds=0)  # noqa: E731
                clock(bound), clock(search)
                tb, ts, res = [], [], None
                for _ in range(repeats):
                    res, ms = clock(bound)
                    tb.append(ms)
                    _, ms = clock(search)
                    ts.append(ms)
                th, counts, Lh = host(X, y, al, np.full(cells, eta), big_M, icpt)
                diff = float(np.max(np.abs(res.lower_bounds_[:, 0] - Lh) / np.maximum(np.abs(Lh), al)))
                ratio = float(np.median(tb) / np.median(th))
                say(f"{cells:6d} {fmt(tb):>34s} {fmt(ts):>34s} {fmt(th):>34s} {ratio:11.3f}   {counts}; {diff:.1e}; open {int((~res.converged_).sum())}"
                    + ("  -- the launch LOSES to one core" if ratio >= 1.0 else ""))
    say("")

    # ---- 2. how tight: the gap to the brute-force optimum per (eta, big_M) ----------------------------------------------------------------
    from _l0_local_bound_reference import ALPHAS, BIG_MS, ETAS, brute_force, hard_problem

    seeds = range(6)
    say("2. HOW TIGHT.  The hard law (30 x 10, AR(1) 0.9, 3 true columns, SNR 2), seeds 0 .. 5, alpha in {1e-3, 0.1, 0.5}: the bound of the engine")
    say("   against the brute-force optimum F* over all 1024 supports inside the box; gap = (F* - bound) / max(|F*|, alpha), 18 cells per row.")
    say(f"{'eta':>6s} {'big_M':>6s} {'median gap':>11s} {'largest gap':>12s} {'cells within 7 %':>17s} {'bound above F*':>15s} {'left open':>10s}")
    results = {}
    for seed in seeds:
        X, y, _, _ = hard_problem(seed)
        for M in BIG_MS:
            res, _ = clock(lambda: l0_local_bound(X, y, alphas=ALPHAS, etas=ETAS, big_M=M, max_sweeps=SWEEPS))
            for a, alpha in enumerate(ALPHAS):
                for e, eta in enumerate(ETAS):
                    best = brute_force(seed, alpha, eta, M)
                    results.setdefault((eta, M), []).append(((best - res.lower_bounds_[a, e]) / max(abs(best), alpha), bool(res.converged_[a, e])))
    for (eta, M), rows in sorted(results.items()):
        gaps = np.array([g for g, _ in rows])
        say(f"{eta:6g} {M:6g} {np.median(gaps):11.3e} {gaps.max():12.3e} {int((gaps <= 0.07).sum()):10d} of {len(gaps)} {int((gaps < -1e-9).sum()):15d} "
            f"{sum(not ok for _, ok in rows):10d}")
    say("   (a gap of 1 says that the bound lies max(|F*|, alpha) below the optimum: it proves nothing worth knowing there.)")
    say("")

    # ---- 3. 290 x 66: the local search, the bound and the proven optimum ------------------------------------------------------------------
    rels = np.logspace(-4, -1, 4)
    al = rels * float(np.var(yr))
    say("3. The reference's 290 x 66 data, fit_intercept, big_M = 100, eta = 0 (the RegularizedL0 objective), alphas / var y = 1e-4 .. 1e-1, the")
    say("   alphas of profiles/l0_local.txt: l0_local_search (max_rounds = 2), the bound (warm-started from it), and RegularizedL0 with wide.")
    (path, t_path) = clock(lambda: l0_local_search(Xr, yr, alphas=al, big_M=100, fit_intercept=True))
    (bound, t_bound) = clock(lambda: l0_local_bound(Xr, yr, alphas=al, big_M=100, fit_intercept=True, starts=path, max_sweeps=SWEEPS))
    gap = bound.gap(path)
    for a, alpha in enumerate(al):
        est, t_ex = clock(lambda: RegularizedL0(alpha=alpha, big_M=100, fit_intercept=True, solver_options={"wide": True, "max_nodes": 1 << 24}).fit(Xr, yr))
        info = est.solver_info_
        kind = "proven optimum" if info["proven_optimal"] else "incumbent (budget ran out)"
        say(f"    alpha / var y = {rels[a]:.1e}: local {path.objectives_[a, 0]:.10e}, bound {bound.lower_bounds_[a, 0]:.10e} (sweeps {bound.sweeps_[a, 0]}, "
            f"closed {bool(bound.converged_[a, 0])}), proven gap {gap[a, 0]:.3e}; exact {info['objective']:.10e} ({kind}, {t_ex:.1f} ms)")
    say(f"    the local search {t_path:.2f} ms, the bound {t_bound:.2f} ms (single calls after the warm-up of section 1)")
    for big_M, eta in ((100.0, 1e-3), (100.0, 1e-2), (0.5, 0.0)):
        path = l0_local_search(Xr, yr, alphas=al, etas=[eta], big_M=big_M, fit_intercept=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            bound = l0_local_bound(Xr, yr, alphas=al, etas=[eta], big_M=big_M, fit_intercept=True, starts=path, max_sweeps=SWEEPS)
        say(f"    eta = {eta:g}, big_M = {big_M:g}: proven gaps of l0_local_search {np.array2string(bound.gap(path)[:, 0], precision=3)}, closed "
            f"{bound.converged_[:, 0].tolist()}")
    say("")

    # ---- 4. slm_solve_l0_local against the parent commit ----------------------------------------------------------------------------------
    if args.parent_tree:
        say("4. slm_solve_l0_local (its kernel's resource lines are the parent's) on the parent commit and on this one: whole calls, fresh")
        say(f"   processes alternating parent, change, {repeats} times; each warms a shape and times it 3 times.  Expected: the change's medians")
        say("   inside the parent's own min .. max.")
        runs = {"parent": {}, "change": {}}
        tool = os.path.join(ROOT, "tools", "l0_timing.py")
        for _ in range(repeats):
            for which, tree in (("parent", args.parent_tree), ("change", ROOT)):
                env = dict(os.environ, PYTHONPATH=os.path.join(tree, "sparse-lm_amd"))
                got = subprocess.run([sys.executable, tool, "--only", "local-single", "--tree", tree], env=env, check=True, capture_output=True,
                                     text=True, timeout=600).stdout
                for key, ts in json.loads(got.strip().splitlines()[-1]).items():
                    runs[which].setdefault(key, []).extend(ts)
        say(f"{'n x p':>10s} {'cells':>6s} {'parent ms: median (min .. max)':>36s} {'change ms: median (min .. max)':>36s} {'inside':>7s}")
        for key in runs["parent"]:
            n_, _, p_, cells = key.split()
            a, b = runs["parent"][key], runs["change"][key]
            med = float(np.median(b))
            verdict = "yes" if min(a) <= med <= max(a) else ("BELOW" if med < min(a) else "ABOVE")
            if max(a) - min(a) > 0.5 * float(np.median(a)):  # (a parent whose own spread is half its median decides nothing)
                verdict = "NOISE"
            say(f"{f'{n_} x {p_}':>10s} {cells:>6s} {fmt(a):>36s} {fmt(b):>36s} {verdict:>7s}")
        say("")
    say("NOT measured: the kernel alone (no event bracket: the whole call is what a caller pays); sample weights; correlated designs at 1024")
    say("columns, where sweeps multiply; more than 256 cells; devices with fewer compute units.")


if __name__ == "__main__":
    main()
