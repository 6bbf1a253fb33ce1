"""Measurements of the l0 local search with groups and a hierarchy (``slm_solve_l0_local_groups``) for ``profiles/l0_local_groups.txt``.

1. Against the exact fit: ``l0_local_group_search`` on the reference's 290 x 66 data with synthetic groups of three consecutive
   columns under a chain hierarchy, against ``RegularizedL0`` (``wide`` where it needs it) at the same alphas: time and objective gap.
2. Against the host twin: synthetic 400 x 1024 in 256 groups of four, one call (round 0: the zero start) at 1, 16, 64 and 256 cells
   against ``l0_lg_solve`` on one core (``tools/l0_local_groups_host_bench.cpp``, compiled here with g++ -O2).
3. ``l0_local_group_cv`` with five folds against the six ``l0_local_group_search`` calls it replaces.
4. ``--parent-tree``: ``slm_solve_l0_local``'s single-row-set call against a built checkout of the parent commit, fresh processes
   alternating (the table and the child process of ``tools/l0_timing.py --only local-single``).

Whole calls, each ending in a synchronise; every shape warmed first; medians with min .. max.  The file grows line by line.
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
sys.path.insert(0, os.path.join(ROOT, "sparse-lm_amd"))

# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage -c csrc/engine_l0.hip
RESOURCES = (
    "l0_local_group_kernel                on gfx950: 256 VGPRs, 196 AGPRs, scratch 0 bytes/lane, LDS 65536 bytes/workgroup, 106 SGPRs (207 SGPR spills to VGPR lanes), 1 wave/SIMD",
    "l0_local_kernel<false> (penalised)   on gfx950: 256 VGPRs,  74 AGPRs, scratch 0 bytes/lane, LDS 0, 104 SGPRs (164 SGPR spills to VGPR lanes), 1 wave/SIMD",
    "l0_local_kernel<true>  (cardinality) on gfx950: 256 VGPRs, 171 AGPRs, scratch 0 bytes/lane, LDS 0, 104 SGPRs (222 SGPR spills to VGPR lanes), 1 wave/SIMD",
    "    (the two lines of l0_local_kernel are those of the parent's build, figure for figure: the kernel is untouched; the new kernel fits",
    "     without scratch)",
)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l0_local_groups.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    args = ap.parse_args()
    repeats = max(1, args.repeats)

    from sklearn.model_selection import KFold

    from sparselm_amd import _engine
    from sparselm_amd.miqp import RegularizedL0, l0_local_group_cv, l0_local_group_search

    dev = _engine.get_engine().device_info()
    lines = [f"the l0 local search with groups and a hierarchy (l0_local_group_search, slm_solve_l0_local_groups) on {dev['name'].strip() or 'device'}, "
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
        return f"{np.median(ms):9.3f} ({min(ms):.3f} .. {max(ms):.3f})"

    # ---- 1. against the exact fit on the reference's data -------------------------------------------------------------------------------
    d = os.path.join(ROOT, "tests", "golden", "reference_examples")
    Xr, yr = np.load(os.path.join(d, "corr.npy")), np.load(os.path.join(d, "energy.npy"))
    groups = np.arange(Xr.shape[1]) // 3
    ng = int(groups.max()) + 1
    chain = [[]] + [[g - 1] for g in range(1, ng)]
    alphas = [1e-3, 1e-4, 1e-5]
    say(f"1. the reference's {Xr.shape[0]} x {Xr.shape[1]} data, {ng} synthetic groups of three consecutive columns under a chain (group g needs g - 1),")
    say("   fit_intercept, big_M = 1000: l0_local_group_search over the alphas in ONE call against RegularizedL0 (wide) fit by fit.")
    one = lambda: l0_local_group_search(Xr, yr, alphas=alphas, groups=groups, hierarchy=chain, big_M=1000, fit_intercept=True)  # noqa: E731
    clock(one)
    ts, path = [], None
    for _ in range(repeats):
        path, ms = clock(one)
        ts.append(ms)
    say(f"   l0_local_group_search, {len(alphas)} alphas, {path.rounds_} rounds: {fmt(ts)} ms")
    for a, alpha in enumerate(alphas):
        est = RegularizedL0(groups=groups, alpha=alpha, hierarchy=chain, big_M=1000, fit_intercept=True, solver_options={"wide": True, "max_nodes": 1 << 26})
        _, t_exact = clock(lambda: est.fit(Xr, yr))
        info = est.solver_info_
        gap = (path.objectives_[a, 0] - info["objective"]) / abs(info["objective"])
        say(f"   alpha {alpha:.0e}: local objective {path.objectives_[a, 0]:.9e} with {int(path.n_active_groups_[a, 0])} groups, {int(path.swaps_[a, 0])} swaps, "
            f"{int(path.trials_[a, 0])} trials; RegularizedL0 {info['objective']:.9e} with {int(np.sum(est.active_groups_))} groups in {t_exact:.1f} ms "
            f"({info['nodes']} nodes, proven {info['proven_optimal']}); (local - exact) / |exact| = {gap:.2e}")
    say("")

    # ---- 2. one call against the host twin -----------------------------------------------------------------------------------------------
    exe = os.path.join(tempfile.mkdtemp(), "l0_local_groups_host_bench")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", os.path.join(ROOT, "tools", "l0_local_groups_host_bench.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(1024)
    Xw = rng.standard_normal((400, 1024))
    gw = np.arange(1024) // 4
    bw = np.zeros(1024)
    for t, g in enumerate(rng.choice(256, 12, replace=False)):
        bw[4 * g:4 * g + 4] = (-1.0) ** (t + np.arange(4))
    yw = Xw @ bw + 0.5 * rng.standard_normal(400)
    need_w = [[]] + [[g - 1] if g % 8 else [] for g in range(1, 256)]  # 32 chains of eight groups

    def host(X, y, gstart, need, cell_alphas):
        n, p = X.shape
        G, c, yy = X.T @ X / n, X.T @ y / n, float(y @ y) / n
        ptr = np.concatenate([[0], np.cumsum([len(v) for v in need])])
        idx = np.array([h for v in need for h in v], dtype=np.float64)
        path_in = exe + ".in"
        with open(path_in, "wb") as fh:
            fh.write(struct.pack("<6q2d", p, p, len(cell_alphas), 1, len(gstart) - 1, len(idx), yy, 100.0))
            for a in (G, c, np.asarray(cell_alphas, dtype=np.float64), np.zeros(len(cell_alphas)), gstart, ptr, idx):
                fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        ts_, out = [], None
        for _ in range(repeats):
            out = subprocess.run([exe, path_in], check=True, capture_output=True, text=True).stdout.splitlines()
            ts_.append(float(out[0].split()[3]))
        return ts_, out[0], np.array([float(v) for v in out[1].split()[1:]])

    say("2. synthetic 400 x 1024 in 256 groups of four (12 true groups, noise 0.5), ONE call (round 0 alone: max_rounds = 0, the zero start,")
    say("   big_M = 100, eta = 0) against l0_lg_solve on one core (the host time is the rule alone on a Gram it is handed; the call's includes the")
    say("   upload, the Gram and the polish).  alphas: a geometric grid from 0.3 var y down to 0.003 var y.")
    for need, what in ((None, "no hierarchy"), (need_w, "32 chains of eight groups")):
        say(f"   {what}")
        say(f"{'cells':>6s} {'call ms: median (min .. max)':>34s} {'host twin ms':>34s} {'call / host':>12s}   the host's counts; max (objective - host F) / |F|")
        for cells in (1, 16, 64, 256):
            al = np.geomspace(0.3, 0.003, cells) * float(np.var(yw)) if cells > 1 else np.array([0.03 * float(np.var(yw))])
            one = lambda: l0_local_group_search(Xw, yw, alphas=al, groups=gw, hierarchy=need, max_rounds=0)  # noqa: E731
            clock(one)
            ts, res = [], None
            for _ in range(repeats):
                res, ms = clock(one)
                ts.append(ms)
            th, counts, Fh = host(Xw, yw, np.arange(0, 1025, 4), need if need is not None else [[] for _ in range(256)], al)
            gap = float(np.max((res.objectives_[:, 0] - Fh) / np.maximum(np.abs(Fh), al)))
            ratio = np.median(ts) / np.median(th)
            say(f"{cells:6d} {fmt(ts):>34s} {fmt(th):>34s} {ratio:12.3f}   {counts.split(' ', 4)[4]}; {gap:.1e}" +
                ("   -- the launch LOSES" if ratio >= 1.0 else ""))
        say("")

    # ---- 3. the five-fold CV call against the per-fold calls it replaces ----------------------------------------------------------------
    say("3. five folds (KFold without shuffle) and all rows, max_rounds = 2: l0_local_group_cv (one launch per round) against 6 calls of")
    say("   l0_local_group_search on X[rows], y[rows], each with its own dataset, upload and Gram.")
    al_w = np.geomspace(0.3, 0.003, 16) * float(np.var(yw))
    for X, y, icpt, al, grp, need, what in ((Xr, yr, True, alphas, groups, chain, "the reference's 290 x 66 data, groups of three under a chain, fit_intercept"),
                                            (Xw, yw, False, al_w, gw, need_w, "synthetic 400 x 1024, groups of four, 32 chains of eight, 16 alphas")):
        rows = [tr for tr, _ in KFold(5).split(X)] + [np.arange(X.shape[0])]
        one = lambda: l0_local_group_cv(X, y, alphas=al, groups=grp, hierarchy=need, cv=KFold(5), fit_intercept=icpt)  # noqa: E731
        loop = lambda: [l0_local_group_search(X[r], y[r], alphas=al, groups=grp, hierarchy=need, fit_intercept=icpt) for r in rows]  # noqa: E731
        clock(one), clock(loop)
        t_one, t_loop, cv, paths = [], [], None, None
        for _ in range(repeats):
            cv, ms = clock(one)
            t_one.append(ms)
            paths, ms = clock(loop)
            t_loop.append(ms)
        info = cv.solver_info_
        same = sum(int(np.array_equal(a.group_supports_, b.group_supports_)) for a, b in zip(cv.paths_ + [cv.full_], paths))
        ratio = np.median(t_one) / np.median(t_loop)
        say(f"   {what}")
        say(f"     l0_local_group_cv {fmt(t_one)} ms, {info['launches']} launches of at most {info['problems']} problems; the 6 calls {fmt(t_loop)} ms, "
            f"{sum(p_.rounds_ for p_ in paths)} launches; one-launch / loop = {ratio:.3f}" + ("  -- the one-launch call LOSES" if ratio >= 1.0 else ""))
        say(f"     row sets with the loop's group supports: {same} of 6; the largest sweep count of any problem {info['max_sweeps']}, accepted swaps {info['max_swaps']}")
    say("")

    # ---- 4. slm_solve_l0_local against the parent commit -----------------------------------------------------------------------------------
    if args.parent_tree:
        say("4. slm_solve_l0_local (one row set; its kernel is untouched) on the parent commit and on this one: whole calls, fresh processes")
        say(f"   alternating parent, change, {repeats} times; each warms a shape and times it 3 times.  Expected: the change's medians inside the")
        say("   parent's own min .. max.")
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
            inside = min(a) <= med <= max(a)
            say(f"{f'{n_} x {p_}':>10s} {cells:>6s} {fmt(a):>36s} {fmt(b):>36s} {'yes' if inside else ('BELOW' if med < min(a) else 'ABOVE'):>7s}")
        say("")
    say("quality, from tests/test_l0_local_groups_cpu.py (the numpy restatement against a brute force over all closed group supports, 7 groups of 2,")
    say("n = 40, alpha in {0.02, 0.05, 0.1} var y, with and without a chain): easy law (AR(1) 0.1, SNR 20, the true groups first) 72 of 72 at the")
    say("optimum; hard law (AR(1) 0.9, SNR 2, the true groups apart) 54 of 72, never below it.")
    say("")
    say("NOT measured: the kernel alone (no event bracket: the whole call is what a caller pays); eta > 0; starts beside zero in round 0; sample")
    say("weights; correlated designs at 1024 columns, where sweeps and trials multiply; groups larger than four at 1024 columns; deep hierarchies")
    say("(a closed list of hundreds of groups is walked by one lane); more than five folds; devices with fewer compute units.")


if __name__ == "__main__":
    main()
