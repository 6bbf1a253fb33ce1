"""Measurements of local subsets (``slm_solve_l0_local_subsets``) for ``profiles/l0_local_subsets.txt``.

1. A sizes grid in ONE call (round 0: the zero start, ``max_rounds=0``) against the host twin ``l0_local_solve<true>`` on one core
   (``tools/l0_local_subsets_host_bench.cpp``, compiled here with g++ -O2), on the reference's 290 x 66 data and on synthetic
   400 x 1024; where it fits, against the exact ``l0_profile`` with ``wide`` (time and the gap in Q).
2. ``l0_local_subsets_cv`` with five folds against the six ``l0_local_subsets`` calls it replaces.
3. ``--parent-tree``: the penalised instantiation through ``slm_solve_l0_local`` against a built checkout of the parent commit,
   fresh processes alternating (the table and the child process of ``tools/l0_timing.py --only local-single``).

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
    "l0_local_kernel<false> (penalised)   on gfx950: 256 VGPRs,  74 AGPRs, scratch 0 bytes/lane, LDS 0, 104 SGPRs (164 SGPR spills to VGPR lanes), 1 wave/SIMD",
    "l0_local_kernel<true>  (cardinality) on gfx950: 256 VGPRs, 171 AGPRs, scratch 0 bytes/lane, LDS 0, 104 SGPRs (222 SGPR spills to VGPR lanes), 1 wave/SIMD",
    "    (the parent's l0_local_kernel:              256 VGPRs,  74 AGPRs, scratch 0,            LDS 0, 104 SGPRs, 163 SGPR spills,                   1 wave/SIMD;",
    "     the one spill more of the penalised instantiation: the stride of stat_out is an argument now)",
)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l0_local_subsets.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    args = ap.parse_args()
    repeats = max(1, args.repeats)

    from sklearn.model_selection import KFold

    from sparselm_amd import _engine
    from sparselm_amd.miqp import l0_local_subsets, l0_local_subsets_cv, l0_profile

    dev = _engine.get_engine().device_info()
    lines = [f"local subsets (l0_local_subsets, slm_solve_l0_local_subsets) on {dev['name'].strip() or 'device'}, {dev['compute_units']} compute units",
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

    exe = os.path.join(tempfile.mkdtemp(), "l0_local_subsets_host_bench")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", os.path.join(ROOT, "tools", "l0_local_subsets_host_bench.cpp"), "-o", exe],
                   check=True)

    def host(X, y, sizes, icpt):
        n, p = X.shape
        xm, ym = (X.mean(axis=0), y.mean()) if icpt else (np.zeros(p), 0.0)
        Xc, yc = X - xm, y - ym
        G, c, yy = Xc.T @ Xc / n, Xc.T @ yc / n, float(yc @ yc) / n
        path = exe + ".in"
        with open(path, "wb") as fh:
            fh.write(struct.pack("<4q2d", p, p, len(sizes), 1, yy, 100.0))
            for a in (G, c, np.asarray(sizes, dtype=np.float64), np.zeros(len(sizes))):
                fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        ts, out = [], None
        for _ in range(repeats):
            out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.splitlines()
            ts.append(float(out[0].split()[3]))
        return ts, out[0], np.array([float(v) for v in out[1].split()[1:]])

    d = os.path.join(ROOT, "tests", "golden", "reference_examples")
    Xr, yr = np.load(os.path.join(d, "corr.npy")), np.load(os.path.join(d, "energy.npy"))
    rng = np.random.default_rng(1024)
    Xw = rng.standard_normal((400, 1024))
    bw = np.zeros(1024)
    bw[rng.choice(1024, 20, replace=False)] = (-1.0) ** np.arange(20)
    yw = Xw @ bw + 0.5 * rng.standard_normal(400)

    # ---- 1. one call against the host twin, and against the exact profile where it fits ---------------------------------------------
    say("1. a sizes grid in ONE call (round 0 alone: max_rounds = 0, the zero start, big_M = 100, eta = 0) against l0_local_solve<true> on one core")
    say("   (the host time is the rule alone on a Gram it is handed; the call's includes the upload, the Gram and the polish).")
    for X, y, icpt, grids, what in ((Xr, yr, True, ([3], list(range(1, 9)), list(range(1, 33))), "the reference's 290 x 66 data, fit_intercept"),
                                    (Xw, yw, False, ([20], list(range(1, 17)), list(range(1, 65)), list(range(1, 65)) * 4),
                                     "synthetic 400 x 1024 (the law of profiles/l0_local.txt)")):
        say(what)
        say(f"{'cells':>6s} {'call ms: median (min .. max)':>34s} {'host twin ms':>34s} {'call / host':>12s}   the host's counts; max |Q - host Q| / |Q|")
        for sizes in grids:
            one = lambda: l0_local_subsets(X, y, sizes=sizes, fit_intercept=icpt, max_rounds=0)  # noqa: E731
            clock(one)
            ts, res = [], None
            for _ in range(repeats):
                res, ms = clock(one)
                ts.append(ms)
            th, counts, Qh = host(X, y, sizes, icpt)
            gap = float(np.max(np.abs(res.objectives_[:, 0] - Qh) / np.abs(Qh)))
            ratio = np.median(ts) / np.median(th)
            say(f"{len(sizes):6d} {fmt(ts):>34s} {fmt(th):>34s} {ratio:12.3f}   {counts.split(' ', 4)[4]}; {gap:.1e}" +
                ("   -- the launch LOSES" if ratio >= 1.0 else ""))
        say("")
    say("against the exact side on the 290 x 66 data (l0_profile with wide, max_groups = K, big_M = 1000, fit_intercept; proven rows only):")
    for K in (3, 4):
        prof, t_prof = clock(lambda: l0_profile(Xr, yr, max_groups=K, big_M=1000, fit_intercept=True, solver_options={"wide": True}))
        res, t_loc = clock(lambda: l0_local_subsets(Xr, yr, sizes=list(range(1, K + 1)), big_M=1000, fit_intercept=True))
        exact = np.minimum.accumulate(prof.values_)[1:]
        gaps = (res.objectives_[:, 0] - exact) / np.abs(exact)
        say(f"  K = {K}: l0_profile {t_prof:.1f} ms ({prof.solver_info_['nodes']} nodes, proven {prof.proven_optimal_}); l0_local_subsets "
            f"(sizes 1 .. {K}, {res.rounds_} rounds) {t_loc:.2f} ms; (Q - optimum) / |optimum| per size: " + ", ".join(f"{g:.2e}" for g in gaps))
    say("")

    # ---- 2. the five-fold CV call against the per-fold calls it replaces ----------------------------------------------------------------
    say("2. five folds (KFold without shuffle) and all rows, max_rounds = 2: l0_local_subsets_cv (one launch per round) against 6 calls of")
    say("   l0_local_subsets on X[rows], y[rows], each with its own dataset, upload and Gram.")
    for X, y, icpt, sizes, what in ((Xr, yr, True, list(range(1, 9)), "the reference's 290 x 66 data, fit_intercept, sizes 1 .. 8"),
                                    (Xw, yw, False, list(range(1, 17)), "synthetic 400 x 1024, sizes 1 .. 16")):
        rows = [tr for tr, _ in KFold(5).split(X)] + [np.arange(X.shape[0])]
        one = lambda: l0_local_subsets_cv(X, y, sizes=sizes, cv=KFold(5), fit_intercept=icpt)  # noqa: E731
        loop = lambda: [l0_local_subsets(X[r], y[r], sizes=sizes, fit_intercept=icpt) for r in rows]  # noqa: E731
        clock(one), clock(loop)
        t_one, t_loop, cv, paths = [], [], None, None
        for _ in range(repeats):
            cv, ms = clock(one)
            t_one.append(ms)
            paths, ms = clock(loop)
            t_loop.append(ms)
        info = cv.solver_info_
        same = sum(int(np.array_equal(a.supports_, b.supports_)) for a, b in zip(cv.paths_ + [cv.full_], paths))
        ratio = np.median(t_one) / np.median(t_loop)
        say(what)
        say(f"  l0_local_subsets_cv {fmt(t_one)} ms, {info['launches']} launches of at most {info['problems']} problems; the 6 calls {fmt(t_loop)} ms, "
            f"{sum(p_.rounds_ for p_ in paths)} launches; one-launch / loop = {ratio:.3f}" + ("  -- the one-launch call LOSES" if ratio >= 1.0 else ""))
        say(f"  row sets with the loop's supports: {same} of 6; the largest sweep count of any problem {info['max_sweeps']}, accepted swaps {info['max_swaps']}")
    say("")

    # ---- 3. the penalised instantiation against the parent commit ---------------------------------------------------------------------------
    if args.parent_tree:
        say("3. slm_solve_l0_local (the penalised instantiation, one row set) on the parent commit and on this one: whole calls, fresh processes")
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
    say("NOT measured: the kernels alone (no event bracket: the whole call is what a caller pays); eta > 0; starts beside zero in round 0; sample")
    say("weights; correlated designs at 1024 columns, where sweeps and swaps multiply; sizes beyond 64 at 1024 columns; more than five folds;")
    say("devices with fewer compute units.")


if __name__ == "__main__":
    main()
