"""Measurements of the l0 local search with an l1 term (``slm_solve_l0_local_l1``) for ``profiles/l1l0_local.txt``.

1. Against the host twin: ONE call (round 0: the zero start) at 1, 16, 64 and 256 cells against ``l0_local_solve<false, true>`` on one
   core (``tools/l1l0_local_host_bench.cpp``, compiled here with g++ -O2), at the reference's 290 x 66 data and at synthetic 400 x 1024.
2. The l1 entry with every lam = 0 against ``slm_solve_l0_local_folds`` on the same cells, alternating in one process: what the l1
   kernel costs beside the penalised one.
3. The reference's 290 x 66 data against the exact side: ``L1L0`` where it fits (66 columns do not: its refusal is written down), and
   ``l1l0_profile`` with ``wide`` and ``max_groups = 16`` (wide mode keeps at most 64 sizes; the local winners hold a few columns), with
   the gap (local - profile) / |profile| per alpha.
4. ``l1l0_local_cv`` with five folds against the six ``l1l0_local_search`` calls it replaces.
5. ``--parent-tree``: ``slm_solve_l0_local``'s single-row-set call against a built checkout of the parent commit, fresh processes
   alternating (the table and the child process of ``tools/l0_timing.py --only local-single``).

Whole calls, each ending in a synchronise; every shape warmed first; medians with min .. max.  The file grows line by line; a row
where the launch loses is written down like any other.
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

# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage -c csrc/engine_l0.hip, on this commit and on its parent
RESOURCES = (
    "l0_local_l1_kernel (the l1 rule)      on gfx950: 256 VGPRs,  78 AGPRs, scratch 0 bytes/lane, LDS 0, 174 SGPR spills to VGPR lanes, 0 VGPR spills, 1 wave/SIMD",
    "l0_local_kernel<false> (penalised)   on gfx950: 256 VGPRs,  74 AGPRs, scratch 0 bytes/lane, LDS 0, 164 SGPR spills to VGPR lanes, 0 VGPR spills, 1 wave/SIMD",
    "l0_local_kernel<true>  (cardinality) on gfx950: 256 VGPRs, 171 AGPRs, scratch 0 bytes/lane, LDS 0, 222 SGPR spills to VGPR lanes, 0 VGPR spills, 1 wave/SIMD",
    "l0_local_group_kernel                on gfx950: 256 VGPRs, 196 AGPRs, scratch 0 bytes/lane, LDS 65536 bytes/workgroup, 207 SGPR spills, 0 VGPR spills, 1 wave/SIMD",
    "    (the three older kernels' lines are those of the parent's build, figure for figure.  The body of l0_local_kernel is a text included",
    "     by its kernels, not a function: as a function inlined into thin kernels the same text compiled to 108 and 203 AGPRs)",
)


WIDE_SIZES = 16  # max_groups of the wide l1l0_profile call of section 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l1l0_local.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    args = ap.parse_args()
    repeats = max(1, args.repeats)

    from sklearn.model_selection import KFold

    from sparselm_amd import _engine
    from sparselm_amd.miqp import L1L0, l1l0_local_cv, l1l0_local_search, l1l0_profile

    dev = _engine.get_engine().device_info()
    lines = [f"the l0 local search with an l1 term (l1l0_local_search, slm_solve_l0_local_l1) on {dev['name'].strip() or 'device'}, "
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

    d = os.path.join(ROOT, "tests", "golden", "reference_examples")
    Xr, yr = np.load(os.path.join(d, "corr.npy")), np.load(os.path.join(d, "energy.npy"))
    rng = np.random.default_rng(1024)
    Xw = rng.standard_normal((400, 1024))
    bw = np.zeros(1024)
    bw[rng.choice(1024, 24, replace=False)] = (-1.0) ** np.arange(24)
    yw = Xw @ bw + 0.5 * rng.standard_normal(400)

    # ---- 1. one call against the host twin -----------------------------------------------------------------------------------------------
    exe = os.path.join(tempfile.mkdtemp(), "l1l0_local_host_bench")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", os.path.join(ROOT, "tools", "l1l0_local_host_bench.cpp"), "-o", exe], check=True)

    def host(X, y, cell_alphas, cell_l1s, big_M, centre):
        n, p = X.shape
        Xc, yc = (X - X.mean(axis=0), y - y.mean()) if centre else (X, y)
        G, c, yy = Xc.T @ Xc / n, Xc.T @ yc / n, float(yc @ yc) / n
        path_in = exe + ".in"
        with open(path_in, "wb") as fh:
            fh.write(struct.pack("<4q2d", p, p, len(cell_alphas), 1, yy, big_M))
            for a in (G, c, np.asarray(cell_alphas, dtype=np.float64), np.asarray(cell_l1s, dtype=np.float64), np.zeros(len(cell_alphas))):
                fh.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        ts_, out = [], None
        for _ in range(repeats):
            out = subprocess.run([exe, path_in], check=True, capture_output=True, text=True).stdout.splitlines()
            ts_.append(float(out[0].split()[3]))
        return ts_, out[0], np.array([float(v) for v in out[1].split()[1:]])

    say("1. ONE call (round 0 alone: max_rounds = 0, the zero start, ridge = 0) against l0_local_solve<false, true> on one core (the host time")
    say("   is the rule alone on a Gram it is handed; the call's includes the upload, the Gram and the polish).  alphas: a geometric grid from")
    say("   0.3 var y down to 0.003 var y; one eta (the l1 weight) per data set.")
    for X, y, icpt, big_M, eta, what in ((Xr, yr, True, 1000.0, 1e-4 * float(np.std(yr)), "the reference's 290 x 66 data, fit_intercept, big_M = 1000"),
                                         (Xw, yw, False, 100.0, 0.05, "synthetic 400 x 1024 (24 true columns, noise 0.5), big_M = 100")):
        say(f"   {what}, eta = {eta:.3g}")
        say(f"{'cells':>6s} {'call ms: median (min .. max)':>34s} {'host twin ms':>34s} {'call / host':>12s}   the host's counts; max (objective - host F) / |F|")
        for cells in (1, 16, 64, 256):
            al = np.geomspace(0.3, 0.003, cells) * float(np.var(y)) if cells > 1 else np.array([0.03 * float(np.var(y))])
            one = lambda: l1l0_local_search(X, y, alphas=al, etas=[eta], big_M=big_M, fit_intercept=icpt, max_rounds=0)  # noqa: E731
            clock(one)
            ts, res = [], None
            for _ in range(repeats):
                res, ms = clock(one)
                ts.append(ms)
            th, counts, Fh = host(X, y, al, np.full(cells, eta), big_M, icpt)
            gap = float(np.max((res.objectives_[:, 0] - Fh) / np.maximum(np.abs(Fh), al)))
            ratio = np.median(ts) / np.median(th)
            say(f"{cells:6d} {fmt(ts):>34s} {fmt(th):>34s} {ratio:12.3f}   {counts.split(' ', 4)[4]}; {gap:.1e}" +
                ("   -- the launch LOSES" if ratio >= 1.0 else ""))
        say("")

    # ---- 2. every lam = 0 against the penalised entry ------------------------------------------------------------------------------------
    say("2. slm_solve_l0_local_l1 with every lam = 0 against slm_solve_l0_local_folds on the same cells (one row set, the zero start),")
    say("   alternating in one process on one dataset, the Gram filed before the clock starts: what the l1 kernel and its polish cost beside the")
    say("   penalised ones.  The decisions are the same (tests/test_l1l0_local_gpu.py); the times should be about equal.")
    say(f"{'n x p':>10s} {'cells':>6s} {'penalised ms: median (min .. max)':>36s} {'l1 entry ms: median (min .. max)':>36s} {'l1 / penalised':>15s}")
    for X, y, what in ((Xr - Xr.mean(axis=0), yr - yr.mean(), "290 x 66"), (Xw, yw, "400 x 1024")):
        with _engine.get_engine().dataset(X, y) as ds:
            for cells in (1, 16, 64, 256):
                al = np.geomspace(0.3, 0.003, cells) * float(np.var(y)) if cells > 1 else np.array([0.03 * float(np.var(y))])
                zero = np.zeros(cells)
                pen = lambda: ds.solve_l0_local_folds([None], [0], al, zero, big_M=1000.0)  # noqa: E731
                l1e = lambda: ds.solve_l0_local_l1([None], [0], al, zero, zero, big_M=1000.0)  # noqa: E731
                clock(pen), clock(l1e)
                ta, tb = [], []
                for _ in range(3 * repeats):
                    ta.append(clock(pen)[1])
                    tb.append(clock(l1e)[1])
                say(f"{what:>10s} {cells:6d} {fmt(ta):>36s} {fmt(tb):>36s} {np.median(tb) / np.median(ta):15.3f}")
    say("")

    # ---- 3. against the exact side on the reference's data -------------------------------------------------------------------------------
    alphas = [1e-3, 1e-4, 1e-5]
    eta = 1e-4 * float(np.std(yr))
    say(f"3. the reference's {Xr.shape[0]} x {Xr.shape[1]} data, fit_intercept, big_M = 1000, eta = {eta:.3g}: l1l0_local_search over the alphas in ONE call")
    say("   against the exact side: L1L0 fit by fit where it fits (66 columns are beyond its 64: it refuses, and the line says so), and")
    say(f"   l1l0_profile with wide and max_groups = {WIDE_SIZES} (wide mode keeps at most 64 sizes), which answers every alpha >= alpha_min over")
    say("   the supports of up to that many columns from one search under a node budget.  A gap below zero is a loss of the profile's: its")
    say("   budget ran out and the row compares incumbents, not optima.")
    one = lambda: l1l0_local_search(Xr, yr, alphas=alphas, etas=[eta], big_M=1000, fit_intercept=True)  # noqa: E731
    clock(one)
    ts, path = [], None
    for _ in range(repeats):
        path, ms = clock(one)
        ts.append(ms)
    say(f"   l1l0_local_search, {len(alphas)} alphas, {path.rounds_} rounds: {fmt(ts)} ms")
    try:
        est = L1L0(alpha=alphas[0], eta=eta, big_M=1000, fit_intercept=True, solver_options={"max_nodes": 1 << 22})
        _, t_exact = clock(lambda: est.fit(Xr, yr))
        say(f"   L1L0 at alpha {alphas[0]:.0e}: objective {est.solver_info_['objective']:.9e} in {t_exact:.1f} ms, proven {est.solver_info_['proven_optimal']}")
    except Exception as exc:  # (the refusal is the measurement)
        say(f"   L1L0 at 66 columns: refused -- {type(exc).__name__}: {str(exc)[:150]}")
    try:
        wide = lambda: l1l0_profile(Xr, yr, eta=eta, max_groups=WIDE_SIZES, alpha_min=min(alphas), big_M=1000, fit_intercept=True,  # noqa: E731
                                    solver_options={"wide": True, "max_nodes": 1 << 24})
        clock(wide)
        prof, t_prof = clock(wide)
        info = prof.solver_info_
        say(f"   l1l0_profile(wide, max_groups = {WIDE_SIZES}, alpha_min = {min(alphas):.0e}, max_nodes = 2^24), the second of two calls: {t_prof:.1f} ms, "
            f"{info['nodes']} nodes, status {info['status']}, proven {info['proven_optimal']}")
        for a, alpha in enumerate(alphas):
            k = int(np.argmin(prof.values_ + alpha * np.arange(len(prof.values_))))
            exact = float(prof.values_[k] + alpha * k)
            gap = (path.objectives_[a, 0] - exact) / abs(exact)
            say(f"   alpha {alpha:.0e}: local objective {path.objectives_[a, 0]:.9e} with {int(path.supports_[a, 0].sum())} columns, {int(path.swaps_[a, 0])} swaps; "
                f"profile {exact:.9e} at size {k}" + (" (the cap)" if k == WIDE_SIZES else "") + f"; (local - profile) / |profile| = {gap:.2e}")
    except Exception as exc:
        say(f"   l1l0_profile(wide): {type(exc).__name__}: {str(exc)[:150]}")
        for a, alpha in enumerate(alphas):
            say(f"   alpha {alpha:.0e}: local objective {path.objectives_[a, 0]:.9e} with {int(path.supports_[a, 0].sum())} columns, {int(path.swaps_[a, 0])} swaps")
    say("")

    # ---- 4. the five-fold CV call against the per-fold calls it replaces ----------------------------------------------------------------
    say("4. five folds (KFold without shuffle) and all rows, max_rounds = 2: l1l0_local_cv (one launch per round) against 6 calls of")
    say("   l1l0_local_search on X[rows], y[rows], each with its own dataset, upload and Gram.")
    al_w = np.geomspace(0.3, 0.003, 16) * float(np.var(yw))
    for X, y, icpt, al, et, what in ((Xr, yr, True, alphas, [eta, 10 * eta], "the reference's 290 x 66 data, 3 alphas x 2 etas, fit_intercept"),
                                     (Xw, yw, False, al_w, [0.02, 0.1], "synthetic 400 x 1024, 16 alphas x 2 etas")):
        rows = [tr for tr, _ in KFold(5).split(X)] + [np.arange(X.shape[0])]
        one = lambda: l1l0_local_cv(X, y, alphas=al, etas=et, cv=KFold(5), fit_intercept=icpt, big_M=1000)  # noqa: E731
        loop = lambda: [l1l0_local_search(X[r], y[r], alphas=al, etas=et, fit_intercept=icpt, big_M=1000) for r in rows]  # noqa: E731
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
        say(f"   {what}")
        say(f"     l1l0_local_cv {fmt(t_one)} ms, {info['launches']} launches of at most {info['problems']} problems; the 6 calls {fmt(t_loop)} ms, "
            f"{sum(p_.rounds_ for p_ in paths)} launches; one-launch / loop = {ratio:.3f}" + ("  -- the one-launch call LOSES" if ratio >= 1.0 else ""))
        say(f"     row sets with the loop's supports: {same} of 6; the largest sweep count of any problem {info['max_sweeps']}, accepted swaps {info['max_swaps']}")
    say("")

    # ---- 5. slm_solve_l0_local against the parent commit -----------------------------------------------------------------------------------
    if args.parent_tree:
        say("5. slm_solve_l0_local (one row set; its kernel's resource lines are the parent's) on the parent commit and on this one: whole calls,")
        say(f"   fresh processes alternating parent, change, {repeats} times; each warms a shape and times it 3 times.  Expected: the change's medians")
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
        noisy = 0
        for key in runs["parent"]:
            n_, _, p_, cells = key.split()
            a, b = runs["parent"][key], runs["change"][key]
            med = float(np.median(b))
            inside = min(a) <= med <= max(a)
            verdict = "yes" if inside else ("BELOW" if med < min(a) else "ABOVE")
            if max(a) - min(a) > 0.5 * float(np.median(a)):  # (a parent whose own spread is half its median decides nothing)
                verdict, noisy = "NOISE", noisy + 1
            say(f"{f'{n_} x {p_}':>10s} {cells:>6s} {fmt(a):>36s} {fmt(b):>36s} {verdict:>7s}")
        if noisy:
            say(f"   NOISE: the parent's own max - min is more than half its median in {noisy} row(s): such a row is no evidence either way.  (At 256 cells")
            say("   of 1024 columns a call brings 2 MB back; in a fresh process some of the first such calls take 20 - 40 ms on either commit, and")
            say("   3 ms once the process has made a few -- section 2 times that shape in one warm process.)")
        say("")
    say("quality, from tests/test_l1l0_local_cpu.py (the numpy restatement against a brute force over all supports with a lasso on each; the hard")
    say("law AR(1) 0.9, SNR 2, n = 30, p = 10, 3 true columns, seeds 0 .. 11, alpha in {0.2, 0.05, 0.01} var y, lam in {0.02, 0.1}): the full rule at")
    say("the optimum in 48 of 72 cases, the descent alone in 23, never below it; 35 cases took swaps; the smallest decision margin 1.1e-4.")
    say("")
    say("NOT measured: the kernel alone (no event bracket: the whole call is what a caller pays); ridge > 0; starts beside zero in round 0; sample")
    say("weights; correlated designs at 1024 columns, where sweeps multiply; more than five folds; devices with fewer compute units.")


if __name__ == "__main__":
    main()
