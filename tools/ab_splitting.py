"""A/B of two builds of the engine on the two one-launch splittings (slm_solve_standardized_sgl, slm_solve_constrained;
csrc/small_bstep.hpp): child processes that load the library named by SLM_HIP_LIBRARY, alternating, each under its own
time limit; the run stops at the first child that does not exit cleanly.

  results: every solve's arrays and counters (sweeps, products, rho, residuals, and the SLM_TRACE=2 line with the direct
           b-steps and factorisations), cold and continued, compared bit for bit between the first library and the others;
  timing:  median wall time per fit of the constrained fits of constraints_timing.py (on chip), the 100 x 80
           SparseGroupLasso(standardize=True) fit and the 25 x 30 Lasso fit of small_fit_timing.py (the control: another kernel).

usage: ab_splitting.py libA.so libB.so [...] [rounds] [--fits N] [--out FILE]   (name a library twice for its own noise)"""
import json, os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

CHILD = r'''
import os, sys, time, json, warnings
import numpy as np
ROOT, mode, out_path, fits = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4])
sys.path[:0] = [ROOT, os.path.join(ROOT, "sparse-lm_amd"), os.path.join(ROOT, "tools")]
import oracle
from sparselm_amd import _engine
from sparselm_amd.model._constrained import stack_constraints
from constraints_timing import ce_case, gauss_case
eng = _engine.get_engine(0)
INT_FIELDS, FLOAT_FIELDS = ("n_iter", "rejects", "status"), ("L", "kkt", "mu")

def feasible(n, p, m):  # (tests/test_constraints_gpu.py::_feasible_problem)
    rng = np.random.default_rng(1000 * n + 10 * p + m)
    X = rng.standard_normal((n, p))
    y = X @ np.where(rng.random(p) < 0.3, rng.standard_normal(p), 0.0) + 0.1 * rng.standard_normal(n)
    A = rng.standard_normal((m, p)) / np.sqrt(p)
    slack = np.where(rng.random(m) < 0.25, 0.0, rng.uniform(0.05, 1.0, m))
    slack[0] = 0.0
    hi = A @ (0.5 * np.linalg.lstsq(X, y, rcond=None)[0]) + slack
    lo = np.full(m, -np.inf)
    lo[0] = hi[0]
    return X, y, A, lo, hi, 0.02 * np.max(np.abs(X.T @ y)) / n

def results():
    out = {}
    def keep(tag, beta, second, rec):
        out[tag + "/beta"], out[tag + "/second"] = beta, second
        out[tag + "/ints"] = np.array([int(rec[f]) for f in INT_FIELDS])
        out[tag + "/floats"] = np.array([float(rec[f]) for f in FLOAT_FIELDS])
    rng = np.random.default_rng(5)  # (tests/test_on_chip_gpu.py::test_standardized_sparse_group_splitting_in_one_launch)
    for n, p, G in ((100, 80, 10), (25, 30, 6), (400, 100, 25), (60, 128, 16), (90, 64, 8), (90, 65, 5)):
        X = rng.standard_normal((n, p)) + 0.5 * rng.standard_normal((n, 1))
        groups = rng.permutation(np.arange(p) % G)
        cols = np.flatnonzero(groups == 0)
        X[:, cols[-1]] = 2.0 * X[:, cols[0]]
        y = X @ np.where(rng.random(p) < 0.25, rng.standard_normal(p), 0.0) + 0.2 * rng.standard_normal(n)
        gidx, GG = oracle.group_index(groups, p)
        a, b = 0.05 * rng.uniform(0.5, 1.5, p), 0.1 * rng.uniform(0.5, 1.5, GG)
        with eng.dataset(X, y) as ds:
            ds.set_groups(groups, GG)
            coef, gn, rec = ds.solve_standardized_sgl(a, b, tol=1e-11, max_sweeps=5000, want_group_norms=True)
            keep(f"sgl_{n}x{p}/cold", coef, gn, rec)
            coef, gn, rec = ds.solve_standardized_sgl(a, b, beta0=coef, warm=True, tol=1e-11, max_sweeps=5000, want_group_norms=True)
            keep(f"sgl_{n}x{p}/warm", coef, gn, rec)
    cases = [(f"cons_{n}x{p}m{m}",) + feasible(n, p, m)
             for n, p, m in ((40, 5, 1), (160, 64, 64), (160, 65, 65), (300, 128, 512), (160, 65, 1), (40, 5, 65))]
    X, y, cons, alpha = ce_case()
    st = stack_constraints(cons, X.shape[1])
    cases.append(("cons_ce", X, y, st.A, st.lo, st.hi, alpha))
    for tag, X, y, A, lo, hi, alpha in cases:
        with eng.dataset(X, y) as ds:
            beta, lam, rec = ds.solve_constrained(alpha, A, lo, hi, tol=1e-10, max_sweeps=5000)
            keep(tag + "/cold", beta, lam, rec)
            beta, lam, rec = ds.solve_constrained(alpha, A, lo, hi, beta0=beta, warm=True, tol=1e-10, max_sweeps=5000)
            keep(tag + "/warm", beta, lam, rec)
    np.savez(out_path, **out)

def median_ms(fit):
    fit()
    ts = []
    for _ in range(fits):
        t0 = time.perf_counter(); fit(); ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))

def timing():
    from sklearn.datasets import make_regression
    from sparselm_amd.model import AdaptiveLasso, Lasso, SparseGroupLasso
    out = {}
    for name, (X, y, cons, alpha) in (("ce_290x66", ce_case()), ("gauss_100x80", gauss_case())):
        for cls in (Lasso, AdaptiveLasso):
            est = cls(alpha=alpha, constraints=cons).fit(X, y)
            assert est.solver_info_["route"] == "on_chip"
            out[f"{name}_{cls.__name__}_ms"] = median_ms(lambda: cls(alpha=alpha, constraints=cons).fit(X, y))
    Xr, yr = make_regression(n_samples=100, n_features=80, n_informative=10, random_state=0)
    out["standardized_sgl_fit_100x80_ms"] = median_ms(
        lambda: SparseGroupLasso(groups=np.arange(80) // 8, alpha=0.5, standardize=True, fit_intercept=True).fit(Xr, yr))
    Xs, ys = make_regression(n_samples=25, n_features=30, n_informative=10, random_state=1)
    out["lasso_fit_25x30_ms"] = median_ms(lambda: Lasso(alpha=0.1).fit(Xs, ys))
    with open(out_path, "w") as f:
        json.dump(out, f)

warnings.simplefilter("ignore")
results() if mode == "results" else timing()
'''


def run(lib, mode, out_path, fits, limit):
    env = dict(os.environ, SLM_HIP_LIBRARY=os.path.abspath(lib))
    env.pop("SLM_TRACE", None)
    if mode == "results":
        env["SLM_TRACE"] = "2"
    o = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", CHILD, ROOT, mode, out_path, str(fits)],
                       env=env, capture_output=True, text=True)
    if o.returncode != 0:  # (a fault, an abort, a time limit: nothing more is started)
        print(o.stdout[-2000:], o.stderr[-3000:])
        raise SystemExit(f"{lib} ({mode}): exit status {o.returncode}; stopped")
    return [l for l in o.stderr.splitlines() if l.startswith("[slm]") and "splitting on chip" in l]


def compare(ref, other, trace_ref, trace_other, say):
    same = True
    for key in ref.files:
        a, b = ref[key], other[key]
        if key.endswith("/ints"):
            if not np.array_equal(a, b):
                same = False
                say(f"  {key}: {a.tolist()} != {b.tolist()}")
        elif not np.array_equal(a, b):
            same = False
            rel = float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(a))), 1e-300))
            say(f"  {key}: differs, largest difference {rel:.3e} of the largest entry")
    if trace_ref != trace_other:
        same = False
        for x, y in zip(trace_ref, trace_other):
            if x != y:
                say(f"  trace: {x}\n     !=  {y}")
    return same


if __name__ == "__main__":
    args = sys.argv[1:]
    fits, out_file = 30, None
    if "--fits" in args:
        i = args.index("--fits"); fits = int(args[i + 1]); del args[i : i + 2]
    if "--out" in args:
        i = args.index("--out"); out_file = args[i + 1]; del args[i : i + 2]
    libs = [x for x in args if not x.isdigit()]
    rounds = int(args[-1]) if args[-1].isdigit() else 3
    lines = []
    def say(text):
        print(text, flush=True); lines.append(text)
        if out_file:
            with open(out_file, "w") as f:
                f.write("\n".join(lines) + "\n")
    tmp = tempfile.mkdtemp()
    # results: once per distinct library
    distinct = list(dict.fromkeys(libs))
    res, trace = {}, {}
    for lib in distinct:
        path = os.path.join(tmp, f"res{len(res)}.npz")
        trace[lib] = run(lib, "results", path, fits, 300)
        res[lib] = np.load(path)
    say(f"results: {len(res[distinct[0]].files) // 4} solves, {len(trace[distinct[0]])} trace lines per library")
    for line in trace[distinct[0]]:
        say("  " + line)
    for lib in distinct[1:]:
        same = compare(res[distinct[0]], res[lib], trace[distinct[0]], trace[lib], say)
        say(f"{lib} against {distinct[0]}: " + ("every array and every counter equal" if same else "DIFFERENT (above)"))
    # timing: alternating; a library named twice is two legs
    legs = [f"{os.path.basename(os.path.dirname(os.path.abspath(l)))}/{os.path.basename(l)}#{i}" for i, l in enumerate(libs)]
    times = {leg: [] for leg in legs}
    for r in range(rounds):
        for leg, lib in zip(legs, libs):
            path = os.path.join(tmp, "timing.json")
            run(lib, "timing", path, fits, 300)
            with open(path) as f:
                times[leg].append(json.load(f))
            say(f"round {r} {leg} " + json.dumps({k: round(v, 4) for k, v in times[leg][-1].items()}))
    say(f"median ms per fit over {fits} fits, one column per round; spread = largest - smallest of a leg's rounds")
    for key in times[legs[0]][0]:
        for leg in legs:
            v = [t[key] for t in times[leg]]
            say(f"{key:>34} {leg:>28}: " + " ".join(f"{x:8.4f}" for x in v) + f"   median {np.median(v):8.4f}  spread {max(v) - min(v):.4f}")
