"""A/B of two builds of the engine on the working-set model solver (ws_solve_kernel, csrc/ws_solve_kernels.hpp): child
processes that load the library named by SLM_HIP_LIBRARY, alternating, each under its own time limit; the run stops at the
first child that does not exit cleanly.  Results only (timing: tools/ab_headline.py).

  solver cases: the cases of tests/test_model_solver_gpu.py (its builders, imported): edge sizes, non-zero counts, real groups,
                lanes / sets, direct steps, start-hard, the direct-step regimes -- z, beta, mu, Lw, every per-lane integer and
                every WMS_COUNTERS value compared bit for bit between the first library and the others;
  paths:        the headline path and config 3's group path of tools/ab_headline.py -- coefficients bit for bit, grad_launches,
                ws_inner_iters and ws_direct_steps for equality.

usage: ab_model_solver.py libA.so libB.so [...] [--out FILE]"""
import os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

CHILD = r'''
import os, sys, warnings
import numpy as np
ROOT, out_path = sys.argv[1], sys.argv[2]
sys.path[:0] = [ROOT, os.path.join(ROOT, "sparse-lm_amd"), os.path.join(ROOT, "tests")]
from bench import make_coef
from sparselm_amd import _engine
import test_model_solver_gpu as T
from _model_reference import make_case, spectrum, support_case, ws_tpc
eng = _engine.get_engine(0)
LANE_INTS = ("served", "zsup", "have_base", "zzero", "want_full", "repeats", "hard_lane", "last_point")
out = {}

def keep(tag, o):
    for name in ("z", "beta", "mu", "t", "Lw"):
        out[f"{tag}/{name}"] = getattr(o, name)
    out[tag + "/ints"] = np.stack([getattr(o, name) for name in LANE_INTS])
    out[tag + "/counters"] = np.array([getattr(o, name) for name in _engine.WMS_COUNTERS])
    out[tag + "/kernels"] = np.array(o.kernels)

for kreal in T.EDGE_SIZES:
    for cond in (10.0, 1e3):
        for preset in (False, True):
            c = make_case(kreal, 700, 100 + kreal, cond=cond, tol=1e-8, mode=kreal % 2)
            keep(f"edge_{kreal}_{cond:g}_{int(preset)}", T._solve(eng, [c], Lw=[1.05 * spectrum(c.mdl)[1]] if preset else None))
for K in (128, 272):
    tpc = ws_tpc(K)
    for nnz in (0, 1, 12 * tpc - 1, 12 * tpc, 12 * tpc + 1, 24 * tpc + 1, K):
        keep(f"nnz_{K}_{nnz}", T._solve(eng, [support_case(K, 700, nnz, 200 + K)]))
for penalty in ("group", "sparse_group", "ridged_group"):
    c = make_case(sum(T.GROUP_SIZES), 700, 320, penalty=penalty, group_sizes=T.GROUP_SIZES, tol=1e-8, strength=0.15)
    keep(f"groups_{penalty}", T._solve(eng, [c]))
for n_lanes, n_sets in ((1, 1), (5, 2), (18, 5), (32, 2), (32, 5)):
    cases = T._lanes(n_lanes, 130, 400 + n_lanes, n_sets)
    keep(f"lanes_{n_lanes}_{n_sets}", T._solve(eng, cases, set_of=np.arange(n_lanes) % n_sets,
                                                grams=np.stack([cases[s].gram for s in range(n_sets)])))
for kind in ("lasso", "group"):
    for cond in (1e6, 1e8):
        c = T._hard_case(kind, cond, 500)
        keep(f"direct_{kind}_{cond:g}", T._solve(eng, [c], direct=True))
        keep(f"hard_{kind}_{cond:g}", T._solve(eng, [c], direct=True, hard=True))
for kind, k, hard in T.REGIMES:
    keep(f"regime_{kind}_{k}", T._solve(eng, [T._regime_case(kind, k)], direct=True, hard=hard))

# the two paths of tools/ab_headline.py
n, p, K = 100000, 5000, 50
with eng.synthetic_dataset(n, p, seed=1000, coef=make_coef(p, 50, seed=0), noise_sd=10.0) as ds:
    g0, _ = ds.gradient(None)
    amax = float(np.max(np.abs(g0)))
    paths = {"headline": [(a, 0.0, 0.0) for a in np.geomspace(amax, 1e-3 * amax, K)]}
    groups = np.arange(p) // 10
    gn = np.sqrt(np.bincount(groups, weights=g0 ** 2))
    bmax = float(np.max(gn / np.sqrt(10.0)))
    paths["group"] = [(0.0, b, 0.0) for b in np.geomspace(bmax, 1e-2 * bmax, K)]
    for name, pts in paths.items():
        if name == "group":
            ds.set_groups(groups, 500)
        r = ds.solve_path(pts, lanes=0, flags=_engine.FLAG_FRESH_L)
        out[f"path_{name}/betas"] = np.asarray(r.betas)
        out[f"path_{name}/counts"] = np.array([int(r.grad_launches), int(r.ws_inner_iters), int(r.ws_direct_steps)])
np.savez(out_path, **out)
'''


def run(lib, out_path, limit=600):
    env = dict(os.environ, SLM_HIP_LIBRARY=os.path.abspath(lib))
    o = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", CHILD, ROOT, out_path], env=env, capture_output=True, text=True)
    if o.returncode != 0:  # (a fault, an abort, a time limit: nothing more is started)
        print(o.stdout[-2000:], o.stderr[-3000:])
        raise SystemExit(f"{lib}: exit status {o.returncode}; stopped")


def compare(ref, other, say):
    same = True
    for key in ref.files:
        a, b = ref[key], other[key]
        if a.dtype.kind in "iuU":
            if not np.array_equal(a, b):
                same = False
                say(f"  {key}: {a.tolist()} != {b.tolist()}")
        elif not np.array_equal(a, b, equal_nan=True):
            same = False
            say(f"  {key}: differs, largest difference {float(np.nanmax(np.abs(a - b))):.3e}")
    return same


if __name__ == "__main__":
    args = sys.argv[1:]
    out_file = None
    if "--out" in args:
        i = args.index("--out"); out_file = args[i + 1]; del args[i : i + 2]
    lines = []
    def say(text):
        print(text, flush=True); lines.append(text)
        if out_file:
            with open(out_file, "w") as f:
                f.write("\n".join(lines) + "\n")
    tmp = tempfile.mkdtemp()
    res, all_same = [], True
    for i, lib in enumerate(args):  # (in the order given: name the libraries alternately for alternating children)
        path = os.path.join(tmp, f"res{i}.npz")
        run(lib, path)
        res.append(np.load(path))
        if i == 0:
            keys = res[0].files
            say(f"{sum(k.endswith('/counters') for k in keys)} solver cases, {sum(k.endswith('/counts') for k in keys)} paths per library")
            for k in keys:
                if k.endswith("/counts"):
                    say(f"  {k} (grad_launches, ws_inner_iters, ws_direct_steps): {res[0][k].tolist()}")
            say("  direct steps, factorisations of the direct-step cases: " + " ".join(
                f"{k.split('/')[0]} {res[0][k][2]}/{res[0][k][5]}" for k in keys if k.endswith("/counters") and k[:3] in ("dir", "har", "reg")))
        else:
            same = compare(res[0], res[i], say)
            all_same = all_same and same
            say(f"{lib} (child {i}) against {args[0]}: " + ("every array and every count equal bit for bit" if same else "DIFFERENT (above)"))
    sys.exit(0 if all_same else 1)
