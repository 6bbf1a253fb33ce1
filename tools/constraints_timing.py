"""Linear constraints: wall time per fit of the on-chip splitting (slm_solve_constrained, one launch) and of the host
sweeps (``solver_options={"on_chip": False}``), with the sweeps, the route each fit took and the two routes' distance.

Problems: the reference's cluster-expansion data (tests/golden/reference_examples: 290 x 66) with non-negativity on
the first coefficients, 100 hull-like inequalities and one equality (the shape of examples/plot_chull.py:160-185), for
Lasso and AdaptiveLasso; and a 100 x 80 Gaussian design with bounds, 20 inequalities and one equality.
`python tools/constraints_timing.py [repeats]` prints one JSON line per case.
"""
import json
import os
import sys
import time
import warnings

import numpy as np
from scipy.optimize import Bounds, LinearConstraint

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "sparse-lm_amd"))

from sparselm_amd.model import AdaptiveLasso, Lasso  # noqa: E402
from sparselm_amd.model._constrained import stack_constraints  # noqa: E402


def ce_case():
    X = np.load(os.path.join(ROOT, "tests", "golden", "reference_examples", "corr.npy"))
    y = np.load(os.path.join(ROOT, "tests", "golden", "reference_examples", "energy.npy"))
    n, p = X.shape
    rng = np.random.default_rng(7)
    rows = rng.choice(100, 100, replace=False)
    others = rng.integers(150, n, (100, 2))
    H = X[rows] - 0.5 * (X[others[:, 0]] + X[others[:, 1]])
    lb = np.full(p, -np.inf)
    lb[:5] = 0.0
    E = np.zeros((1, p))
    E[0, 6], E[0, 7] = 1.0, -1.0
    cons = [Bounds(lb, np.inf), LinearConstraint(H, -np.inf, -1e-3), LinearConstraint(E, 0.0, 0.0)]
    return X, y, cons, 1e-2 * np.max(np.abs(X.T @ y)) / n


def gauss_case(n=100, p=80):
    rng = np.random.default_rng(1)
    X = rng.standard_normal((n, p))
    y = X @ np.where(rng.random(p) < 0.3, rng.standard_normal(p), 0.0) + 0.1 * rng.standard_normal(n)
    lb = np.full(p, -np.inf)
    lb[:10] = 0.0
    A = rng.standard_normal((20, p))
    E = np.zeros((1, p))
    E[0, 12], E[0, 13] = 1.0, -1.0
    cons = [Bounds(lb, np.inf), LinearConstraint(A, -np.inf, 0.3), LinearConstraint(E, 0.0, 0.0)]
    return X, y, cons, 0.05 * np.max(np.abs(X.T @ y)) / n


def timed(make, X, y, repeats):
    make().fit(X, y)  # (first fit: build of the kernels' tables, dataset upload into the cache)
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        est = make().fit(X, y)
        ts.append(time.perf_counter() - t0)
    return est, 1e3 * float(np.median(ts))


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    warnings.simplefilter("ignore")
    for name, (X, y, cons, alpha) in (("ce_290x66", ce_case()), ("gauss_100x80", gauss_case())):
        for cls in (Lasso, AdaptiveLasso):
            chip, t_chip = timed(lambda: cls(alpha=alpha, constraints=cons), X, y, repeats)
            host, t_host = timed(lambda: cls(alpha=alpha, constraints=cons, solver_options={"on_chip": False}), X, y, repeats)
            diff = float(np.max(np.abs(chip.coef_ - host.coef_)) / max(np.max(np.abs(host.coef_)), 1e-300))
            print(json.dumps({
                "case": name, "estimator": cls.__name__, "m": stack_constraints(cons, X.shape[1]).m,
                "on_chip_ms": round(t_chip, 3), "host_ms": round(t_host, 3), "speedup": round(t_host / t_chip, 1),
                "route_chip": chip.solver_info_["route"], "route_host": host.solver_info_["route"],
                "sweeps_chip": chip.solver_info_["sweeps"], "sweeps_host": host.solver_info_["sweeps"],
                "rel_diff": diff, "max_violation": chip.solver_info_["max_violation"],
            }), flush=True)


if __name__ == "__main__":
    main()
