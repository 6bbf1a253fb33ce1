"""Exact l0 search: nodes visited, wall time and nodes per second at the reference's sizes (its tests run the mixed-integer
estimators on 25 x 20 and 25 x 30 ``make_regression`` draws with ``sparse_bound = p // 2``, ``alpha = 3``, ``eta = 1``;
``big_M = 1000`` here so that the box stays out of the way), for each of the four estimators.  Writes
``profiles/l0_search.txt``.  ``--max-nodes N`` sets the budget of every call (default 2^24, enough to see the rate).

The engine's default budget (``kL0DefaultNodes``, csrc/engine_l0.hip) is the largest power of two for which a call that
exhausts it at 25 x 30 stays under two seconds at the rate measured here; both numbers are in the file's last lines,
followed by one timed call under the default budget itself.

Then the l1 mode (``L1L0``, ``slm_solve_l0_l1``) at the same two sizes beside ``RegularizedL0`` on the same data and
``alpha``, for ``eta`` = 1e-3, 0.05 and 0.5 of ``||X^T y / n||_inf``: nodes, descents run (candidates that passed the
lower-bound filter), wall time.  No figure is promised for these: how many candidates pass the filter depends on ``eta``."""

import argparse
import math
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "sparse-lm_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-nodes", type=int, default=1 << 24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l0_search.txt"))
    args = ap.parse_args()
    from sklearn.datasets import make_regression

    from sparselm_amd import _engine
    from sparselm_amd.miqp import L1L0
    from sparselm_amd.model import L2L0, BestSubsetSelection, RegularizedL0, RidgedBestSubsetSelection

    dev = _engine.get_engine().device_info()
    name = dev["name"].strip() or "device"  # (some runtimes report the architecture only)
    lines = [f"exact l0 search on {name}, {dev['compute_units']} compute units: budget {args.max_nodes} nodes per call", ""]
    lines.append(f"{'estimator':28s} {'n x p':8s} {'nodes':>12s} {'wall s':>9s} {'nodes/s':>12s} {'proven':>7s} {'objective':>16s}")
    opts = {"max_nodes": args.max_nodes}
    slowest_rate = math.inf
    for p in (20, 30):
        X, y = make_regression(25, p, n_informative=10, noise=1.0, random_state=0)
        makers = [
            lambda: BestSubsetSelection(sparse_bound=p // 2, big_M=1000, solver_options=opts),
            lambda: RidgedBestSubsetSelection(sparse_bound=p // 2, eta=1.0, big_M=1000, solver_options=opts),
            lambda: RegularizedL0(alpha=3.0, big_M=1000, solver_options=opts),
            lambda: L2L0(alpha=3.0, eta=1.0, big_M=1000, solver_options=opts),
        ]
        for make in makers:
            make().fit(X, y)  # (warm: the first call of a process loads the code object)
            est = make()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                t0 = time.perf_counter()
                est.fit(X, y)
                wall = time.perf_counter() - t0
            info = est.solver_info_
            rate = info["nodes"] / wall
            if not info["proven_optimal"] and p == 30:
                slowest_rate = min(slowest_rate, rate)
            lines.append(f"{type(est).__name__:28s} {'25x%d' % p:8s} {info['nodes']:12d} {wall:9.4f} {rate:12.3e} "
                         f"{str(info['proven_optimal']):>7s} {info['objective']:16.8e}")
    lines.append("")
    if math.isfinite(slowest_rate):
        budget = 1 << int(math.floor(math.log2(2.0 * slowest_rate)))
        lines.append(f"slowest budget-exhausting call at 25x30: {slowest_rate:.3e} nodes/s (wall time of the whole fit)")
        lines.append(f"largest power of two that stays under 2 s at that rate: 2^{int(math.log2(budget))} = {budget} nodes")
    else:
        lines.append("no call at 25x30 exhausted the budget: raise --max-nodes to measure the rate of an exhausting call")
    # the engine's default budget itself, timed (not extrapolated): best subset at 25 x 30 with no max_nodes given
    X, y = make_regression(25, 30, n_informative=10, noise=1.0, random_state=0)
    est = BestSubsetSelection(sparse_bound=15, big_M=1000)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t0 = time.perf_counter()
        est.fit(X, y)
        wall = time.perf_counter() - t0
    info = est.solver_info_
    lines.append(f"BestSubsetSelection 25x30 under the default budget: {info['nodes']} nodes in {wall:.3f} s, "
                 f"proven optimal: {info['proven_optimal']}, objective {info['objective']:.8e}")
    # the l1 mode beside RegularizedL0: same data, same alpha
    lines += ["", f"l1 mode (L1L0) beside RegularizedL0, alpha = 3, big_M = 1000, budget {args.max_nodes} nodes per call; eta relative to ||X^T y / n||_inf", ""]
    lines.append(f"{'estimator':28s} {'n x p':8s} {'eta rel':>8s} {'nodes':>12s} {'descents':>10s} {'wall s':>9s} {'proven':>7s} {'bound used':>16s} "
                 f"{'objective':>16s}")
    for p in (20, 30):
        X, y = make_regression(25, p, n_informative=10, noise=1.0, random_state=0)
        cinf = float(np.max(np.abs(X.T @ y / X.shape[0])))
        makers = [(None, lambda: RegularizedL0(alpha=3.0, big_M=1000, solver_options=opts))]
        makers += [(rel, lambda rel=rel: L1L0(alpha=3.0, eta=rel * cinf, big_M=1000, solver_options=opts)) for rel in (1e-3, 0.05, 0.5)]
        for rel, make in makers:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                make().fit(X, y)
                est = make()
                t0 = time.perf_counter()
                est.fit(X, y)
                wall = time.perf_counter() - t0
            info = est.solver_info_
            lines.append(f"{type(est).__name__:28s} {'25x%d' % p:8s} {'-' if rel is None else '%g' % rel:>8s} {info['nodes']:12d} "
                         f"{info.get('descents', 0):10d} {wall:9.4f} {str(info['proven_optimal']):>7s} {info['q_all']:16.8e} {info['objective']:16.8e}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
