"""Exact l0 search: nodes visited, wall time and nodes per second at the reference's sizes (its tests run the mixed-integer
estimators on 25 x 20 and 25 x 30 ``make_regression`` draws with ``sparse_bound = p // 2``, ``alpha = 3``, ``eta = 1``;
``big_M = 1000`` here so that the box stays out of the way), for each of the four estimators.  Writes
``profiles/l0_search.txt``.  ``--max-nodes N`` sets the budget of every call (default 2^24, enough to see the rate).

The engine's default budget (``kL0DefaultNodes``, csrc/engine_l0.hip) is the largest power of two for which a call that
exhausts it at 25 x 30 stays under two seconds at the rate measured here; both numbers are in the file's last lines,
followed by one timed call under the default budget itself.

Then the l1 mode (``L1L0``, ``slm_solve_l0_l1``) at the same two sizes beside ``RegularizedL0`` on the same data and
``alpha``, for ``eta`` = 1e-3, 0.05 and 0.5 of ``||X^T y / n||_inf``: nodes, descents run (candidates that passed the
lower-bound filter), wall time.  No figure is promised for these: how many candidates pass the filter depends on ``eta``.

Then the profile (``sparselm_amd.miqp.l0_profile``, ``slm_solve_l0_profile``), written to ``profiles/l0_profile.txt``: nodes,
wall time and nodes/s of ONE profile call beside the summed wall time of the separate estimator fits it replaces, same
process, same device -- 25 x 20 and 25 x 30 with ``max_groups = 8`` against ``BestSubsetSelection(sparse_bound=1..8)``; the
45 x 30 training split of the reference's ``examples/plot_line_search.py`` with that example's ``eta`` (1.0, ``L2L0``'s default
while ``alpha`` is scanned) and ``alpha_min`` = the smallest of its five alphas, against ``L2L0`` at the five; one call at
``alpha_min = 0`` beside one at that ``alpha_min``; and the nodes of a single ``RegularizedL0(alpha_min)`` search beside the
profile's at the same ``alpha_min`` (the profile's bound uses only sizes <= the node's own, so it prunes less).  Nothing is
promised: the file states what was found.

Then the wide mode (``solver_options={"wide": True}``, ``slm_solve_l0_wide``), written to ``profiles/l0_wide.txt``: the wide
kernel forced (through the dataset call) on the 25 x 20 and 25 x 30 problems above beside the narrow kernel on the same
dataset in the same run -- the price of ``WIDE`` per node; ``BestSubsetSelection(sparse_bound=K)`` at 150 x 100 with K = 3
and at 200 x 128 with K = 4; and ``L2L0(fit_intercept=True, alpha=3.16e-7, eta=1.66e-6)`` on the reference's 290 x 66
cluster-expansion data under the default budget.

Then the constrained mode (``add_constraints``, ``slm_solve_l0_constrained``), written to ``profiles/l0_constrained.txt``: the four
estimators at the two sizes above under non-negativity and four random rows, beside the same estimator without constraints --
nodes, ``qp_solves`` (candidates valued on chip), ``unsettled`` and the wall time of the whole call -- and one problem of 64
columns under 64 rows.  An estimator without a ridge term at 25 x 30 is refused (its Gram is singular) and recorded so.  No
rate is promised: how many candidates pass the filter depends on the constraints.

Then the exclusion bound (``solver_options={"bound": "exclusion"}``, ``slm_solve_l0_xb`` / ``slm_solve_l0_xb_wide``), written to
``profiles/l0_bound.txt``: every row beside the plain search of the same build on the same device, the calls alternating --
the four estimators at the two sizes above under the default budget (nodes and the wall time of the whole call: the bounded
kernel costs more per node, so a problem the plain search finishes in milliseconds may get slower); best subset K = 15 at
25 x 30 with a ridge term; and ``L2L0`` on the reference's 290 x 66 data at alpha = 3.16e-7, 1e-6 and 1e-5.  No time is
promised.

Then the batched profile (``sparselm_amd.miqp.l0_profile_cv``, ``slm_solve_l0_profile_batch``), written to
``profiles/l0_cv.txt`` by ``--only cv`` (it is not part of a run without ``--only``): the profiles of five folds and of all rows
from one launch beside the six ``l0_profile`` calls they replace and beside ``GridSearchCV`` going fit by fit, on the 25 x 20
data with ``max_groups = 8`` (launch-bound); and batched against the sum of the singles on the line-search example's 45 x 30
split with ``eta = 1`` and ``alpha_min = 1e-3 var y`` (node-bound), with every problem's node count; and that split's all-rows
problem through the single entry beside one, two and six copies of it through the batched entry (copies finish together: what
they lose is not lost to idle workgroups of finished problems).  Whole calls, each ending
in a synchronise, after a warm-up of every shape; ``--repeats`` (default 5) repeats with the variants alternating; median and
spread.  Nothing is promised but what the file states.

Then the l1 profile (``sparselm_amd.miqp.l1l0_profile``, ``slm_solve_l0_l1_profile`` / ``_wide``), written to
``profiles/l1l0_profile.txt`` by ``--only l1profile`` (it is not part of a run without ``--only``): at 25 x 20 and 25 x 30 one profile
call at one ``eta`` with ``alpha_min`` the smallest of ten alphas beside the ten ``L1L0`` fits it replaces, in the same run --
nodes, descents and ms per call, warm, the median of ``--repeats`` (default 5) with the variants alternating; and one call on
the reference's 290 x 66 data (status, nodes, descents, time).  Every call runs under ``--max-nodes`` (a descent costs far more
than a node, so the default budget of 2^30 nodes would take minutes per call at 25 x 30).  Nothing is promised but what the file states.

Then the profile grid (``sparselm_amd.miqp.l1l0_profile_cv`` / ``l2l0_profile_cv``, ``slm_solve_l0_profile_grid``), written to
``profiles/l0_grid_cv.txt`` by ``--only gridcv`` (it is not part of a run without ``--only``): at 25 x 20 with five folds and eight
``eta`` values one ``l1l0_profile_cv`` call (48 problems, one launch) beside the 48 ``l1l0_profile`` calls it replaces, and one
``l2l0_profile_cv`` call beside the 8 ``l0_profile_cv`` calls it replaces; and the node-bound 45 x 30 split of ``--only cv`` for
the ridge kind, every problem under ``--max-nodes``.  Whole calls, warm, the variants alternating, medians of ``--repeats``
(default 5).  Nothing is promised but what the file states; a row where the one launch is slower is written down like any other.

Then the local search (``sparselm_amd.miqp.l0_local_search``, ``slm_solve_l0_local``), written to ``profiles/l0_local.txt`` by
``--only local`` (it is not part of a run without ``--only``): beside ``RegularizedL0`` on the reference's 290 x 66 data and at 25 x 30
(time, and the objective's gap to the proven or incumbent value); at 200 x 512 and 400 x 1024 one launch of 1, 16, 64 and 256 cells
against the host twin ``l0_local_solve<false>`` on one core (``tools/l0_local_host_bench.cpp``, compiled here with g++); the time per applied
coordinate change at 1024 columns.  No ratio is promised: the file names the number of cells from which the launch wins, or says that it
did not, and what was not measured.

``--only search`` / ``--only profile`` / ``--only wide`` / ``--only constrained`` / ``--only bound`` / ``--only cv`` / ``--only l1profile`` /
``--only gridcv`` / ``--only local`` runs one part."""

import argparse
import math
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "sparse-lm_amd"))


def timed(fn):
    """(result, wall seconds) of the second of two calls: the first loads code objects and builds nothing that is kept."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        fn()
        t0 = time.perf_counter()
        out = fn()
        return out, time.perf_counter() - t0


def profile_section(out_path):
    from sklearn.datasets import make_regression
    from sklearn.model_selection import train_test_split

    from sparselm_amd import _engine
    from sparselm_amd.miqp import l0_profile
    from sparselm_amd.model import L2L0, BestSubsetSelection, RegularizedL0

    dev = _engine.get_engine().device_info()
    name = dev["name"].strip() or "device"
    lines = [f"exact l0 profile on {name}, {dev['compute_units']} compute units: one profile call beside the separate fits it replaces",
             "(wall time of the whole Python call, second of two calls each; default node budget; big_M = 1000)", ""]
    head = f"{'what':58s} {'n x p':8s} {'nodes':>12s} {'wall s':>9s} {'nodes/s':>12s} {'proven':>7s}"

    def row(what, shape, nodes, wall, proven):
        lines.append(f"{what:58s} {shape:8s} {nodes:12d} {wall:9.4f} {nodes / wall:12.3e} {str(proven):>7s}")
        print(lines[-1], flush=True)

    # ---- best subset at the bounds 1 .. 8 -----------------------------------------------------------------------------------
    lines += ["best subset, max_groups = 8, against BestSubsetSelection(sparse_bound=1..8)", head]
    for p in (20, 30):
        X, y = make_regression(25, p, n_informative=10, noise=1.0, random_state=0)
        prof, wall = timed(lambda: l0_profile(X, y, max_groups=8, big_M=1000))
        row("l0_profile(max_groups=8)", "25x%d" % p, prof.solver_info_["nodes"], wall, prof.proven_optimal_)
        total_wall, total_nodes, same = 0.0, 0, True
        for K in range(1, 9):
            est, w = timed(lambda: BestSubsetSelection(sparse_bound=K, big_M=1000).fit(X, y))
            total_wall += w
            total_nodes += est.solver_info_["nodes"]
            same = same and np.array_equal(est.coef_, prof.best_subset(K)[0]) and est.solver_info_["proven_optimal"]
        row("sum of 8 BestSubsetSelection fits", "25x%d" % p, total_nodes, total_wall, same)
        lines.append(f"    one profile call / eight fits: {wall / total_wall:.3f} of the wall time; coefficients identical at every bound: {same}")
    # ---- the line-search example's alpha scan ---------------------------------------------------------------------------------
    X, y = make_regression(n_samples=60, n_features=30, n_informative=8, noise=40.0, bias=-15.0, random_state=0)
    X, _, y, _ = train_test_split(X, y, test_size=0.25, random_state=0)
    var = float(np.var(y))
    alphas = np.logspace(-6, 1, 5) * var
    eta = 1.0
    lines += ["", f"L2L0 alpha scan of the line-search example (45 x 30, fit_intercept, eta = {eta:g}): alphas = logspace(-6, 1, 5) * var(y), "
              f"var(y) = {var:.4e}; alpha_min = the smallest", head]
    prof, wall = timed(lambda: l0_profile(X, y, alpha_min=alphas[0], eta=eta, big_M=1000, fit_intercept=True))
    row("l0_profile(alpha_min=1e-6 var y)", "45x30", prof.solver_info_["nodes"], wall, prof.proven_optimal_)
    total_wall, total_nodes, same = 0.0, 0, True
    for alpha in alphas:
        est, w = timed(lambda: L2L0(alpha=alpha, eta=eta, big_M=1000, fit_intercept=True).fit(X, y))
        total_wall += w
        total_nodes += est.solver_info_["nodes"]
        agree = np.array_equal(est.coef_, prof.regularized(alpha)[0])
        same = same and agree
        row(f"  L2L0(alpha={alpha:.3e}): size {int(est.active_groups_.sum())}, same coefficients {agree}", "45x30", est.solver_info_["nodes"], w,
            est.solver_info_["proven_optimal"])
    row("sum of 5 L2L0 fits", "45x30", total_nodes, total_wall, same)
    lines.append(f"    one profile call / five fits: {wall / total_wall:.3f} of the wall time; coefficients identical at every alpha: {same}")
    # ---- alpha_min = 0 beside that alpha_min, and a single RegularizedL0 search at alpha_min -------------------------------------
    lines += ["", "the same problem: the full table (alpha_min = 0) beside the pruned one, and single searches at alpha_min", head]
    full, wall0 = timed(lambda: l0_profile(X, y, alpha_min=0.0, eta=eta, big_M=1000, fit_intercept=True))
    row("l0_profile(alpha_min=0)", "45x30", full.solver_info_["nodes"], wall0, full.proven_optimal_)
    row("l0_profile(alpha_min=1e-6 var y)", "45x30", prof.solver_info_["nodes"], wall, prof.proven_optimal_)
    for rel in (1e-6, 1e-3, 1e-2):
        a = rel * var
        pr, wp = timed(lambda: l0_profile(X, y, alpha_min=a, big_M=1000, fit_intercept=True))
        est, we = timed(lambda: RegularizedL0(alpha=a, big_M=1000, fit_intercept=True).fit(X, y))
        row(f"l0_profile(alpha_min={rel:g} var y), eta = 0", "45x30", pr.solver_info_["nodes"], wp, pr.proven_optimal_)
        row(f"RegularizedL0(alpha={rel:g} var y)", "45x30", est.solver_info_["nodes"], we, est.solver_info_["proven_optimal"])
        if est.solver_info_["nodes"]:
            lines.append(f"    the profile visits {pr.solver_info_['nodes'] / est.solver_info_['nodes']:.2f} x the nodes of the single search at its alpha_min")
    lines += ["", "proven False: the call ran out of the default budget of 2^30 nodes -- the estimator then holds its incumbent and the profile",
              "its table of incumbents, so 'same coefficients' on such a row compares two incumbents, not two optima."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)
    print(text)


def wide_section(out_path, max_nodes):
    from sklearn.datasets import make_regression

    from sparselm_amd import _engine
    from sparselm_amd.model import L2L0, BestSubsetSelection

    dev = _engine.get_engine().device_info()
    name = dev["name"].strip() or "device"
    lines = [f"wide exact l0 search on {name}, {dev['compute_units']} compute units", "(wall time of the whole call, second of two calls each)", ""]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    # ---- the price of WIDE per node: both kernels on the same dataset ------------------------------------------------------------
    say(f"the wide kernel forced on narrow problems beside the narrow kernel (dataset calls, big_M = 1000, budget {max_nodes} nodes per call)")
    say(f"{'problem':34s} {'n x p':8s} {'kernel':7s} {'nodes':>12s} {'wall s':>9s} {'nodes/s':>12s} {'proven':>7s} {'objective':>16s}")
    for p in (20, 30):
        X, y = make_regression(25, p, n_informative=10, noise=1.0, random_state=0)
        with _engine.get_engine().dataset(X, y) as ds:
            for what, kw in (("best subset, K = p / 2", dict(max_groups=p // 2)), ("ridged best subset, eta = 1", dict(max_groups=p // 2, eta=1.0)),
                             ("RegularizedL0, alpha = 3", dict(alpha=3.0)), ("L2L0, alpha = 3, eta = 1", dict(alpha=3.0, eta=1.0))):
                rates = {}
                for kernel, call in (("narrow", ds.solve_l0), ("wide", ds.solve_l0_wide)):
                    (_, _, info), wall = timed(lambda: call(big_M=1000.0, max_nodes=max_nodes, **kw))
                    rates[kernel] = info["nodes"] / wall
                    say(f"{what:34s} {'25x%d' % p:8s} {kernel:7s} {info['nodes']:12d} {wall:9.4f} {rates[kernel]:12.3e} "
                        f"{str(info['proven_optimal']):>7s} {info['objective']:16.8e}")
                say(f"    wide / narrow nodes per second: {rates['wide'] / rates['narrow']:.3f}")
    # ---- a small bound over a wide dictionary ------------------------------------------------------------------------------------
    say("")
    say("BestSubsetSelection(sparse_bound=K, big_M=1000, solver_options={'wide': True}), default budget")
    say(f"{'n x p':10s} {'K':>3s} {'nodes':>12s} {'wall s':>9s} {'nodes/s':>12s} {'proven':>7s} {'capacity_cut':>13s} {'objective':>16s}")
    for n, p, K in ((150, 100, 3), (200, 128, 4)):
        X, y = make_regression(n, p, n_informative=10, noise=1.0, random_state=0)
        est, wall = timed(lambda: BestSubsetSelection(sparse_bound=K, big_M=1000, solver_options={"wide": True}).fit(X, y))
        info = est.solver_info_
        say(f"{'%dx%d' % (n, p):10s} {K:3d} {info['nodes']:12d} {wall:9.4f} {info['nodes'] / wall:12.3e} {str(info['proven_optimal']):>7s} "
            f"{str(info['capacity_cut']):>13s} {info['objective']:16.8e}")
    # ---- the reference's cluster-expansion data ----------------------------------------------------------------------------------
    d = os.path.join(ROOT, "tests", "golden", "reference_examples")
    X, y = np.load(os.path.join(d, "corr.npy")), np.load(os.path.join(d, "energy.npy"))
    say("")
    say(f"L2L0(fit_intercept=True, alpha=3.16e-7, eta=1.66e-6, solver_options={{'wide': True}}) on the reference's {X.shape[0]} x {X.shape[1]} data, "
        "default budget")
    est, wall = timed(lambda: L2L0(fit_intercept=True, alpha=3.16e-7, eta=1.66e-6, solver_options={"wide": True}).fit(X, y))
    info = est.solver_info_
    say(f"    finished: {info['proven_optimal']} (status {info['status']}), {info['nodes']} nodes in {wall:.3f} s ({info['nodes'] / wall:.3e} nodes/s)")
    say(f"    objective {info['objective']:.10e}, lower bound {info['lower_bound']:.10e}, seed {info['seed_objective']:.10e}, q_all {info['q_all']:.10e}")
    say(f"    active columns {int(est.active_groups_.sum())} of {X.shape[1]}, capacity_cut {info['capacity_cut']}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


def bound_section(out_path):
    from sklearn.datasets import make_regression

    from sparselm_amd import _engine
    from sparselm_amd.model import L2L0, BestSubsetSelection, RegularizedL0, RidgedBestSubsetSelection

    dev = _engine.get_engine().device_info()
    name = dev["name"].strip() or "device"
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "l0_host.hpp")) as fh:
        xcap = next(line.split("=")[1].split(";")[0].strip() for line in fh if line.startswith("constexpr int L0_XCAP"))
    lines = [f"exact l0 search with the exclusion bound on {name}, {dev['compute_units']} compute units; L0_XCAP = {xcap}",
             "(wall time of the whole Python call; plain and bounded calls alternate, the second of two calls each is reported; default node",
             " budget; big_M = 1000)", ""]
    head = (f"{'estimator':46s} {'n x p':8s} {'bound':>9s} {'nodes':>12s} {'wall s':>9s} {'proven':>7s} {'objective':>18s} {'margin':>10s}")

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def pair(what, shape, make, X, y):
        """``make(options)`` -> estimator; plain, bounded, plain, bounded"""
        res = {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(2):
                for kind, extra in (("q_all", {}), ("exclusion", {"bound": "exclusion"})):
                    est = make(extra)
                    t0 = time.perf_counter()
                    est.fit(X, y)
                    res[kind] = (est, time.perf_counter() - t0)
        for kind in ("q_all", "exclusion"):
            est, wall = res[kind]
            info = est.solver_info_
            ran = info.get("bound", "q_all")
            say(f"{what:46s} {shape:8s} {ran if kind == 'exclusion' else 'q_all':>9s} {info['nodes']:12d} {wall:9.4f} {str(info['proven_optimal']):>7s} "
                f"{info['objective']:18.10e} {info.get('bound_margin', float('nan')):10.2e}")
        a, b = res["q_all"], res["exclusion"]
        same = np.array_equal(a[0].coef_, b[0].coef_)
        say(f"    exclusion / q_all: {b[0].solver_info_['nodes'] / max(a[0].solver_info_['nodes'], 1):.3g} of the nodes, {b[1] / a[1]:.3g} of the wall "
            f"time; same coefficients: {same}" + ("" if "bound_reason" not in b[0].solver_info_ else f"; fell back: {b[0].solver_info_['bound_reason']}"))

    say(head)
    for p in (20, 30):
        X, y = make_regression(25, p, n_informative=10, noise=1.0, random_state=0)
        shape = "25x%d" % p
        pair("BestSubsetSelection(K = p / 2)", shape, lambda o: BestSubsetSelection(sparse_bound=p // 2, big_M=1000, solver_options=o), X, y)
        pair("RidgedBestSubsetSelection(K = p / 2, eta = 1)", shape,
             lambda o: RidgedBestSubsetSelection(sparse_bound=p // 2, eta=1.0, big_M=1000, solver_options=o), X, y)
        pair("RegularizedL0(alpha = 3)", shape, lambda o: RegularizedL0(alpha=3.0, big_M=1000, solver_options=o), X, y)
        pair("L2L0(alpha = 3, eta = 1)", shape, lambda o: L2L0(alpha=3.0, eta=1.0, big_M=1000, solver_options=o), X, y)
    say("")
    say("best subset K = 15 at 25 x 30 with a ridge term (without one n < p: the Gram is singular and the call falls back)")
    say(head)
    X, y = make_regression(25, 30, n_informative=10, noise=1.0, random_state=0)
    for eta in (1.0, 1e-3):
        pair(f"RidgedBestSubsetSelection(K = 15, eta = {eta:g})", "25x30",
             lambda o: RidgedBestSubsetSelection(sparse_bound=15, eta=eta, big_M=1000, solver_options=o), X, y)
    d = os.path.join(ROOT, "tests", "golden", "reference_examples")
    X, y = np.load(os.path.join(d, "corr.npy")), np.load(os.path.join(d, "energy.npy"))
    say("")
    say(f"L2L0(fit_intercept=True, eta=1.66e-6, solver_options={{'wide': True}}) on the reference's {X.shape[0]} x {X.shape[1]} data")
    say(head)
    for alpha in (1e-5, 1e-6, 3.16e-7):
        pair(f"L2L0(alpha = {alpha:g})", "%dx%d" % X.shape,
             lambda o: L2L0(fit_intercept=True, alpha=alpha, eta=1.66e-6, solver_options=dict(o, wide=True)), X, y)
    say("")
    say("not measured: the share of the wall time in which one wavefront walked the last ticket alone (the engine keeps no such count).")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


def constrained_section(out_path, max_nodes):
    from scipy.optimize import Bounds, LinearConstraint
    from sklearn.datasets import make_regression

    from sparselm_amd import _engine
    from sparselm_amd.model import L2L0, BestSubsetSelection, RegularizedL0, RidgedBestSubsetSelection

    dev = _engine.get_engine().device_info()
    name = dev["name"].strip() or "device"
    lines = [f"constrained exact l0 search on {name}, {dev['compute_units']} compute units: budget {max_nodes} nodes per call",
             "(wall time of the whole Python call, second of two calls each; big_M = 1000; constraints: coefficients >= 0 and four random",
             " rows r^T b <= 0.5 |r^T b_ols| + 1, beside the same estimator without constraints)", ""]
    head = (f"{'estimator':28s} {'n x p':8s} {'constraints':>11s} {'nodes':>12s} {'qp_solves':>10s} {'unsettled':>9s} {'wall s':>9s} {'status':>11s} "
            f"{'objective':>16s}")

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def run(make, X, y, shape, what):
        try:
            est, wall = timed(lambda: make().fit(X, y))
        except NotImplementedError as exc:
            say(f"{type(make()).__name__:28s} {shape:8s} {what:>11s} refused: {str(exc)[:110]}")
            return
        info = est.solver_info_
        say(f"{type(est).__name__:28s} {shape:8s} {what:>11s} {info['nodes']:12d} {info.get('qp_solves', 0):10d} {info.get('unsettled', 0):9d} "
            f"{wall:9.4f} {info['status']:>11s} {info['objective']:16.8e}")

    say(head)
    for p in (20, 30):
        X, y = make_regression(25, p, n_informative=10, noise=1.0, random_state=0)
        R = np.random.default_rng(p).standard_normal((4, p))
        b_ols = np.linalg.lstsq(X, y, rcond=None)[0]
        cons = [Bounds(0.0, np.inf), LinearConstraint(R, -np.inf, 0.5 * np.abs(R @ b_ols) + 1.0)]
        for c, what in ((None, "none"), (cons, "nonneg + 4")):
            opts = {"max_nodes": max_nodes}
            for make in (lambda: BestSubsetSelection(sparse_bound=p // 2, big_M=1000, solver_options=opts).add_constraints(c),
                         lambda: RidgedBestSubsetSelection(sparse_bound=p // 2, eta=1.0, big_M=1000, solver_options=opts).add_constraints(c),
                         lambda: RegularizedL0(alpha=3.0, big_M=1000, solver_options=opts).add_constraints(c),
                         lambda: L2L0(alpha=3.0, eta=1.0, big_M=1000, solver_options=opts).add_constraints(c)):
                run(make, X, y, "25x%d" % p, what)
    say("")
    say("64 columns under 64 rows: L2L0(alpha = 3, eta = 1), rows r^T b <= 0.5 |r^T b_ols| + 1")
    say(head)
    X, y = make_regression(100, 64, n_informative=10, noise=1.0, random_state=0)
    R = np.random.default_rng(64).standard_normal((64, 64))
    b_ols = np.linalg.lstsq(X, y, rcond=None)[0]
    cons = LinearConstraint(R, -np.inf, 0.5 * np.abs(R @ b_ols) + 1.0)
    for c, what in ((None, "none"), (cons, "64 rows")):
        run(lambda: L2L0(alpha=3.0, eta=1.0, big_M=1000, solver_options={"max_nodes": max_nodes}).add_constraints(c), X, y, "100x64", what)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


def cv_section(out_path, repeats):
    from sklearn.datasets import make_regression
    from sklearn.model_selection import KFold, train_test_split

    from sparselm_amd import _engine
    from sparselm_amd.miqp import l0_profile, l0_profile_cv
    from sparselm_amd.model import BestSubsetSelection
    from sparselm_amd.model_selection import GridSearchCV

    dev = _engine.get_engine().device_info()
    name = dev["name"].strip() or "device"
    lines = [f"batched exact l0 profile on {name}, {dev['compute_units']} compute units: five folds and all rows in one launch",
             f"(wall time of the whole Python call, which ends in a synchronise; every variant warmed up once, then {repeats} repeats with the",
             " variants alternating; median [min .. max]; default node budget; big_M = 1000; KFold(5, shuffle=True, random_state=0))", ""]

    def say(line):
        lines.append(line)
        print(line, flush=True)

    def measure(variants):
        """{name: sorted wall times} of ``repeats`` rounds over the variants in turn, after one warm-up round; and the last results"""
        walls, last = {k: [] for k in variants}, {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for rnd in range(repeats + 1):
                for k, fn in variants.items():
                    t0 = time.perf_counter()
                    last[k] = fn()
                    if rnd:
                        walls[k].append(time.perf_counter() - t0)
        return {k: sorted(v) for k, v in walls.items()}, last

    def fmt(v):
        return f"{float(np.median(v)):9.4f} [{v[0]:.4f} .. {v[-1]:.4f}]"

    cv = KFold(5, shuffle=True, random_state=0)

    def singles(X, y, **kw):
        return [l0_profile(X[tr], y[tr], **kw) for tr, _ in cv.split(X)] + [l0_profile(X, y, **kw)]

    # ---- (a) launch-bound ---------------------------------------------------------------------------------------------------------
    X, y = make_regression(25, 20, n_informative=10, noise=1.0, random_state=0)
    kw = dict(max_groups=8, big_M=1000)
    walls, last = measure({
        "batched": lambda: l0_profile_cv(X, y, cv=cv, **kw),
        "singles": lambda: singles(X, y, **kw),
        "grid": lambda: GridSearchCV(BestSubsetSelection(big_M=1000), {"sparse_bound": list(range(1, 9))}, cv=cv).fit(X, y),
    })
    cvp, six = last["batched"], last["singles"]
    same = all(np.array_equal(a.supports_, b.supports_) and np.allclose(a.values_, b.values_, rtol=1e-9, atol=0)
               for a, b in zip(cvp.profiles_ + [cvp.full_], six))
    picked = cvp.best_subset_search(list(range(1, 9)))
    say("(a) launch-bound: 25 x 20, max_groups = 8, no intercept")
    say(f"    one l0_profile_cv call (1 launch, 6 problems)          {fmt(walls['batched'])} s")
    say(f"    sum of the six l0_profile calls it replaces            {fmt(walls['singles'])} s")
    say(f"    GridSearchCV(BestSubsetSelection, sparse_bound=1..8)   {fmt(walls['grid'])} s   (40 fits and a refit)")
    say(f"    batched / six singles: {np.median(walls['batched']) / np.median(walls['singles']):.3f} of the median wall time; same supports and values "
        f"(1e-9) in all six tables: {same}")
    say(f"    nodes per problem: batched {[p['nodes'] for p in cvp.solver_info_['problems']]}, singles {[p.solver_info_['nodes'] for p in six]}")
    say(f"    selection: l0_profile_cv {picked.best_params_}, GridSearchCV {last['grid'].best_params_}")
    # ---- (b) node-bound -----------------------------------------------------------------------------------------------------------
    X, y = make_regression(n_samples=60, n_features=30, n_informative=8, noise=40.0, bias=-15.0, random_state=0)
    X, _, y, _ = train_test_split(X, y, test_size=0.25, random_state=0)
    kw = dict(alpha_min=1e-3 * float(np.var(y)), eta=1.0, big_M=1000, fit_intercept=True)
    walls, last = measure({"batched": lambda: l0_profile_cv(X, y, cv=cv, **kw), "singles": lambda: singles(X, y, **kw)})
    cvp, six = last["batched"], last["singles"]
    ratio = float(np.median(walls["batched"]) / np.median(walls["singles"]))
    spread = max((w[-1] - w[0]) / float(np.median(w)) for w in walls.values())
    say("")
    say("(b) node-bound: the line-search example's 45 x 30 split, fit_intercept, eta = 1, alpha_min = 1e-3 var y")
    say(f"    one l0_profile_cv call (1 launch, 6 problems)          {fmt(walls['batched'])} s")
    say(f"    sum of the six l0_profile calls it replaces            {fmt(walls['singles'])} s")
    say(f"    batched / six singles: {ratio:.3f} of the median wall time; the run's spread (max - min over the median): {spread:.3f}")
    say(f"    nodes per problem, batched: {[p['nodes'] for p in cvp.solver_info_['problems']]}")
    say(f"    nodes per problem, singles: {[p.solver_info_['nodes'] for p in six]}")
    say(f"    finished, batched: {[p['proven_optimal'] for p in cvp.solver_info_['problems']]}; singles: {[p.proven_optimal_ for p in six]}")
    nb, ns = sum(p["nodes"] for p in cvp.solver_info_["problems"]), sum(p.solver_info_["nodes"] for p in six)
    say(f"    nodes/s: batched {nb / float(np.median(walls['batched'])):.3e}, singles {ns / float(np.median(walls['singles'])):.3e}")
    if ratio > 1.0 + spread:
        say(f"    the batched call is slower by {100.0 * (ratio - 1.0):.1f} % of the singles' median, more than the run's spread")
    # ---- (c) where a difference arises: the same problem through the single entry, the batched entry alone, and in copies ---------
    Xc, yc = X - X.mean(axis=0), y - y.mean()
    kw = dict(alpha_min=kw["alpha_min"], eta=1.0, big_M=1000.0)
    with _engine.get_engine().dataset(Xc, yc) as ds:
        variants = {"the single entry": lambda: [ds.solve_l0_profile(**kw)[3]["nodes"]]}
        for copies in (1, 2, 6):
            variants[f"the batched entry, {copies} cop{'y' if copies == 1 else 'ies'} of it"] = (
                lambda copies=copies: [i["nodes"] for i in ds.solve_l0_profile_batch([None] * copies, [0] * copies, **kw)[4]])
        walls, last = measure(variants)
    say("")
    say("(c) the all-rows problem of (b), centred by hand, on one dataset: copies of one problem finish together, so no workgroup idles")
    say("    behind a finished problem; one copy has the single entry's grid")
    base = float(np.median(walls["the single entry"]))
    for k, v in walls.items():
        say(f"    {k:38s} {fmt(v)} s   {len(last[k])} x {last[k][0]} nodes   {float(np.median(v)) / (len(last[k]) * base):.3f} of as many single calls")
    say("    read with (b): the instantiation costs what one copy costs over the single entry; what copies lose they lose without any")
    say("    problem finishing early, so idle workgroups of finished problems are not what (b) shows.  The cause of the loss that comes")
    say("    with a split grid was not found: each problem keeps its share of the waves for the whole run, the node counts are equal.")
    say("not measured: the time workgroups of finished problems idle while other problems run (the engine keeps no such count).")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        fh.write(text)


def l1_profile_section(out_path, repeats, max_nodes):
    from sklearn.datasets import make_regression

    from sparselm_amd import _engine
    from sparselm_amd.miqp import L1L0, l1l0_profile

    dev = _engine.get_engine().device_info()
    name = dev["name"].strip() or "device"
    lines = [f"l1 profile (l1l0_profile) on {name}, {dev['compute_units']} compute units: one profile call beside the L1L0 fits it replaces",
             f"(wall time of whole Python calls, each ending in a synchronise; every shape warmed first; {repeats} repeats with the variants "
             f"alternating, medians with the spread min .. max; budget {max_nodes} nodes per call; big_M = 1000)", ""]
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    opts = {"max_nodes": max_nodes}

    def say(line):  # (the file grows line by line: a run that is cut short leaves what it measured)
        lines.append(line)
        print(line, flush=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def clock(fn):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            out = fn()
            return out, (time.perf_counter() - t0) * 1e3

    def fmt(ms):
        return f"{np.median(ms):9.3f} ({min(ms):.3f} .. {max(ms):.3f})"

    for p in (20, 30):
        X, y = make_regression(25, p, n_informative=10, noise=1.0, random_state=0)
        var, cinf = float(np.var(y)), float(np.max(np.abs(X.T @ y / X.shape[0])))
        eta = 0.05 * cinf
        alphas = np.logspace(-4, 0, 10) * var
        profile = lambda: l1l0_profile(X, y, eta=eta, alpha_min=alphas[0], big_M=1000, solver_options=opts)  # noqa: E731
        fits = lambda: [L1L0(alpha=a, eta=eta, big_M=1000, solver_options=opts).fit(X, y) for a in alphas]  # noqa: E731
        clock(profile), clock(fits)  # (warm: the first call of a shape loads the code objects)
        t_prof, t_fits, prof, ests = [], [], None, None
        for _ in range(repeats):
            (prof, ms) = clock(profile)
            t_prof.append(ms)
            (ests, ms) = clock(fits)
            t_fits.append(ms)
        same = all(np.array_equal(e.coef_, prof.regularized(a)[0]) for e, a in zip(ests, alphas))
        proven = prof.proven_optimal_ and all(e.solver_info_["proven_optimal"] for e in ests)
        unproven = [f"{a / var:.1e}" for e, a in zip(ests, alphas) if not e.solver_info_["proven_optimal"]]
        say(f"25 x {p}, eta = 0.05 ||X^T y / n||_inf, alphas = logspace(-4, 0, 10) var y, alpha_min = the smallest")
        say(f"{'what':42s} {'nodes':>12s} {'descents':>10s} {'ms per call: median (min .. max)':>36s}")
        say(f"{'l1l0_profile(alpha_min=1e-4 var y)':42s} {prof.solver_info_['nodes']:12d} {prof.solver_info_['descents']:10d} {fmt(t_prof):>36s}")
        say(f"{'the ten L1L0 fits together':42s} {sum(e.solver_info_['nodes'] for e in ests):12d} "
            f"{sum(e.solver_info_['descents'] for e in ests):10d} {fmt(t_fits):>36s}")
        say(f"    sizes along the alphas {[int(e.active_groups_.sum()) for e in ests]}; every call proven: {proven}; coefficients identical at "
            f"every alpha: {same}")
        if not proven:
            say(f"    the budget ran out in: the profile {not prof.proven_optimal_}; the fits at alpha / var y = {unproven} -- such rows compare "
                "incumbents, not optima")
        say(f"    one profile call / ten fits: {np.median(t_prof) / np.median(t_fits):.3f} of the wall time")
        say("")
    d = os.path.join(ROOT, "tests", "golden", "reference_examples")
    X, y = np.load(os.path.join(d, "corr.npy")), np.load(os.path.join(d, "energy.npy"))
    alpha_min, eta = 3.16e-7, 1.66e-6
    call = lambda: l1l0_profile(X, y, eta=eta, alpha_min=alpha_min, max_groups=64, fit_intercept=True,  # noqa: E731
                                solver_options={"wide": True, "max_nodes": max_nodes})
    clock(call)
    prof, ms = clock(call)
    info = prof.solver_info_
    say(f"the reference's {X.shape[0]} x {X.shape[1]} data: l1l0_profile(eta=1.66e-6, alpha_min=3.16e-7, max_groups=64, fit_intercept=True, "
        f"solver_options={{'wide': True}}), budget {max_nodes} nodes, the second of two calls")
    say(f"    status {info['status']} (proven: {info['proven_optimal']}), {info['nodes']} nodes, {info['descents']} descents, {ms / 1e3:.3f} s "
        f"({info['nodes'] / (ms / 1e3):.3e} nodes/s)")
    k = prof.regularized_size(alpha_min)
    say(f"    bound on all columns {info['q_all']:.10e}; filled rows {int(np.isfinite(prof.values_).sum())} of {len(prof.values_)}; at alpha_min the "
        f"table reads size {k}, objective {prof.values_[k] + alpha_min * k:.10e}")
    say("    (nothing replaces this row: L1L0 itself stops at 64 columns)")


def grid_cv_section(out_path, repeats, max_nodes):
    from sklearn.datasets import make_regression
    from sklearn.model_selection import KFold, train_test_split

    from sparselm_amd import _engine
    from sparselm_amd.miqp import l0_profile_cv, l1l0_profile, l1l0_profile_cv, l2l0_profile_cv

    dev = _engine.get_engine().device_info()
    name = dev["name"].strip() or "device"
    lines = [f"exact l0 profile grid on {name}, {dev['compute_units']} compute units: (five folds + all rows) x eight eta in one launch",
             f"(wall time of whole Python calls, each ending in a synchronise; every variant warmed up once, then {repeats} repeats with the",
             f" variants alternating; median [min .. max]; budget {max_nodes} nodes per problem; big_M = 1000; KFold(5, shuffle=True, random_state=0))", ""]
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    opts = {"max_nodes": max_nodes}
    cv = KFold(5, shuffle=True, random_state=0)

    def say(line):  # (the file grows line by line: a run that is cut short leaves what it measured)
        lines.append(line)
        print(line, flush=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def measure(variants):
        walls, last = {k: [] for k in variants}, {}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for rnd in range(repeats + 1):
                for k, fn in variants.items():
                    t0 = time.perf_counter()
                    last[k] = fn()
                    if rnd:
                        walls[k].append(time.perf_counter() - t0)
        return {k: sorted(v) for k, v in walls.items()}, last

    def fmt(v):
        return f"{float(np.median(v)):9.4f} [{v[0]:.4f} .. {v[-1]:.4f}]"

    def tables(grid):  # row sets outermost, etas innermost: the engine's order
        return [(c.profiles_ + [c.full_]) for c in grid.cvs_]

    def report(what_one, what_many, count, walls, same, grid, many_infos):
        ratio = float(np.median(walls["one"]) / np.median(walls["many"]))
        spread = max((w[-1] - w[0]) / float(np.median(w)) for w in walls.values())
        probs = grid.solver_info_["problems"]
        say(f"    one {what_one} call (1 launch, {len(probs)} problems){'':8s} {fmt(walls['one'])} s")
        say(f"    the {count} {what_many} calls it replaces{'':18s} {fmt(walls['many'])} s")
        say(f"    one call / {count} calls: {ratio:.3f} of the median wall time; the run's spread (max - min over the median): {spread:.3f}; same supports "
            f"and values (1e-9) in all {len(probs)} tables: {same}")
        say(f"    nodes: one call {sum(p['nodes'] for p in probs)}, the {count} calls {sum(i['nodes'] for i in many_infos)}; finished: one call "
            f"{sum(p['proven_optimal'] for p in probs)} of {len(probs)}, the {count} calls {sum(i['proven_optimal'] for i in many_infos)} of {len(many_infos)}")
        if "descents" in probs[0]:
            say(f"    descents: one call {sum(p['descents'] for p in probs)}, the {count} calls {sum(i['descents'] for i in many_infos)}")
        if ratio > 1.0 + spread:
            say(f"    the one call is SLOWER by {100.0 * (ratio - 1.0):.1f} % of the {count} calls' median, more than the run's spread")

    def agree(a, b, alphas=None):
        """The same table; with ``alphas`` (a table pruned by alpha_min > 0, whose rows need not be the best of their size, or one that
        saturates under an l1 term): the same answer at each of them, which is what such tables promise."""
        if alphas is None:
            return bool(np.array_equal(a.supports_, b.supports_) and np.allclose(a.values_, b.values_, rtol=1e-9, atol=0))
        rows = [(a.regularized_size(al), b.regularized_size(al)) for al in alphas]
        return all(np.array_equal(a.supports_[i], b.supports_[j]) and np.isclose(a.values_[i], b.values_[j], rtol=1e-9, atol=0) for i, j in rows)

    # ---- (a), (b) launch-bound: 25 x 20, five folds, eight etas ----------------------------------------------------------------------
    X, y = make_regression(25, 20, n_informative=10, noise=1.0, random_state=0)
    var, cinf = float(np.var(y)), float(np.max(np.abs(X.T @ y / X.shape[0])))
    rels = np.logspace(-2, -0.3, 8)
    etas = rels * cinf
    kw = dict(alpha_min=1e-4 * var, big_M=1000, solver_options=opts)
    sets = [tr for tr, _ in cv.split(X)] + [np.arange(len(y))]
    walls, last = measure({
        "one": lambda: l1l0_profile_cv(X, y, etas=etas, cv=cv, **kw),
        "many": lambda: [[l1l0_profile(X[rows], y[rows], eta=eta, **kw) for rows in sets] for eta in etas],
    })
    grid, many = last["one"], last["many"]
    alphas = np.logspace(-4, 0, 10) * var
    same = all(agree(a, b, alphas) for ta, tb in zip(tables(grid), many) for a, b in zip(ta, tb))
    say("(a) l1 kind: 25 x 20, no intercept, etas = logspace(-2, -0.3, 8) ||X^T y / n||_inf, alpha_min = 1e-4 var y")
    say("    (pruned tables under an l1 term: 'same' compares what they promise, the support and value read at alphas = logspace(-4, 0, 10) var y)")
    report("l1l0_profile_cv", "l1l0_profile", 48, walls, same, grid, [t.solver_info_ for tb in many for t in tb])
    per_eta = [sum(t.solver_info_["descents"] for t in ta) for ta in tables(grid)]
    say(f"    descents per eta, six row sets together, smallest eta first: {per_eta}")
    say(f"    (every problem has the same {grid.solver_info_['problems'][0]['launches']} launch and an equal share of the workgroups: a problem with few "
        "descents leaves its share idle while the others run)")
    say("")
    kw4 = dict(kw, max_groups=4)
    walls, last = measure({
        "one": lambda: l1l0_profile_cv(X, y, etas=etas, cv=cv, **kw4),
        "many": lambda: [[l1l0_profile(X[rows], y[rows], eta=eta, **kw4) for rows in sets] for eta in etas],
    })
    grid, many = last["one"], last["many"]
    same = all(agree(a, b, alphas) for ta, tb in zip(tables(grid), many) for a, b in zip(ta, tb))
    say("(a') l1 kind, small: the same with max_groups = 4")
    report("l1l0_profile_cv", "l1l0_profile", 48, walls, same, grid, [t.solver_info_ for tb in many for t in tb])
    say("")
    retas = np.logspace(-2, 1, 8)
    kw = dict(max_groups=8, big_M=1000, solver_options=opts)
    walls, last = measure({
        "one": lambda: l2l0_profile_cv(X, y, etas=retas, cv=cv, **kw),
        "many": lambda: [l0_profile_cv(X, y, cv=cv, eta=eta, **kw) for eta in retas],
    })
    grid, many = last["one"], last["many"]
    same = all(agree(a, b) for ta, c in zip(tables(grid), many) for a, b in zip(ta, c.profiles_ + [c.full_]))
    say("(b) ridge kind: 25 x 20, no intercept, etas = logspace(-2, 1, 8), max_groups = 8")
    report("l2l0_profile_cv", "l0_profile_cv", 8, walls, same, grid, [i for c in many for i in c.solver_info_["problems"]])
    # ---- (c) node-bound: the 45 x 30 split of profiles/l0_cv.txt, every problem under the budget --------------------------------------------
    X, y = make_regression(n_samples=60, n_features=30, n_informative=8, noise=40.0, bias=-15.0, random_state=0)
    X, _, y, _ = train_test_split(X, y, test_size=0.25, random_state=0)
    retas = np.logspace(-1, 1, 8)
    kw = dict(alpha_min=1e-3 * float(np.var(y)), big_M=1000, fit_intercept=True, solver_options=opts)
    walls, last = measure({
        "one": lambda: l2l0_profile_cv(X, y, etas=retas, cv=cv, **kw),
        "many": lambda: [l0_profile_cv(X, y, cv=cv, eta=eta, **kw) for eta in retas],
    })
    grid, many = last["one"], last["many"]
    same = all(agree(a, b) for ta, c in zip(tables(grid), many) for a, b in zip(ta, c.profiles_ + [c.full_]))
    say("")
    say(f"(c) ridge kind, node-bound: the line-search example's 45 x 30 split, fit_intercept, etas = logspace(-1, 1, 8), alpha_min = 1e-3 var y;")
    say(f"    a problem that does not finish within {max_nodes} nodes stops with its incumbents (two sets of incumbents need not agree)")
    report("l2l0_profile_cv", "l0_profile_cv", 8, walls, same, grid, [i for c in many for i in c.solver_info_["problems"]])
    nb = sum(p["nodes"] for p in grid.solver_info_["problems"])
    ns = sum(i["nodes"] for c in many for i in c.solver_info_["problems"])
    say(f"    nodes/s: one call {nb / float(np.median(walls['one'])):.3e}, the 8 calls {ns / float(np.median(walls['many'])):.3e}")
    say("")
    say("not measured: the default budget of 2^30 nodes per problem (48 node-bound problems under it take minutes per call); the l1 kind at")
    say("25 x 30 or on the 45 x 30 split; a device of fewer than 64 compute units, where the 48 problems exceed two workgroups per CU and run in")
    say("waves; the time workgroups of finished problems idle while other problems run (the engine keeps no such count, so the reading of (a) --")
    say("the call lasts as long as its heaviest problem on a 48th of the device -- rests on the descent counts alone); GridSearchCV fit by fit.")

# the resource line of l0_local_kernel (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage -c csrc/engine_l0.hip):
# the build does not report it, so it is kept here and checked whenever the kernel changes
LOCAL_KERNEL_RESOURCES = ("l0_local_kernel on gfx950: 255 VGPRs, 78 AGPRs, scratch 0 bytes/lane, LDS 0 bytes, 104 SGPRs (156 SGPR spills to "
                          "VGPR lanes, no VGPR spill), 1 wave/SIMD")

LOCAL_OTHER_KERNELS = ("the twelve instantiations of l0_search_kernel compile to the resource lines of the parent commit (compared line by line; "
                       "l0_local_kernels.hpp includes l0_kernels.hpp and changes nothing in it)")
# measured on a CPU with the committed restatement (tests/_l0_local_reference.py) against tests/_l0_reference.brute_force; the
# test tests/test_l0_local_cpu.py asserts what these lines say, case by case
LOCAL_HIT_COUNTS = (
    "how often the rule finds the optimum (CPU, the numpy restatement against brute force; tests/test_l0_local_cpu.py): the law n = 30,",
    "p = 14, AR(1) correlation 0.9, 4 true columns, SNR 2 (_l0_local_reference.hard_law), seeds 0 - 23, alpha in {0.02, 0.05, 0.1} var y, 72 cases:",
    "    the descent alone at the exact optimum in 13 of 72, with swaps in 32 of 72; swaps strictly better in 39, never worse; never below the optimum",
    "    (the prototype of the issue, on its own draw of that law: 11 and 41 of 72, strictly better in 55)",
    "    so on this law the search MISSES the optimum in 40 of 72 cases: it is a local search, and the exact estimators are the yardstick to 128 columns",
)


def local_section(out_path, repeats, max_nodes):
    import subprocess
    import tempfile

    from sklearn.datasets import make_regression

    from sparselm_amd import _engine
    from sparselm_amd.miqp import RegularizedL0, l0_local_search

    dev = _engine.get_engine().device_info()
    name = dev["name"].strip() or "device"
    lines = [f"l0 local search (l0_local_search, slm_solve_l0_local) on {name}, {dev['compute_units']} compute units",
             f"(wall time of whole calls, each ending in a synchronise; every shape warmed first; {repeats} repeats with the variants alternating, "
             "medians with the spread min .. max)", LOCAL_KERNEL_RESOURCES, LOCAL_OTHER_KERNELS, "", *LOCAL_HIT_COUNTS, ""]
    os.makedirs(os.path.dirname(out_path), exist_ok=True)

    def say(line):  # (the file grows line by line: a run that is cut short leaves what it measured)
        lines.append(line)
        print(line, flush=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def clock(fn):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            out = fn()
            return out, (time.perf_counter() - t0) * 1e3

    def fmt(ms):
        return f"{np.median(ms):9.3f} ({min(ms):.3f} .. {max(ms):.3f})"

    # ---- 1. beside the exact search: the reference's 290 x 66 data and 25 x 30 ----------------------------------------------------------
    d = os.path.join(ROOT, "tests", "golden", "reference_examples")
    Xr, yr = np.load(os.path.join(d, "corr.npy")), np.load(os.path.join(d, "energy.npy"))
    Xs, ys = make_regression(25, 30, n_informative=10, noise=1.0, random_state=0)
    for X, y, icpt, big_M, rels, exact_opts in ((Xr, yr, True, 100, np.logspace(-4, -1, 4), {"wide": True, "max_nodes": max_nodes}),
                                                (Xs, ys, False, 1000, np.logspace(-4, 0, 5), {"max_nodes": max_nodes})):
        alphas = rels * float(np.var(y))
        local = lambda: l0_local_search(X, y, alphas=alphas, big_M=big_M, fit_intercept=icpt)  # noqa: E731
        exact = lambda: [RegularizedL0(alpha=a, big_M=big_M, fit_intercept=icpt, solver_options=exact_opts).fit(X, y) for a in alphas]  # noqa: E731
        clock(local), clock(exact)
        t_loc, t_ex, path, ests = [], [], None, None
        for _ in range(repeats):
            (path, ms) = clock(local)
            t_loc.append(ms)
            (ests, ms) = clock(exact)
            t_ex.append(ms)
        say(f"{X.shape[0]} x {X.shape[1]}, fit_intercept = {icpt}, big_M = {big_M}, alphas / var y = {[float(f'{r:.1e}') for r in rels]}; the exact search under "
            f"{max_nodes} nodes per fit")
        say(f"{'what':46s} {'ms per call: median (min .. max)':>36s}")
        say(f"{'l0_local_search, all alphas, max_rounds = 2':46s} {fmt(t_loc):>36s}   rounds {path.rounds_}, swaps {path.swaps_[:, 0].tolist()}, "
            f"sweeps {path.sweeps_[:, 0].tolist()}, converged {path.converged_[:, 0].tolist()}")
        say(f"{'the RegularizedL0 fits together':46s} {fmt(t_ex):>36s}")
        for a, est in enumerate(ests):
            info = est.solver_info_
            kind = "proven optimum" if info["proven_optimal"] else "incumbent (budget ran out)"
            gap = (path.objectives_[a, 0] - info["objective"]) / max(abs(info["objective"]), alphas[a])
            say(f"    alpha / var y = {rels[a]:.1e}: local {path.objectives_[a, 0]:.10e} ({int(path.supports_[a, 0].sum())} columns), exact "
                f"{info['objective']:.10e} ({int(est.active_groups_.sum())} columns, {kind}); relative gap {gap:+.3e}")
        say("    (a call lasts as long as its slowest problem: the sweeps above are the winners'; a start that loses may run up to the cap of 10 000")
        say("    sweeps -- with fewer rows than columns and a small alpha a neighbour's start can hold a singular set of columns -- and the entry")
        say("    reports the winner's counts only, so where a call's time goes beyond them was not measured)")
        say("")

    # ---- 2. wide synthetic problems: the one launch against the host twin on one core ------------------------------------------------------
    exe = os.path.join(tempfile.mkdtemp(), "l0_local_host_bench")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", os.path.join(ROOT, "tools", "l0_local_host_bench.cpp"), "-o", exe], check=True)

    def host(G, c, yy, alphas, etas, big_M, swaps=True):
        p = len(c)
        with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as fh:
            np.array([p, p, len(alphas), int(swaps)], dtype=np.int64).tofile(fh)
            np.array([yy, big_M], dtype=np.float64).tofile(fh)
            for arr in (G, c, alphas, etas):
                np.ascontiguousarray(arr, dtype=np.float64).tofile(fh)
        try:
            out = subprocess.run([exe, fh.name], check=True, capture_output=True, text=True).stdout.splitlines()
        finally:
            os.remove(fh.name)
        words = out[0].split()
        return {"ms": float(words[3]), "changes": int(words[5]), "sweeps": int(words[7]), "swaps": int(words[9]),
                "F": np.array(out[1].split()[1:], dtype=float)}

    say("synthetic: rows of independent standard normal columns, 20 true columns at random places with coefficients +-1, noise 0.5; eta = 0;")
    say("alphas = geomspace(0.003, 0.3, cells) var y; big_M = 100; zero starts.  GPU: Dataset.solve_l0_local on a dataset that holds its Gram")
    say("(the whole call: upload of the cells, ONE launch, read-back, the winners' Gram rows to the host, the polish of every winner).  Host: l0_local_solve<false> of")
    say("csrc/l0_host.hpp, g++ -O2, one core, the cells one after the other, the rule alone (no polish) on numpy's Gram.")
    say(f"{'n x p':>10s} {'cells':>6s} {'GPU ms: median (min .. max)':>34s} {'host ms: median (min .. max)':>36s} {'GPU / host':>11s} {'changes':>9s} {'same F':>7s}")
    wins = {}
    per_change = []
    for n, p in ((200, 512), (400, 1024)):
        rng = np.random.default_rng(p)
        X = rng.standard_normal((n, p))
        beta = np.zeros(p)
        beta[rng.choice(p, 20, replace=False)] = (-1.0) ** np.arange(20)
        y = X @ beta + 0.5 * rng.standard_normal(n)
        G, c, yy = X.T @ X / n, X.T @ y / n, float(y @ y) / n
        with _engine.get_engine().dataset(X, y) as ds:
            for cells in (1, 16, 64, 256):
                alphas = (np.geomspace(0.003, 0.3, cells) if cells > 1 else np.array([0.03])) * float(np.var(y))
                etas = np.zeros(cells)
                gpu = lambda: ds.solve_l0_local(alphas, etas, big_M=100.0)  # noqa: E731
                clock(gpu), host(G, c, yy, alphas, etas, 100.0)
                t_gpu, t_host, res, ref = [], [], None, None
                for _ in range(repeats):
                    (res, ms) = clock(gpu)
                    t_gpu.append(ms)
                    ref = host(G, c, yy, alphas, etas, 100.0)
                    t_host.append(ref["ms"])
                before = np.array([info["descent_objective"] for info in res[3]])
                same = int(np.sum(np.abs(before - ref["F"]) <= 1e-9 * np.maximum(np.abs(ref["F"]), alphas)))
                ratio = np.median(t_gpu) / np.median(t_host)
                wins.setdefault((n, p), []).append((cells, ratio))
                say(f"{f'{n} x {p}':>10s} {cells:6d} {fmt(t_gpu):>34s} {fmt(t_host):>36s} {ratio:11.3f} {ref['changes']:9d} {same:4d}/{cells}")
            if p == 1024:  # ---- 3. the time of one applied change: single cells that differ in their number of changes ----------------
                for rel in (0.3, 0.01, 0.003):
                    alphas = np.array([rel * float(np.var(y))])
                    gpu = lambda: ds.solve_l0_local(alphas, np.zeros(1), big_M=100.0)  # noqa: E731
                    clock(gpu)
                    ts = [clock(gpu)[1] for _ in range(repeats)]
                    ref = host(G, c, yy, alphas, np.zeros(1), 100.0)
                    per_change.append((rel, float(np.median(ts)), ref["changes"], ref["ms"]))
    say("")
    for (n, p), rows in wins.items():
        won = [cells for cells, ratio in rows if ratio < 1.0]
        say(f"{n} x {p}: the launch " + (f"wins from {min(won)} cells on (of 1, 16, 64, 256)" if won else "did not win at any of 1, 16, 64, 256 cells"))
    say("")
    say("time per applied coordinate change at 400 x 1024, single cells (one wavefront), whole calls:")
    for rel, ms, changes, host_ms in per_change:
        say(f"    alpha = {rel:g} var y: {changes:7d} changes, GPU call {ms:9.3f} ms, host rule {host_ms:9.3f} ms")
    (_, t0, c0, h0), (_, t1, c1, h1) = per_change[0], per_change[-1]
    if c1 > c0:
        say(f"    slope between the first and the last: GPU {(t1 - t0) / (c1 - c0) * 1e3:.2f} us per change (one dependent 8 KB row read, the next scan), "
            f"host {(h1 - h0) / (c1 - c0) * 1e3:.2f} us per change")
    say("")
    say("NOT measured: the kernel alone (no event bracket: the whole call is what a caller pays, and it carries the copy of the winners' Gram rows")
    say("to the host for the polish); more than one start per cell; eta > 0; correlated designs, where sweeps and swaps multiply; devices with")
    say("fewer compute units; the host twin on several cores (the cells are independent: a 16-core host divides its column by up to 16).")


# the resource lines of the two kernels of csrc/l0_local_kernels.hpp after row sets went in (same command as above), beside the parent's
LOCAL_CV_RESOURCES = (
    "l0_local_kernel on gfx950: 256 VGPRs, 74 AGPRs, scratch 0 bytes/lane, LDS 0 bytes, 104 SGPRs (163 SGPR spills to VGPR lanes), 1 wave/SIMD",
    "    (the parent, one Gram for all problems: 255 VGPRs, 78 AGPRs, scratch 0, 104 SGPRs, 156 SGPR spills, 1 wave/SIMD)",
    "l0_eliminate_kernel on gfx950: 16 VGPRs, 0 AGPRs, scratch 0 bytes/lane, LDS 0 bytes, 34 SGPRs, no spills, 8 waves/SIMD",
    "the other 101 kernels of engine_l0.hip, the twelve instantiations of the exact search among them: resource lines unchanged, compared line by line",
)


def _single_table(repeats):
    """The 200 x 512 and 400 x 1024 table of local_section, the GPU column alone: {"n x p cells": [ms, ...]}."""
    from sparselm_amd import _engine

    out = {}
    for n, p in ((200, 512), (400, 1024)):
        rng = np.random.default_rng(p)
        X = rng.standard_normal((n, p))
        beta = np.zeros(p)
        beta[rng.choice(p, 20, replace=False)] = (-1.0) ** np.arange(20)
        y = X @ beta + 0.5 * rng.standard_normal(n)
        with _engine.get_engine().dataset(X, y) as ds:
            for cells in (1, 16, 64, 256):
                alphas = (np.geomspace(0.003, 0.3, cells) if cells > 1 else np.array([0.03])) * float(np.var(y))
                ds.solve_l0_local(alphas, np.zeros(cells), big_M=100.0)
                ts = []
                for _ in range(repeats):
                    t0 = time.perf_counter()
                    ds.solve_l0_local(alphas, np.zeros(cells), big_M=100.0)
                    ts.append((time.perf_counter() - t0) * 1e3)
                out[f"{n} x {p} {cells}"] = ts
    return out


def local_cv_section(out_path, repeats, parent_tree):
    """profiles/l0_local_cv.txt: l0_local_cv against the loop it replaces, and the single-row-set path against the parent's."""
    import json
    import subprocess

    from sklearn.model_selection import KFold

    from sparselm_amd import _engine
    from sparselm_amd.miqp import l0_local_cv, l0_local_search

    dev = _engine.get_engine().device_info()
    name = dev["name"].strip() or "device"
    lines = [f"l0 local search over folds (l0_local_cv, slm_solve_l0_local_folds) on {name}, {dev['compute_units']} compute units",
             f"(wall time of whole calls, each ending in a synchronise; every shape warmed first; {repeats} repeats with the variants alternating, "
             "medians with the spread min .. max)", *LOCAL_CV_RESOURCES, ""]
    os.makedirs(os.path.dirname(out_path), exist_ok=True)

    def say(line):  # (the file grows line by line: a run that is cut short leaves what it measured)
        lines.append(line)
        print(line, flush=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")

    def clock(fn):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            out = fn()
            return out, (time.perf_counter() - t0) * 1e3

    def fmt(ms):
        return f"{np.median(ms):9.3f} ({min(ms):.3f} .. {max(ms):.3f})"

    # ---- 1. what l0_local_cv replaces: cv + 1 calls of l0_local_search on the row subsets, each with its own upload and Gram ---------------
    d = os.path.join(ROOT, "tests", "golden", "reference_examples")
    Xr, yr = np.load(os.path.join(d, "corr.npy")), np.load(os.path.join(d, "energy.npy"))
    rng = np.random.default_rng(1024)
    Xw = rng.standard_normal((400, 1024))
    bw = np.zeros(1024)
    bw[rng.choice(1024, 20, replace=False)] = (-1.0) ** np.arange(20)
    yw = Xw @ bw + 0.5 * rng.standard_normal(400)
    say("five folds (KFold without shuffle) and all rows; max_rounds = 2; big_M = 100.  one launch per round: l0_local_cv.  the loop: 6 calls of")
    say("l0_local_search on X[rows], y[rows], each with its own dataset, upload and Gram -- what a user had to write before.")
    for X, y, icpt, rels, what in ((Xr, yr, True, np.logspace(-4, -1, 4), "the reference's 290 x 66 data, fit_intercept, alphas / var y = 1e-4 .. 1e-1 (4)"),
                                   (Xw, yw, False, np.geomspace(0.003, 0.3, 16), "synthetic 400 x 1024 (the law of profiles/l0_local.txt), 16 alphas")):
        alphas = rels * float(np.var(y))
        rows = [tr for tr, _ in KFold(5).split(X)] + [np.arange(X.shape[0])]
        one = lambda: l0_local_cv(X, y, alphas=alphas, cv=KFold(5), fit_intercept=icpt)  # noqa: E731
        loop = lambda: [l0_local_search(X[r], y[r], alphas=alphas, fit_intercept=icpt) for r in rows]  # noqa: E731
        clock(one), clock(loop)
        t_one, t_loop, cv, paths = [], [], None, None
        for _ in range(repeats):
            (cv, ms) = clock(one)
            t_one.append(ms)
            (paths, ms) = clock(loop)
            t_loop.append(ms)
        info = cv.solver_info_
        same = sum(int(np.array_equal(a.supports_, b.supports_)) for a, b in zip(cv.paths_ + [cv.full_], paths))
        say(what)
        say(f"{'what':46s} {'ms per call: median (min .. max)':>36s}")
        say(f"{'l0_local_cv, 6 row sets in each launch':46s} {fmt(t_one):>36s}   launches {info['launches']}, at most {info['problems']} problems each")
        say(f"{'6 calls of l0_local_search':46s} {fmt(t_loop):>36s}   launches {sum(p_.rounds_ for p_ in paths)}")
        ratio = np.median(t_one) / np.median(t_loop)
        say(f"    one-launch / loop = {ratio:.3f}" + ("  -- the one-launch call LOSES here" if ratio >= 1.0 else ""))
        say(f"    sweeps: the largest of ANY problem {info['max_sweeps']}, of the kept winners {info['winner_max_sweeps']}; accepted swaps: any problem "
            f"{info['max_swaps']}, winners {info['winner_max_swaps']}; row sets with the loop's supports: {same} of 6")
        say("")

    # ---- 2. the single-row-set path against the parent commit's, alternating processes on this box ----------------------------------------------
    if parent_tree:
        say("slm_solve_l0_local (one row set) on the parent commit and on this one: the GPU column of profiles/l0_local.txt's table, whole calls.")
        say(f"Fresh processes alternate parent, change, {repeats} times; each warms a shape and times it 3 times; below the median of all its times")
        say("and their min .. max.  Expected: every median of the change inside the parent's own min .. max.")
        runs = {"parent": {}, "change": {}}
        for _ in range(repeats):
            for which, tree in (("parent", parent_tree), ("change", ROOT)):
                env = dict(os.environ, PYTHONPATH=os.path.join(tree, "sparse-lm_amd"))
                got = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", "local-single", "--tree", tree], env=env, check=True,
                                     capture_output=True, text=True, timeout=600).stdout
                for key, ts in json.loads(got.strip().splitlines()[-1]).items():
                    runs[which].setdefault(key, []).extend(ts)
        say(f"{'n x p':>10s} {'cells':>6s} {'parent ms: median (min .. max)':>36s} {'change ms: median (min .. max)':>36s} {'inside':>7s}")
        outside = []
        for key in runs["parent"]:
            n_, _, p_, cells = key.split()
            a, b = runs["parent"][key], runs["change"][key]
            inside = min(a) <= np.median(b) <= max(a)
            if not inside:
                outside.append((key, float(np.median(b)), min(a), max(a)))
            say(f"{f'{n_} x {p_}':>10s} {cells:>6s} {fmt(a):>36s} {fmt(b):>36s} {'yes' if inside else 'NO':>7s}")
        for key, med, lo, hi in outside:
            say(f"    OUTSIDE the parent's range ({'below' if med < lo else 'above'} it): {key} cells, change median {med:.3f} ms against {lo:.3f} .. {hi:.3f}")
        say("")
    say("Host copies for the polish: per row set only the rows of its Gram that its winners hold are fetched (8 ps bytes each; beyond 64 rows one")
    say("strided copy of the stretch that holds them), not the 8 ld^2 bytes of every Gram; what a full fetch would cost was not measured.")
    say("NOT measured: the kernels alone (no event bracket: the whole call is what a caller pays); the cost of the elimination launch by itself;")
    say("more than five folds; starts beside zero in round 0; eta > 0; sample weights (their Grams are built row set by row set, not from the")
    say("folds' complements); correlated designs, where sweeps and swaps multiply; devices with fewer compute units.")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max-nodes", type=int, default=1 << 24)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "l0_search.txt"))
    ap.add_argument("--profile-out", default=os.path.join(ROOT, "profiles", "l0_profile.txt"))
    ap.add_argument("--wide-out", default=os.path.join(ROOT, "profiles", "l0_wide.txt"))
    ap.add_argument("--constrained-out", default=os.path.join(ROOT, "profiles", "l0_constrained.txt"))
    ap.add_argument("--bound-out", default=os.path.join(ROOT, "profiles", "l0_bound.txt"))
    ap.add_argument("--cv-out", default=os.path.join(ROOT, "profiles", "l0_cv.txt"))
    ap.add_argument("--l1-profile-out", default=os.path.join(ROOT, "profiles", "l1l0_profile.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--grid-cv-out", default=os.path.join(ROOT, "profiles", "l0_grid_cv.txt"))
    ap.add_argument("--local-out", default=os.path.join(ROOT, "profiles", "l0_local.txt"))
    ap.add_argument("--local-cv-out", default=os.path.join(ROOT, "profiles", "l0_local_cv.txt"))
    ap.add_argument("--parent-tree", default=None, help="localcv: a built checkout of the parent commit, for the single-row-set comparison")
    ap.add_argument("--tree", default=None, help="local-single: the checkout whose package this process imports")
    ap.add_argument("--only", choices=["search", "profile", "wide", "constrained", "bound", "cv", "l1profile", "gridcv", "local", "localcv",
                                       "local-single"], default=None)
    args = ap.parse_args()
    if args.only == "local-single":  # (a child of localcv: the table as one JSON line)
        import json

        if args.tree:
            sys.path.insert(0, os.path.join(args.tree, "sparse-lm_amd"))
        print(json.dumps(_single_table(3)))
        return
    if args.only == "localcv":
        local_cv_section(args.local_cv_out, max(1, args.repeats), args.parent_tree)
        return
    if args.only == "local":
        local_section(args.local_out, max(1, args.repeats), args.max_nodes)
        return
    if args.only == "gridcv":
        grid_cv_section(args.grid_cv_out, max(1, args.repeats), args.max_nodes)
        return
    if args.only == "l1profile":
        l1_profile_section(args.l1_profile_out, max(1, args.repeats), args.max_nodes)
        return
    if args.only == "cv":
        cv_section(args.cv_out, max(5, args.repeats))
        return
    if args.only in (None, "bound"):
        bound_section(args.bound_out)
    if args.only in (None, "constrained"):
        constrained_section(args.constrained_out, args.max_nodes)
    if args.only in (None, "wide"):
        wide_section(args.wide_out, args.max_nodes)
    if args.only in (None, "profile"):
        profile_section(args.profile_out)
    if args.only not in (None, "search"):
        return
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
