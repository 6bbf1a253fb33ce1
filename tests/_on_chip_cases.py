"""Case table of the on-chip solver's shape tests (tests/test_on_chip_shapes_cpu.py keeps it honest without a GPU,
tests/test_on_chip_shapes_gpu.py runs it): the widths, row counts, row weights, faces and result routes at which
`small_solve_kernel` (csrc/small_kernels.hpp) and `PathCall::run_on_chip` (csrc/engine_path.hip) change path.

Nothing here is a number copied from a run.  The shapes are derived from the constants of the sources, read as text, by the
formulas of the code they stand in (`layout`); the inputs are seeded; the references are `oracle.fista` at tol 1e-14 on
the rows and weights a lane sees, computed once per case and shared.
"""

from __future__ import annotations

import functools
import os
import re
import time

import numpy as np

import oracle

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "sparse-lm_amd", "csrc")

CHIP_TOL = 1e-12     # tolerance of the on-chip calls
ORACLE_TOL = 1e-14   # tolerance of the reference
UNIQUE_EIG = 1e-6    # lambda_min / lambda_max of the Gram of the rows that count, below which coefficients are not compared


# ---- the constants, as the sources state them ------------------------------------------------------------------------
def _int_expr(text):
    """`156 * 1024` -> 159744: products of integer literals only."""
    out = 1
    for tok in text.split("*"):
        out *= int(tok.strip())
    return out


def read_constants(csrc=CSRC):
    with open(os.path.join(csrc, "small_kernels.hpp")) as f:
        small = f.read()
    with open(os.path.join(csrc, "engine_internal.hpp")) as f:
        internal = f.read()
    with open(os.path.join(csrc, "engine_path.hip")) as f:
        path = f.read()

    def one(pattern, text, what):
        m = re.search(pattern, text)
        assert m is not None, f"{what}: not found in the source any more -- re-derive the case table"
        return m.group(1)

    c = {
        "SM_PMAX": _int_expr(one(r"constexpr int SM_PMAX = ([0-9* ]+);", small, "SM_PMAX")),
        "SM_THREADS": _int_expr(one(r"constexpr int SM_THREADS = ([0-9* ]+);", small, "SM_THREADS")),
        "SM_LDS_BYTES": _int_expr(one(r"constexpr int SM_LDS_BYTES = ([0-9* ]+);", small, "SM_LDS_BYTES")),
        "ONE_WAVE_MAX": int(one(r"const bool one_wave = p <= (\d+);", small, "one_wave")),
        "WIDE_ABOVE": int(one(r"const bool wide = p > (\d+);", small, "wide")),
        "GRAM_MAXB": int(one(r"constexpr int MAXB = (\d+);", small, "MAXB of sm_build_gram")),
        "kSmallOutDoubles": _int_expr(one(r"constexpr size_t kSmallOutDoubles = ([0-9* ]+);", internal, "kSmallOutDoubles")),
        "kSnapInfos": _int_expr(one(r"static const int kSnapInfos = ([0-9* ]+);", internal, "kSnapInfos")),
        "CHIP_DOUBLES": int(one(r"ds->p <= SM_PMAX && \(double\)ds->n \* \(double\)ds->ld <= (\d+)\.0", path, "the n * ld bound of small_ok")),
    }
    # SM_FACE_HEAD = 128 + 4 * SM_PMAX
    head = re.search(r"constexpr int SM_FACE_HEAD = (\d+) \+ (\d+) \* SM_PMAX;", small)
    assert head is not None, "SM_FACE_HEAD: not found in the source any more -- re-derive the case table"
    c["SM_FACE_HEAD"] = int(head.group(1)) + int(head.group(2)) * c["SM_PMAX"]
    return c


CONSTANTS = read_constants()


# ---- the formulas of the kernel and its host code ----------------------------------------------------------------------
def layout(p, c=None):
    """What small_solve_kernel, sm_build_gram and run_on_chip compute from the width p."""
    c = CONSTANTS if c is None else c
    ld = 16 * ((p + 15) // 16)                                      # row stride of the device copy of X
    stage_doubles = (c["SM_LDS_BYTES"] - 8 * (p * p + 3 * p) - 64) // 8  # run_on_chip
    nb = (p + 1 + 3) >> 2                                           # sm_build_gram: block rows of [X, y]
    nblocks = nb * (nb + 1) // 2
    mchunk = (((p + 3) >> 2) + 7) & ~7                              # rows of G per wavefront in the product
    ranges = [(min(w * mchunk, p), min((w + 1) * mchunk, p)) for w in range(c["SM_THREADS"] // 64)]
    free = stage_doubles - 3 * p - c["SM_FACE_HEAD"]               # sm_face_cap(stage_doubles - 3 p)
    cap = 0
    while cap < c["SM_PMAX"] and (cap + 1) * (cap + 2) // 2 <= free:
        cap += 1
    return {
        "ld": ld,
        "stage_doubles": stage_doubles,
        "nb": nb,
        "nblocks": nblocks,
        "blocks_per_thread": -(-nblocks // c["SM_THREADS"]),
        "rows_per_chunk": stage_doubles // (4 * nb),
        "n_max": c["CHIP_DOUBLES"] // ld,
        "one_wave": p <= c["ONE_WAVE_MAX"],
        "wide": p > c["WIDE_ABOVE"],
        "mchunk": mchunk,
        "ranges": ranges,
        "face_cap": cap,
    }


WIDTHS = (1, 2, 31, 32, 33, 63, 64, 65, 87, 88, 95, 96, 97, 123, 124, 127, 128)
ROW_WIDTHS = (16, 64, 97, 128)
FACE_WIDTHS = (40, 41, 42, 43)


def row_counts(p):
    """The row counts of part (b) at width p, and the first one the chip does not take."""
    lay = layout(p)
    rpc = lay["rows_per_chunk"]
    return (1, 2, 3, rpc - 1, rpc, rpc + 1, 2 * rpc + 3, lay["n_max"]), lay["n_max"] + 1


def weight_shapes():
    """(p, n) of part (c): one row more than a chunk at 33, two chunks and three rows at 97, and the chip's last shape at 128
    (forty-two chunks and a short one) -- the last two are shapes of part (b)."""
    return ((33, layout(33)["rows_per_chunk"] + 1), (97, 2 * layout(97)["rows_per_chunk"] + 3), (128, layout(128)["n_max"]))


# ---- inputs -------------------------------------------------------------------------------------------------------------
def _seed(*parts):
    return np.random.default_rng([0x0C41] + [int(x) for x in parts])


def _gaussian(rng, n, p):
    """i.i.d. Gaussian design, min(7, p) true coefficients, noise 0.5, an offset in y."""
    X = rng.standard_normal((n, p))
    k = min(7, p)
    beta = np.zeros(p)
    beta[rng.choice(p, k, replace=False)] = rng.uniform(1.0, 3.0, k) * rng.choice([-1.0, 1.0], k)
    y = X @ beta + 0.5 * rng.standard_normal(n) + 3.0
    return X, y


def _ar1(rng, n, p, rho=0.95):
    E = rng.standard_normal((n, p))
    X = E.copy()
    for j in range(1, p):
        X[:, j] = rho * X[:, j - 1] + np.sqrt(1 - rho**2) * E[:, j]
    return X


def _groups_of_five(rng, p):
    """Groups of five under a permuted labelling (the kernel works in group-sorted order: the permutation is what makes
    `order` matter); the last group is smaller where 5 does not divide p."""
    return rng.permutation(np.arange(p) // 5)


def _scales(X, y, w, n_eff, groups):
    """alpha_max of the l1 term and of the group term on the rows the lane sees."""
    c = X.T @ (w * y) / n_eff
    amax = float(np.max(np.abs(c)))
    if groups is None:
        return amax, amax
    G = int(groups.max()) + 1
    return amax, float(np.max(np.sqrt(np.bincount(groups, weights=c * c, minlength=G))))


def _points(kind, amax, gmax, n_points=2):
    """A warm path of `n_points` points of one penalty kind, the last at the strength the issue names."""
    f = np.geomspace(2.0 ** (n_points - 1), 1.0, n_points)
    if kind == "lasso":
        return [(0.3 * amax * s, 0.0, 0.0) for s in f]
    if kind == "group":
        return [(0.0, 0.3 * gmax * s, 0.0) for s in f]
    if kind == "sgl":
        return [(0.1 * amax * s, 0.15 * gmax * s, 0.0) for s in f]
    if kind == "sgl_ridge":
        return [(0.1 * amax * s, 0.15 * gmax * s, 0.2) for s in f]
    raise ValueError(kind)


def _lane(points, n, row_weight=None, n_eff=None, compare="coef", **extra):
    return dict(points=[tuple(map(float, pt)) for pt in points], row_weight=row_weight, n_eff=n_eff, compare=compare, **extra)


def _case(tag, X, y, groups, lanes, expect):
    return dict(tag=tag, X=X, y=y, groups=groups, lanes=lanes, expect=expect)


def width_cases(p):
    """(a) n = 2 p + 7 rows; lasso at 0.3 alpha_max, a group penalty on permuted groups of five, sparse-group plus ridge; two
    points each.  Every point must be settled on chip."""
    n = 2 * p + 7
    out = []
    for k, kind in enumerate(("lasso", "group", "sgl_ridge")):
        rng = _seed(1, p, k)
        X, y = _gaussian(rng, n, p)
        groups = None if kind == "lasso" else _groups_of_five(rng, p)
        amax, gmax = _scales(X, y, np.ones(n), n, groups)
        out.append(_case(f"width-{p}-{kind}", X, y, groups, [_lane(_points(kind, amax, gmax), n)], "chip"))
    return out


def row_cases(p):
    """(b) the row counts around the chunk of the Gram build, the smallest ones, the chip's last shape and the first beyond it;
    lasso and sparse-group.  n < 2 p: by objective and certificate; n >= 2 p: by coefficients as well.

    A stated limit of the kernel, met at 1 x 128: a point with group norms gets 320 products and eight Newton steps, and one
    whose groups are still sliding towards zero when those are spent goes to the general path (small_kernels.hpp, the loop of
    the points with group norms).  On a Gram matrix of rank one at full width the first proximal step from zero brings in
    most of the 26 groups and all but one have to slide out again: at (0.1 alpha_max, 0.15 group alpha_max) the chip gave the
    point up (the general path then settled it in 166 passes, one coefficient in the support).  The edge under test is the
    staging of fewer rows than there are staging wavefronts, not that iteration, so the sparse-group strength of n = 1, 2, 3
    is doubled -- fewer groups enter at the first step -- and the rows keep their `mode == 2` assertion."""
    counts, beyond = row_counts(p)
    out = []
    for n in counts + (beyond,):
        for k, kind in enumerate(("lasso", "sgl")):
            rng = _seed(2, p, n, k)
            X, y = _gaussian(rng, n, p)
            groups = None if kind == "lasso" else _groups_of_five(rng, p)
            amax, gmax = _scales(X, y, np.ones(n), n, groups)
            compare = "coef" if n >= 2 * p else "objective"
            if kind == "sgl" and n < 4:  # (the limit of the docstring)
                amax, gmax = 2.0 * amax, 2.0 * gmax
            out.append(_case(f"rows-{p}-{n}-{kind}", X, y, groups, [_lane(_points(kind, amax, gmax, 1), n, compare=compare)],
                             "general" if n == beyond else "chip"))
    return out


def weight_cases(p, n):
    """(c) three lanes in one call: a 0/1 fold mask with its n_eff; general weights in (0, 2), a seventh of them zero; a mask
    that leaves fewer rows than p although n > p (by objective)."""
    assert n > p
    out = []
    for k, kind in enumerate(("lasso", "sgl")):
        rng = _seed(3, p, n, k)
        X, y = _gaussian(rng, n, p)
        groups = None if kind == "lasso" else _groups_of_five(rng, p)
        fold = (rng.permutation(n) % 5 != 2).astype(float)
        general = rng.uniform(0.0, 2.0, n)
        general[rng.permutation(n)[: n // 7]] = 0.0
        few = np.zeros(n)
        few[rng.choice(n, p // 2, replace=False)] = 1.0
        lanes = []
        for w, n_eff, compare in ((fold, int(fold.sum()), "coef"), (general, None, "coef"), (few, int(few.sum()), "objective")):
            amax, gmax = _scales(X, y, w, n_eff or n, groups)
            lanes.append(_lane(_points(kind, amax, gmax, 2), n, row_weight=w, n_eff=n_eff, compare=compare))
        out.append(_case(f"weights-{p}-{n}-{kind}", X, y, groups, lanes, "chip"))
    return out


def face_cases():
    """(d) AR(1) columns, rho = 0.95, every coefficient of the truth at work and a penalty small enough that the minimiser's
    support is the whole width: faces of 40, 41, 42, 43 unknowns (one per residue mod 4), 128 unknowns where the factor holds
    65, and a group penalty at 42.  Whichever route answers must be right; the mode is reported, not asserted."""
    out = []
    for p, n, kind in [(q, 200, "lasso") for q in FACE_WIDTHS] + [(128, 1024, "lasso"), (42, 200, "group")]:
        rng = _seed(4, p, n, kind == "group")
        X = _ar1(rng, n, p)
        y = X @ rng.uniform(1.0, 3.0, p) + 0.5 * rng.standard_normal(n)
        groups = None if kind == "lasso" else _groups_of_five(rng, p)
        amax, gmax = _scales(X, y, np.ones(n), n, groups)
        pts = [(1e-3 * amax, 0.0, 0.0)] if kind == "lasso" else [(0.0, 1e-3 * gmax, 0.0)]
        out.append(_case(f"face-{p}-{n}-{kind}", X, y, groups, [_lane(pts, n)], None))
    return out


ROUTE_SHAPE = (300, 128)


def route_calls():
    """(e) four calls on one 300 x 128 dataset, lanes of different path lengths, alphas and l1 weights:
    staged coefficients with the records in the snapshot / fetched separately, coefficients by copy commands, and group norms
    from sixteen lanes.  Returns (X, y, groups, {name: (lanes, want_group_norms)})."""
    n, p = ROUTE_SHAPE
    rng = _seed(5)
    X, y = _gaussian(rng, n, p)
    groups = _groups_of_five(rng, p)
    amax, gmax = _scales(X, y, np.ones(n), n, groups)

    def lanes(lengths, lo):
        out = []
        for i, K in enumerate(lengths):
            top = 0.9 - 0.011 * i  # (every lane its own alphas)
            a = rng.uniform(0.5, 1.5, p)
            if i % 2 == 0:
                pts = [(amax * s, 0.0, 0.0) for s in np.geomspace(top, lo * top, K)]
            else:
                pts = [(0.4 * amax * s, 0.6 * gmax * s, 0.0) for s in np.geomspace(top, lo * top, K)]
            out.append(_lane(pts, n, a=a))
        return out

    calls = {
        "snapshot+staged": (lanes([1, 2, 3, 4, 5], 0.3), False),
        "fetched+staged": (lanes([2 + i % 5 for i in range(20)], 0.3), False),
        "fetched+copied": (lanes([(4, 5, 6, 5)[i % 4] for i in range(64)], 0.3), False),
        "group-norms": (lanes([3 + i % 5 for i in range(16)], 0.3), True),
    }
    return X, y, groups, calls


def total_points(lanes):
    return sum(len(lane["points"]) for lane in lanes)


# ---- what a lane sees, its reference, its certificate ----------------------------------------------------------------------
def lane_penalties(case, lane, k):
    """(a, b, d, gidx, G) of point k of a lane, as full vectors."""
    p = case["X"].shape[1]
    gidx, G = oracle.group_index(case["groups"], p)
    sa, sb, sd = lane["points"][k]
    a = np.ones(p) if lane.get("a") is None else np.asarray(lane["a"], dtype=float)
    return sa * a, sb * np.ones(G), sd * np.ones(G), gidx, G


def lane_rows(case, lane):
    """(rows, targets) the oracle solves on: the training rows of a 0/1 mask (n_eff = their number), the rows scaled by
    sqrt(w) for general weights (1/n stays the dataset's)."""
    X, y, w = case["X"], case["y"], lane["row_weight"]
    if w is None:
        return X, y
    if lane["n_eff"] is not None:
        assert set(np.unique(w)) <= {0.0, 1.0} and int(w.sum()) == lane["n_eff"]
        keep = w == 1.0
        return X[keep], y[keep]
    s = np.sqrt(w)
    return X * s[:, None], y * s


def numpy_gradient(case, lane, beta):
    """X^T (w * (X b - y)) / n_eff, from the case's own arrays."""
    X, y = case["X"], case["y"]
    w = np.ones(len(y)) if lane["row_weight"] is None else lane["row_weight"]
    n_eff = lane["n_eff"] if lane["n_eff"] is not None else len(y)
    return X.T @ (w * (X @ beta - y)) / n_eff


def certificate(case, lane, k, beta):
    """(KKT residual from numpy's gradient, max |g|) of point k at beta."""
    a, b, d, gidx, G = lane_penalties(case, lane, k)
    g = numpy_gradient(case, lane, beta)
    return oracle.kkt_residual(g, beta, a, b, d, gidx, G), float(np.max(np.abs(g)))


def lane_objective(case, lane, k, beta):
    Xl, yl = lane_rows(case, lane)
    a, b, d, gidx, G = lane_penalties(case, lane, k)
    return oracle.objective(Xl, yl, beta, a, b, d, gidx, G)


def _lane_reference(case, lane):
    Xl, yl = lane_rows(case, lane)
    t0 = time.perf_counter()
    betas, converged, beta = [], True, None
    for k in range(len(lane["points"])):
        a, b, d, gidx, G = lane_penalties(case, lane, k)
        beta, info = oracle.fista(Xl, yl, a, b, d, gidx, G, beta0=beta, tol=ORACLE_TOL, max_iter=500000)
        converged = converged and bool(info["converged"])
        betas.append(beta)
    eig = np.linalg.eigvalsh(Xl.T @ Xl)
    return dict(betas=np.array(betas), converged=converged, seconds=time.perf_counter() - t0,
                unique=bool(eig[0] >= UNIQUE_EIG * eig[-1]))


_REFERENCES: dict = {}


def reference(case):
    """The oracle's answers of every lane of a case, computed once: a list of dicts with `betas` (K, p), `converged`,
    `unique` (the Gram of the rows that count has lambda_min >= 1e-6 lambda_max) and `seconds`."""
    if case["tag"] not in _REFERENCES:
        _REFERENCES[case["tag"]] = [_lane_reference(case, lane) for lane in case["lanes"]]
    return _REFERENCES[case["tag"]]


@functools.lru_cache(maxsize=None)
def cases(part, *key):
    """The case lists, built once: cases("width", p), cases("rows", p), cases("weights", p, n), cases("faces")."""
    return tuple({"width": width_cases, "rows": row_cases, "weights": weight_cases, "faces": face_cases}[part](*key))
