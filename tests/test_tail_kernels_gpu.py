"""The tail kernels (csrc/tail_kernels.hpp) at every width at which they take another path, small enough to run in seconds:
the register kernel fista_tail_kernel<E> (E = 1, 2, 6), the streaming kernel fista_tail_stream_kernel<E> with unrolled
walks (E = 7, 10), with runtime loops and the feature image in LDS (p = 10 241) and with the image in global scratch
(p = 16 385).  With FLAG_NO_WORKING_SET | FLAG_NO_MODEL_GRAM every iterate comes from the tail kernel; by default that is
the spectral scheme (mode 1), with FLAG_FISTA_ONLY the accelerated one (mode 0).  Penalties: lasso, all three terms on
singleton groups, and a group penalty on real groups of five under a permuted labelling (the last group is smaller where
p is no multiple of five).  Each is a two-point warm path at tol = 1e-9 against oracle.fista at tol = 1e-13, to
1e-6 * max|b| (the bound of test_width_limits_gpu.py).

The cross is trimmed to keep the file quick -- the oracle's p > n solves are most of its time: every width runs the lasso in
both modes; the singleton and the group penalty run in both modes at the seam (6 144 / 6 145) and at the runtime loops
(10 241), and in the spectral mode at one feature in the last slot (1 025) and at the scratch image (16 385).
"""

import os

import numpy as np
import pytest

import oracle
from sparselm_amd import _engine

pytestmark = pytest.mark.gpu

for _v in ("OMP_NUM_THREADS",):
    os.environ.setdefault(_v, "16")

N = 256
PLAIN = _engine.FLAG_NO_WORKING_SET | _engine.FLAG_NO_MODEL_GRAM
WIDTHS = (1024, 1025, 6144, 6145, 10240, 10241, 16385)
SEAM = (6144, 6145)
MODE1_ONLY = (1025, 10241, 16385)
CASES = [(p, "lasso", fista) for p in WIDTHS for fista in (False, True)]
CASES += [(p, pen, fista) for p in SEAM for pen in ("singleton", "groups") for fista in (False, True)]
CASES += [(p, pen, False) for p in MODE1_ONLY for pen in ("singleton", "groups")]
CASES += [(10241, pen, True) for pen in ("singleton", "groups")]  # the image prox on runtime loops, FISTA mode


@pytest.fixture(scope="module")
def eng():
    return _engine.get_engine(0)


_problems = {}


def problem(p, pen):
    """(X, y, groups or None, points, reference solutions): built once per (p, penalty), shared by both modes."""
    if (p, pen) in _problems:
        return _problems[(p, pen)]
    rng = np.random.default_rng(p)
    X = rng.standard_normal((N, p))
    support = rng.choice(p, 5, replace=False)
    groups = None
    if pen == "groups":
        groups = rng.permutation(np.arange(p) // 5).astype(np.int32)
        support = np.flatnonzero(np.isin(groups, groups[support[:2]]))
    y = X[:, support] @ rng.uniform(1.0, 3.0, len(support)) + 0.1 * rng.standard_normal(N)
    g0 = X.T @ y / N
    if pen == "groups":
        top = float(np.max(np.sqrt(np.bincount(groups, weights=g0 * g0))))
        points = [(0.0, 0.5 * top, 0.0), (0.0, 0.3 * top, 0.0)]
    else:
        top = float(np.max(np.abs(g0)))
        points = [(0.5 * top, 0.0, 0.0), (0.3 * top, 0.0, 0.0)] if pen == "lasso" else [(0.4 * top, 0.1 * top, 0.05), (0.25 * top, 0.05 * top, 0.05)]
    gidx, G = oracle.group_index(groups, p)
    refs, b = [], None
    for sa, sb, sd in points:
        b, _ = oracle.fista(X, y, sa, sb, sd, gidx, G, beta0=b, tol=1e-13)
        refs.append(b)
    _problems[(p, pen)] = (X, y, groups, G, points, refs)
    return _problems[(p, pen)]


@pytest.mark.parametrize("p,pen,fista", CASES)
def test_tail_kernel_widths(eng, p, pen, fista):
    X, y, groups, G, points, refs = problem(p, pen)
    with eng.dataset(X, y) as ds:
        if groups is not None:
            ds.set_groups(groups, G)
        res = ds.solve_path(points, tol=1e-9, flags=PLAIN | (_engine.FLAG_FISTA_ONLY if fista else 0), want_group_norms=groups is not None)
    print(p, pen, "fista" if fista else "spectral", "mode", res.mode, "n_iter", res.n_iter,
          "err", [float(np.max(np.abs(res.betas[k] - refs[k])) / np.max(np.abs(refs[k]))) for k in range(2)])
    assert res.converged
    assert list(res.mode) == [0 if fista else 1] * 2
    for k in range(2):
        top = float(np.max(np.abs(refs[k])))
        assert top > 0
        assert np.max(np.abs(res.betas[k] - refs[k])) <= 1e-6 * top
        if groups is not None:
            norms = np.sqrt(np.bincount(groups, weights=res.betas[k] ** 2, minlength=G))
            assert np.max(np.abs(res.group_norms[k] - norms)) <= 1e-12 * max(float(np.max(norms)), 1.0)
