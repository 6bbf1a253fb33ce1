"""Both directions of the judge of the working-set model solver (tests/_model_reference.py), without a GPU.

Correct solves pass: the reference minimiser agrees with oracle.fista on a design whose Gram is the model's G, meets
settled_bound at tol = 0, and the faultless numpy transcription of the kernel's iteration passes ``judge_settled``.
Defective solves are flagged: each fault of ``FAULTS`` put into the transcription exceeds settled_bound or breaks the
write-back contract.
"""

import numpy as np
import pytest

import oracle
from _model_reference import (
    FAULTS,
    K_ROUND_FLOOR,
    PENALTIES,
    WS_INNER_TOL,
    judge_settled,
    make_case,
    model_kkt,
    model_minimiser,
    model_value,
    settled_bound,
    spectrum,
    support_case,
    transcript_solve,
    ws_K,
    ws_tpc,
)

GROUPS = {"group": [1, 2, 8, 5], "sparse_group": [3, 4, 9], "ridged_group": [2, 6, 8]}


def _case(penalty, seed=3, **kw):
    sizes = GROUPS.get(penalty)
    k = sum(sizes) if sizes else 16
    return make_case(k, 40, seed, penalty=penalty, group_sizes=sizes, **kw)


def test_constants_come_from_the_headers():
    assert WS_INNER_TOL == 0.05
    assert K_ROUND_FLOOR == 16.0 * 2.0**-52


@pytest.mark.parametrize("penalty", PENALTIES)
def test_minimiser_agrees_with_the_oracle_fista(penalty):
    c = _case(penalty)
    m = c.mdl
    k = m.k
    # a design whose Gram is G and whose gradient at z0 is g0: X = sqrt(k) chol(G)^T, X^T y / k = G z0 - g0
    Lc = np.linalg.cholesky(m.G)
    X = np.sqrt(k) * Lc.T
    y = np.linalg.solve(X.T, k * (m.G @ m.z0 - m.g0))
    np.testing.assert_allclose(X.T @ X / k, m.G, rtol=0, atol=1e-14 * np.abs(m.G).max() * k)
    beta, info = oracle.fista(X, y, m.a, m.b, m.d, m.gidx, m.ng, L=1.02 * spectrum(m)[1], tol=1e-14, max_iter=400000)
    assert info["converged"]
    ref = model_minimiser(m)
    lam_min, lam_max = spectrum(m)
    # oracle.fista stops at a prox-gradient residual of 1e-14 ||beta||: (lambda_max + L) / lambda_min times that in distance
    bound = 2.02 * lam_max / lam_min * 1e-14 * np.linalg.norm(beta) + 64 * k * 2.0**-52 * np.linalg.norm(beta)
    assert np.linalg.norm(beta - ref.x.astype(np.float64)) <= bound
    assert np.array_equal(beta != 0.0, ref.x != 0.0)
    # ... and it meets the bound of a settled solve at tol = 0
    assert ref.kkt <= settled_bound(m, ref.x.astype(np.float64), 0.0, lam_max)
    assert float(model_value(m, ref.x)) <= float(model_value(m, beta)) + 1e-13 * abs(float(model_value(m, beta)))


@pytest.mark.parametrize("penalty", PENALTIES)
def test_model_kkt_is_the_oracle_kkt_residual(penalty):
    c = _case(penalty, seed=5)
    m = c.mdl
    x = model_minimiser(m).x.astype(np.float64)
    x = x + 1e-3 * np.random.default_rng(0).standard_normal(m.k) * (x != 0.0)
    grad = m.g0 + m.G @ (x - m.z0)
    want = oracle.kkt_residual(grad, x, m.a, m.b, m.d, m.gidx, m.ng)
    assert want > 1e-6
    assert abs(float(model_kkt(m, x)) - want) <= 1e-12 * want


def _run(c, fault=None):
    out = transcript_solve(c.mdl, c.cols, c.p, c.zprev, c.gprev, c.z_start, c.tol, c.mode, fault=fault)
    pad = out.x_positions[c.k:]
    bad, fig = judge_settled(c.mdl, c.cols, c.zprev, c.z_start, c.mode, c.tol, out.z[0], out.beta[0], int(out.served[0]),
                             float(out.Lw[0]), padding=pad)
    return out, bad, fig


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("penalty", PENALTIES)
def test_faultless_transcription_passes(penalty, mode):
    c = _case(penalty, seed=7, mode=mode)
    out, bad, fig = _run(c)
    assert out.settled and out.inner_iters < 400
    assert bad == [], (bad, fig)


def _nnz_tail_case():
    """nnz = 1 mod 12 TPC non-zero entries of x - z0 at every iterate: the batch tail of the listed product."""
    k = 64
    c = support_case(k, 100, 12 * ws_tpc(ws_K(k)) + 1, 11)
    assert int(np.count_nonzero(model_minimiser(c.mdl).x)) == c.nnz
    return c


_FAULT_CASE = {
    "drop_nnz_tail": _nnz_tail_case,
    "drop_last_column": lambda: _case("lasso", seed=13, strength=0.02),
    "no_z0_shift": lambda: _case("lasso", seed=13),
    "group_norm_short": lambda: _case("group", seed=13, strength=0.1),
    "group_threshold_pa": lambda: _case("sparse_group", seed=13, strength=0.1),
    "prox_unscaled": lambda: _case("lasso", seed=13),
    "no_ridge": lambda: _case("weighted_l1_ridge", seed=13),
    "padding_nonzero": lambda: make_case(13, 40, 13, penalty="lasso"),
    "outside_not_reset": lambda: _case("lasso", seed=13),
    "beta_in_mode1": lambda: _case("lasso", seed=13, mode=1),
}


def test_every_fault_has_a_case():
    assert set(_FAULT_CASE) == set(FAULTS)


@pytest.mark.parametrize("fault", FAULTS)
def test_each_fault_is_flagged(fault):
    c = _FAULT_CASE[fault]()
    _, clean, fig = _run(c)
    assert clean == [], (clean, fig)  # the same case passes without the fault
    out, bad, fig = _run(c, fault=fault)
    assert bad != [], (fault, fig)
