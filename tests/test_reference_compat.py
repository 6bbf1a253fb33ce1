"""The reference's own helper code around sparselm_amd estimators.

What the reference's ``sparselm.tools`` returned around our fits is recorded in tests/golden/reference_tools_golden.npz
(tests/golden/make_reference_tools_golden.py); here the package's counterparts, on CPU with the oracle behind the
surface, must reproduce those numbers from the same inputs.  Nothing from the reference is copied into this repo.
"""

import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_tools_golden.npz")


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def test_reference_constrain_coefficients_wraps_our_fit(recorded):
    # reference src/sparselm/tools.py:14-97 used the way its docstring shows, around our estimator
    from _oracle_backend import OracleBackend
    from sparselm_amd import _backend
    from sparselm_amd.model import Lasso
    from sparselm_amd.tools import constrain_coefficients

    X, y = recorded["constrain_X"], recorded["constrain_y"]

    def fit_method(X, y):
        return Lasso(alpha=1e-3, solver_options={"tol": 1e-12}).fit(X, y).coef_

    with _backend.use_backend(OracleBackend()):
        free = fit_method(X, y)
        assert free[0] > 2.5
        coefs = constrain_coefficients([0, 1], high=2.0, low=-1.0)(fit_method)(X, y)
    assert coefs[0] == 2.0 and coefs[1] == -1.0
    assert abs(coefs[5] - 1.0) < 0.5
    np.testing.assert_allclose(free, recorded["constrain_free_coef"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(coefs, recorded["constrain_coef"], rtol=0, atol=1e-9)


def test_reference_r2_to_cv_error_on_our_predictions(recorded):
    from _oracle_backend import OracleBackend
    from sklearn.metrics import r2_score
    from sparselm_amd import _backend
    from sparselm_amd.model import Lasso
    from sparselm_amd.tools import r2_score_to_cv_error

    X, y = recorded["r2_X"], recorded["r2_y"]
    with _backend.use_backend(OracleBackend()):
        pred = Lasso(alpha=0.05, fit_intercept=True).fit(X, y).predict(X)
    np.testing.assert_allclose(pred, recorded["r2_pred"], rtol=0, atol=1e-9)
    err = r2_score_to_cv_error(r2_score(y, pred), y, pred)
    assert np.isfinite(err) and err >= 0
    np.testing.assert_allclose(err, recorded["r2_cv_error"], rtol=1e-9)
