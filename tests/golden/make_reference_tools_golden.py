"""Record what the reference's own helpers (``sparselm.tools``) return around this package's estimators.

tests/test_reference_compat.py compares the package against these numbers, so the suite needs no copy of the reference:
  * ``constrain_coefficients([0, 1], high=2.0, low=-1.0)`` of the reference wrapped around ``Lasso(alpha=1e-3).fit``
    (the unconstrained fit, then the constrained one);
  * ``r2_score_to_cv_error`` of the reference on the predictions of ``Lasso(alpha=0.05, fit_intercept=True)``.
Both fits run with the CPU oracle behind the estimator surface (tests/_oracle_backend.py), as in the tests.

Usage:  python tests/golden/make_reference_tools_golden.py REFERENCE_SRC
        (REFERENCE_SRC: the directory that holds the reference's ``sparselm`` package; writes
        tests/golden/reference_tools_golden.npz)
"""

from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sparse-lm_amd"), os.path.join(ROOT, "tests")]


def main(reference_src):
    sys.path.insert(0, reference_src)
    import sparselm.tools as ref_tools  # numpy-only module of the reference
    from sklearn.metrics import r2_score

    from _oracle_backend import OracleBackend
    from sparselm_amd import _backend
    from sparselm_amd.model import Lasso

    out = {}
    rng = np.random.default_rng(0)
    X = rng.standard_normal((60, 6))
    y = X @ np.array([3.0, -2.0, 0.5, 0.0, 0.0, 1.0]) + 0.01 * rng.standard_normal(60)

    def fit_method(X, y):
        return Lasso(alpha=1e-3, solver_options={"tol": 1e-12}).fit(X, y).coef_

    with _backend.use_backend(OracleBackend()):
        out["constrain_free_coef"] = fit_method(X, y)
        out["constrain_coef"] = ref_tools.constrain_coefficients([0, 1], high=2.0, low=-1.0)(fit_method)(X, y)
    out["constrain_X"], out["constrain_y"] = X, y

    rng = np.random.default_rng(1)
    X = rng.standard_normal((80, 5))
    y = X @ np.arange(1.0, 6.0) + rng.standard_normal(80)
    with _backend.use_backend(OracleBackend()):
        pred = Lasso(alpha=0.05, fit_intercept=True).fit(X, y).predict(X)
    out["r2_X"], out["r2_y"], out["r2_pred"] = X, y, pred
    out["r2_score"] = np.array(r2_score(y, pred))
    out["r2_cv_error"] = np.array(ref_tools.r2_score_to_cv_error(out["r2_score"], y, pred))

    path = os.path.join(HERE, "reference_tools_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
