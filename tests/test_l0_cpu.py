"""The exact l0 estimators without a GPU: the brute-force reference the GPU tests compare against, the public surface
(names, constructor signatures, parameter validation before any device is touched).

Mirrors /root/reference/tests/test_miqp.py:33-66 (perfect signal recovery) and :226-237 (bad input)."""

import ast
import inspect
import os

import numpy as np
import pytest
from sklearn.datasets import make_regression, make_sparse_coded_signal

from _l0_reference import brute_force, forward_stepwise, objective_of, search_rank

REFERENCE_SRC = "/root/reference/src/sparselm/model/_miqp"

# (name, default) in order, as the reference's constructors have them (_best_subset.py:100-112, 220-234;
# _regularized_l0.py:120-132, 502-516)
_TAIL = [("ignore_psd_check", True), ("fit_intercept", False), ("copy_X", True), ("warm_start", False), ("solver", None),
         ("solver_options", None)]
SIGNATURES = {
    "BestSubsetSelection": [("groups", None), ("sparse_bound", 100), ("big_M", 100), ("hierarchy", None)] + _TAIL,
    "RidgedBestSubsetSelection": [("groups", None), ("sparse_bound", 100), ("eta", 1.0), ("big_M", 100), ("hierarchy", None),
                                  ("tikhonov_w", None)] + _TAIL,
    "RegularizedL0": [("groups", None), ("alpha", 1.0), ("big_M", 100), ("hierarchy", None)] + _TAIL,
    "L2L0": [("groups", None), ("alpha", 1.0), ("eta", 1.0), ("big_M", 100), ("hierarchy", None), ("tikhonov_w", None)] + _TAIL,
}


def test_brute_force_recovers_a_perfect_signal():
    # /root/reference/tests/test_miqp.py:33-43 with the brute force in the solver's place
    y, D, code = make_sparse_coded_signal(n_samples=1, n_components=24, n_features=12, n_nonzero_coefs=6, random_state=0)
    X, y, beta = np.asarray(D).T, np.ravel(y), np.ravel(code)
    assert X.shape == (12, 24) and np.count_nonzero(beta) == 6
    ref = brute_force(X, y, K=6)
    np.testing.assert_array_equal(np.flatnonzero(beta), np.flatnonzero(ref["coef"]))
    np.testing.assert_array_almost_equal(beta, ref["coef"], decimal=6)
    np.testing.assert_array_equal(ref["active"], beta != 0)


def test_brute_force_box_ridge_and_hierarchy_are_consistent():
    X, y = make_regression(40, 8, n_informative=4, noise=1.0, random_state=3)
    free = brute_force(X, y, K=3)
    assert abs(free["objective"] - objective_of(X, y, free["coef"], 3)) <= 1e-12 * abs(free["objective"])
    boxed = brute_force(X, y, K=3, big_M=0.5 * np.max(np.abs(free["coef"])))
    assert boxed["objective"] > free["objective"] and np.max(np.abs(boxed["coef"])) <= 0.5 * np.max(np.abs(free["coef"])) * (1 + 1e-12)
    ridged = brute_force(X, y, K=3, eta=1.0)
    assert np.linalg.norm(ridged["coef"]) < np.linalg.norm(free["coef"])
    # every feature needs another one, in a ring: a feasible support is all eight or none, and K = 4 < 8 leaves none
    chained = [[7]] + [[i] for i in range(7)]
    assert not brute_force(X, y, K=4, hierarchy=chained)["active"].any()
    cols, rss = forward_stepwise(X, y, 3)
    assert rss >= (2 * 40) * free["objective"] + y @ y - 1e-9 * (y @ y)  # greedy is never better than the optimum


def test_search_rank_on_a_hand_made_case():
    """Four columns that touch one row each: c_j = x_j y_j / 4 and G_jj = x_j^2 / 4, so a column's score is y_j^2 / 4 whatever
    its scale -- 1, 2.25, 2.25 (an exact tie: the lower label goes first) and 0.25."""
    X = np.diag([2.0, 1.0, 1.0, 3.0])
    y = np.array([2.0, 3.0, -3.0, 1.0])
    assert search_rank(X, y).tolist() == [2, 0, 1, 3]
    assert search_rank(X, y, eta=0.1, W=np.eye(4)).tolist() == [2, 0, 1, 3]
    # groups by sorted label: 3 -> {column 2}: 2.25; 5 -> {column 3}: 0.25; 7 -> {columns 0, 1}: (1 + 0.5625) / (1 + 0.25) = 1.25
    assert search_rank(X, y, groups=[7, 7, 3, 5]).tolist() == [0, 2, 1]
    # a column of zeros scores zero and goes last; equal scores keep the order of the labels
    assert search_rank(np.diag([1.0, 0.0, 1.0]), np.array([1.0, 5.0, 1.0])).tolist() == [0, 2, 1]


def test_max_size_closes_a_penalised_problem_like_the_full_enumeration():
    X, y = make_regression(40, 10, n_informative=3, noise=1.0, random_state=4)
    alpha = 0.02 * float(y @ y) / (2 * 40)
    full = brute_force(X, y, alpha=alpha)
    assert full["closed"] and full["n_supports"] == 2**10 and 0 < full["active"].sum() <= 4
    part = brute_force(X, y, alpha=alpha, max_size=4)
    assert part["closed"] and part["n_supports"] == 1 + 10 + 45 + 120 + 210
    np.testing.assert_array_equal(part["active"], full["active"])
    assert part["objective"] == full["objective"] and part["coef"].tobytes() == full["coef"].tobytes()
    assert 0 < part["gap"] <= full["gap"] and part["kappa"] == full["kappa"]
    # a bound K at or below max_size: everything admissible was enumerated
    assert brute_force(X, y, alpha=alpha, K=3, max_size=4)["closed"]
    assert brute_force(X, y, K=3, max_size=3)["n_supports"] == brute_force(X, y, K=3)["n_supports"]


def test_max_size_one_too_small_is_not_closed():
    """Orthogonal columns of norm sqrt n and y = 2 x_0 - 2 x_1 + 2 x_2: a column's gain is 1/2 * 2^2 = 2, so for alpha = 0.5 the
    optimum is exactly those three.  Two are not enough (-4 + 3 alpha is below the best pair's -4 + 2 alpha + ... nothing the
    reference can rule out: q_all + 3 alpha = -4.5 < -3), three are (q_all + 4 alpha = -4 > -4.5)."""
    Q = np.linalg.qr(np.random.default_rng(0).standard_normal((12, 6)))[0] * np.sqrt(12)
    y = 2 * Q[:, 0] - 2 * Q[:, 1] + 2 * Q[:, 2]
    short = brute_force(Q, y, alpha=0.5, max_size=2)
    assert not short["closed"] and short["active"].sum() == 2 and abs(short["objective"] + 3.0) < 1e-12
    enough = brute_force(Q, y, alpha=0.5, max_size=3)
    assert enough["closed"] and enough["active"].tolist() == [True, True, True, False, False, False]
    assert abs(enough["objective"] + 4.5) < 1e-12
    np.testing.assert_array_equal(enough["active"], brute_force(Q, y, alpha=0.5)["active"])


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_constructor_signatures_equal_the_reference(name):
    from sparselm_amd import model

    cls = getattr(model, name)
    ours = [(k, v.default) for k, v in inspect.signature(cls.__init__).parameters.items() if k != "self"]
    assert ours == SIGNATURES[name]
    assert sorted(cls().get_params()) == sorted(k for k, _ in SIGNATURES[name])
    if not os.path.isdir(REFERENCE_SRC):  # (the reference is not mounted here: the recorded signature above stands)
        return
    found = None
    for fname in ("_best_subset.py", "_regularized_l0.py"):
        with open(os.path.join(REFERENCE_SRC, fname)) as fh:
            tree = ast.parse(fh.read())
        for node in tree.body:
            if isinstance(node, ast.ClassDef) and node.name == name:
                init = next(n for n in node.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
                args = [a.arg for a in init.args.args[1:]]
                defaults = [ast.literal_eval(d) for d in init.args.defaults]
                found = list(zip(args, defaults))
    assert found == ours


def test_names_are_exported_beside_the_lasso_family():
    from sparselm_amd import model

    assert model.MIQP_ESTIMATORS == ("BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L2L0")
    for name in model.MIQP_ESTIMATORS:
        assert name not in model.__all__
        assert inspect.isclass(getattr(model, name))
    assert not hasattr(model, "L1L0")
    from sparselm_amd.model import L2L0  # noqa: F401


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to open an engine fails the test: validation errors have to come first."""
    from sparselm_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were validated")

    monkeypatch.setattr(_engine, "get_engine", boom)


def test_bad_input_raises_before_any_device(no_device):
    # /root/reference/tests/test_miqp.py:226-237, and the hierarchy checks of this package
    from sparselm_amd.model import L2L0, BestSubsetSelection, RegularizedL0, RidgedBestSubsetSelection

    X, y = make_regression(25, 6, n_informative=3, random_state=0)
    with pytest.raises(ValueError):
        BestSubsetSelection(sparse_bound=-1).fit(X, y)
    with pytest.raises(ValueError):
        RidgedBestSubsetSelection(eta=-1.0).fit(X, y)
    with pytest.raises(ValueError):
        L2L0(eta=-1.0).fit(X, y)
    with pytest.raises(ValueError):
        RegularizedL0(alpha=-1.0).fit(X, y)
    with pytest.raises(ValueError):
        RegularizedL0(big_M=-1).fit(X, y)
    with pytest.raises(ValueError):
        RegularizedL0(hierarchy=[[1]] * 5).fit(X, y)  # wrong length
    with pytest.raises(ValueError):
        RegularizedL0(hierarchy=[[9], [], [], [], [], []]).fit(X, y)  # unknown label
    with pytest.raises(ValueError):
        BestSubsetSelection(groups=[0, 0, 1, 1, 2, 2], hierarchy=[[1], [], [5]]).fit(X, y)  # 5 is a column, not a label
    with pytest.raises(ValueError):
        BestSubsetSelection(groups=[0, 0, 1]).fit(X, y)  # wrong length of groups
    with pytest.raises(ValueError):
        L2L0(tikhonov_w=np.eye(5)).fit(X, y)
    with pytest.raises(ValueError):
        BestSubsetSelection(solver_options={"tol": 1e-8}).fit(X, y)


def test_abi_names_the_new_entry():
    from sparselm_amd import _engine

    assert _engine.ABI_VERSION == 24 and "slm_solve_l0" in _engine.ABI_SYMBOLS
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "slm_engine.h")) as fh:
        header = fh.read()
    assert "#define SLM_ABI_VERSION 24" in header and "int slm_solve_l0(" in header
