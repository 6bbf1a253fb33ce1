"""Linear constraints on the exact l0 estimators without a GPU (``add_constraints``, ``slm_solve_l0_constrained``): the public
surface (the header's entry, the ABI's symbol list and version, the binding, the dataset method, the ``constraints``
attribute, ``add_constraints`` and ``clone``); what is refused before any device is touched; the folding of ``Bounds`` into the
per-column box and the route of the multipliers back; the brute-force reference of the GPU tests against closed forms; and
the constrained part of csrc/l0_host.hpp compiled with g++ and run on the CPU, plainly and under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/l0_con_host_test.cpp)."""

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.optimize import Bounds, LinearConstraint
from sklearn.base import clone
from sklearn.datasets import make_regression

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L2L0")


# ---- the public surface -------------------------------------------------------------------------------------------------------
def test_abi_names_the_constrained_entry_and_keeps_its_version():
    from sparselm_amd import _engine

    assert _engine.ABI_VERSION == 24
    with open(os.path.join(ROOT, "include", "slm_engine.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "binding.cpp")) as fh:
        binding = fh.read()
    assert "#define SLM_ABI_VERSION 24" in header
    assert "slm_solve_l0_constrained" in _engine.ABI_SYMBOLS and "int slm_solve_l0_constrained(" in header
    assert hasattr(_engine.Dataset, "solve_l0_constrained")
    assert "slm_solve_l0_constrained(" in binding and 'm.def("solve_l0_constrained"' in binding
    for name in ("slm_solve_l0", "slm_solve_l0_l1", "slm_solve_l0_profile", "slm_solve_l0_wide", "slm_solve_l0_profile_wide"):
        assert name in _engine.ABI_SYMBOLS and f"int {name}(" in header


def test_the_limits_are_the_header_s():
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "l0_host.hpp")) as fh:
        host = fh.read()
    assert "constexpr int L0_CON_MMAX = 64;" in host and "constexpr double L0_CON_TOL = 1e-9;" in host
    assert "constexpr int L0_CON_SWEEPS = 20000;" in host


@pytest.mark.parametrize("name", NAMES)
def test_constraints_survive_clone_and_the_constructor_stays_the_reference_s(name):
    """``constraints`` is an attribute that ``add_constraints`` sets, not a constructor argument (tests/test_l0_cpu.py holds the
    constructors to the reference's): ``get_params`` does not know it, ``clone`` carries it over all the same."""
    from sparselm_amd import model

    cls = getattr(model, name)
    cons = [Bounds(0.0, np.inf), LinearConstraint(np.ones((1, 4)), 0.0, 1.0)]
    est = cls().add_constraints(cons)
    assert cls().constraints is None and clone(cls()).constraints is None
    assert "constraints" not in inspect.signature(cls.__init__).parameters and "constraints" not in est.get_params()
    with pytest.raises(TypeError):
        cls(constraints=cons)
    twin = clone(est)
    assert twin is not est and twin.get_params() == est.get_params()
    assert twin.constraints is not est.constraints and len(twin.constraints) == 2
    assert all(a is b for a, b in zip(twin.constraints, est.constraints))
    # a clone's list is its own: adding to one leaves the other alone; a parameter set on the clone does not drop the list
    twin.add_constraints(Bounds(-1.0, 1.0))
    assert len(est.constraints) == 2 and len(twin.constraints) == 3
    assert len(clone(twin).set_params(big_M=7.0).constraints) == 3


def test_add_constraints_builds_a_new_list():
    from sparselm_amd.model import L2L0

    mine = [Bounds(0.0, np.inf)]
    extra = LinearConstraint(np.ones((1, 4)), 0.0, 1.0)
    est = L2L0().add_constraints(mine)
    assert est.constraints == mine and est.constraints is not mine
    assert est.add_constraints(extra) is est
    assert len(mine) == 1 and len(est.constraints) == 2
    fresh = L2L0().add_constraints([extra])
    assert fresh.constraints == [extra]
    single = L2L0().add_constraints(extra).add_constraints(mine)
    assert single.constraints == [extra, mine[0]]
    assert L2L0.constraints is None  # (nothing was written to the class)


# ---- refusals before any device -----------------------------------------------------------------------------------------------
@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to open an engine fails the test: validation errors have to come first."""
    from sparselm_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were validated")

    monkeypatch.setattr(_engine, "get_engine", boom)


@pytest.mark.parametrize("name", NAMES)
def test_bad_constraints_raise_before_any_device(no_device, name):
    from sparselm_amd import model

    cls = getattr(model, name)
    X, y = make_regression(30, 8, n_informative=3, random_state=0)
    with pytest.raises(ValueError, match="columns"):
        cls().add_constraints(LinearConstraint(np.ones((1, 7)), 0.0, 1.0)).fit(X, y)
    with pytest.raises(ValueError, match="lb > ub"):
        cls().add_constraints(LinearConstraint(np.ones((2, 8)), [0.0, 2.0], [1.0, 1.0])).fit(X, y)
    with pytest.raises(TypeError, match="scipy"):
        cls().add_constraints("beta >= 0").fit(X, y)
    with pytest.raises(ValueError, match="infeasible"):
        cls().add_constraints([Bounds(0.0, np.inf), LinearConstraint(np.ones((1, 8)), -np.inf, -1.0)]).fit(X, y)
    with pytest.raises(ValueError, match="wide"):
        cls(solver_options={"wide": True}).add_constraints(Bounds(0.0, np.inf)).fit(X, y)
    with pytest.raises(ValueError, match="unknown solver_options"):
        cls(solver_options={"qp_sweeps": 5}).add_constraints(Bounds(0.0, np.inf)).fit(X, y)
    # a valid call gets as far as the device, with and without the new option
    with pytest.raises(AssertionError, match="device was touched"):
        cls().add_constraints(Bounds(0.0, np.inf)).fit(X, y)
    with pytest.raises(AssertionError, match="device was touched"):
        cls(solver_options={"max_qp_sweeps": 50}).add_constraints([LinearConstraint(np.ones((1, 8)), 0.0, 1.0)]).fit(X, y)


def test_l1l0_takes_no_constraints(no_device):
    from sparselm_amd.miqp import L1L0

    X, y = make_regression(30, 8, n_informative=3, random_state=0)
    with pytest.raises(ValueError, match="no constraints"):
        L1L0(alpha=1.0, eta=0.1).add_constraints(Bounds(0.0, np.inf)).fit(X, y)
    with pytest.raises(AssertionError, match="device was touched"):
        L1L0(alpha=1.0, eta=0.1).fit(X, y)
    assert "constraints" not in L1L0().get_params()  # its constructor stays the reference's


# ---- folding --------------------------------------------------------------------------------------------------------------------
def test_bounds_fold_into_the_box_and_the_multipliers_find_their_way_back():
    from sparselm_amd.model._miqp import _FoldedConstraints

    p = 5
    lb = np.array([0.0, -np.inf, 0.5, -2.0, -np.inf])
    ub = np.array([np.inf, np.inf, 3.0, -1.0, 4.0])
    row = LinearConstraint(np.arange(10.0).reshape(2, p), [-np.inf, 1.0], [np.inf, 2.0])  # (its first row has no finite side: dropped)
    f = _FoldedConstraints([Bounds(lb, ub), row, Bounds(-1.0, 1.0)], p)
    # intervals that contain 0 narrow the box -- the tighter of the two Bounds objects wins
    assert f.box_lo.tolist() == [0.0, -1.0, -1.0, -1.0, -1.0] and f.box_hi.tolist() == [1.0, 1.0, 1.0, 1.0, 1.0]
    # the other two (0.5 <= b_2 <= 3, -2 <= b_3 <= -1) are rows e_2, e_3; then the LinearConstraint's kept row
    assert f.A.tolist() == [[0, 0, 1, 0, 0], [0, 0, 0, 1, 0], [5, 6, 7, 8, 9]]
    assert f.lo.tolist() == [0.5, -2.0, 1.0] and f.hi.tolist() == [3.0, -1.0, 2.0]
    assert f.cs.m == 4 + 1 + 5  # (entry 1 of the first Bounds has no finite side)
    coef = np.array([0.0, 0.3, 0.5, -1.0, 1.0])
    mu = np.array([-0.7, 0.0, 9.0, 9.0, 0.4])
    got = f.split(np.array([-0.2, 0.6, 0.1]), coef, mu, np.ones(p, dtype=bool))
    assert [g.shape for g in got] == [(5,), (2,), (5,)]
    assert got[0].tolist() == [-0.7, 0.0, -0.2, 0.6, 0.0]  # b_0 at its lb = 0; rows e_2, e_3; b_4 = 1 is not at ub = 4
    assert got[1].tolist() == [0.0, 0.1]
    assert got[2].tolist() == [0.0, 0.0, 0.0, 0.0, 0.4]    # ... it is at the second object's ub = 1
    # a column of an inactive group reports nothing
    assert f.split(np.zeros(3), coef, mu, np.array([False, True, True, True, True]))[0][0] == 0.0
    empty = _FoldedConstraints(Bounds(0.0, np.inf), 3)
    assert empty.A.shape == (0, 3) and empty.box_lo.tolist() == [0.0] * 3 and np.all(np.isinf(empty.box_hi))


# ---- the reference of the GPU tests, against closed forms ---------------------------------------------------------------------------
def test_reference_against_closed_forms():
    from _l0_constrained_reference import best_of, solve_support_con, support_table

    # orthogonal columns of norm sqrt n: H = I, c = X^T y / n; one row a^T b <= h on the support {0, 1}
    n = 12
    Q = np.linalg.qr(np.random.default_rng(0).standard_normal((n, 4)))[0] * np.sqrt(n)
    y = Q @ np.array([1.0, 2.0, -1.0, 0.5])
    A, lo, hi = np.array([[1.0, 1.0, 0.0, 0.0]]), np.array([-np.inf]), np.array([1.0])
    b, val, lam, status = solve_support_con(Q, y, np.array([0, 1]), A, lo, hi)
    assert status == "optimal" and abs(lam[0] - 1.0) <= 1e-12 and np.allclose(b, [0.0, 1.0], atol=1e-12) and abs(val + 1.5) <= 1e-12
    # a support on which the row is zero and excludes 0, and one the box makes infeasible
    assert solve_support_con(Q, y, np.array([2, 3]), A, np.array([0.5]), np.array([np.inf]))[3] == "infeasible"
    assert solve_support_con(Q, y, np.array([0, 1]), A, np.array([3.0]), np.array([np.inf]), big_M=1.0)[3] == "infeasible"
    assert solve_support_con(Q, y, np.zeros(0, dtype=int), A, np.array([0.5]), np.array([np.inf]))[3] == "infeasible"
    # without constraints that bind the table is the plain best subset: gains c_j^2 / 2 = 0.5, 2, 0.5, 0.125
    tab = support_table(Q, y, A, lo, np.array([10.0]))
    assert len(tab) == 16
    ref = best_of(tab, 4, K=2)
    assert ref["support"] in ((0, 1), (1, 2)) and abs(ref["objective"] + 2.5) <= 1e-12 and ref["gap"] <= 1e-12  # a tie
    ref = best_of(tab, 4, alpha=0.3)
    assert ref["support"] == (0, 1, 2) and abs(ref["objective"] - (-3.0 + 0.9)) <= 1e-12 and abs(ref["gap"] - 0.175) <= 1e-12
    assert best_of(tab, 4, K=1, hierarchy=[[], [3], [], []])["support"] in ((0,), (2,))


# ---- the host side, on the CPU ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_l0_con_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l0_con_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "l0_con_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "l0_con_host_test: ok" in run.stdout
