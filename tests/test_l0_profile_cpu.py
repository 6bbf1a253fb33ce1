"""``l0_profile`` without a GPU: the per-size brute-force table the GPU tests compare against (tests/_l0_profile_reference.py)
checked against the brute force of tests/_l0_reference.py; the public surface (import path, the header's entry, the ABI's
symbol list, the binding); parameter validation before any device is touched; ``L0Profile``'s own arithmetic on hand-made
tables; and the profile part of csrc/l0_host.hpp compiled with g++ and run on the CPU, plainly and under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/l0_profile_host_test.cpp)."""

import os
import shutil
import subprocess

import numpy as np
import pytest
from sklearn.datasets import make_regression

from _l0_profile_reference import best_subset_of, envelope_sizes, profile_table, regularized_of
from _l0_reference import brute_force

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# ---- the reference ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True])
def test_reference_table_meets_the_brute_force(grouped):
    X, y = make_regression(40, 16 if grouped else 8, n_informative=4, noise=30.0, random_state=0)
    groups = np.repeat(np.arange(8), 2) if grouped else None
    hierarchy = [[] for _ in range(8)]
    hierarchy[2], hierarchy[5] = [6], [2]
    for kw in (dict(), dict(eta=0.3), dict(big_M=20.0), dict(hierarchy=hierarchy)):
        table = profile_table(X, y, groups=groups, **kw)
        assert table["values"][0] == 0.0 and not table["actives"][0].any() and (table["actives"].sum(axis=1) == np.arange(9)).all()
        for K in (0, 1, 3, 6, 8):  # the prefix-min is best subset at the bound K
            ref = brute_force(X, y, groups=groups, K=K, **kw)
            k = best_subset_of(table, K)
            assert ref["objective"] == table["values"][k] and np.array_equal(ref["active"], table["actives"][k])
            assert ref["coef"].tobytes() == table["coefs"][k].tobytes()
        for rel in (1e-4, 0.05, 0.6):  # values[k] + alpha k is the regularised problem
            alpha = rel * float(np.var(y))
            ref = brute_force(X, y, groups=groups, alpha=alpha, **kw)
            k = regularized_of(table, alpha)
            assert np.array_equal(ref["active"], table["actives"][k]) and ref["coef"].tobytes() == table["coefs"][k].tobytes()
            assert abs(ref["objective"] - (table["values"][k] + alpha * k)) <= 1e-15 * abs(ref["objective"])
        # the runner-up of a size is the best of that size once the winner is taken away
        assert (table["seconds"] >= table["values"]).all() and np.isinf(table["seconds"][0]) and np.isinf(table["gaps"][0])
    n_all = profile_table(X, y, groups=groups)["n_supports"]
    assert n_all == 2**8 and profile_table(X, y, groups=groups, hierarchy=hierarchy)["n_supports"] < n_all


def test_reference_premises_of_the_gpu_tests():
    """What tests/test_l0_profile_gpu.py relies on, on the reference's numbers: at 40 x 12 with noise 30 every size has a
    best-to-second gap of at least 3e-5 and the values fall strictly (seed 0; the GPU file asserts the same for its own runs)."""
    X, y = make_regression(40, 12, n_informative=5, noise=30.0, random_state=0)
    X, y = X - X.mean(axis=0), y - y.mean()
    table = profile_table(X, y)
    assert (table["gaps"][1:12] >= 3e-5).all() and (np.diff(table["values"]) < 0).all() and (table["kappas"] <= 1e4).all()


def test_envelope_sizes_on_hand_made_tables():
    assert envelope_sizes([0.0, -3.0, -5.0, -6.0, -6.5]) == [0, 1, 2, 3, 4]           # concave gains: every size
    assert envelope_sizes([0.0, -1.0, -5.0, -5.5, -9.0]) == [0, 2, 4]                 # sizes 1 and 3 lie above their chords
    assert envelope_sizes([0.0, -4.0, -4.0, -3.0]) == [0, 1]                          # nothing beyond the minimum
    assert envelope_sizes([0.0, np.inf, -6.0, np.inf, -7.0]) == [0, 2, 4]
    assert envelope_sizes([0.0, -2.0, -4.0]) == [0, 2]                                # on the chord: a tie, never the unique optimum


# ---- L0Profile's arithmetic -----------------------------------------------------------------------------------------------------
def hand_made(values, alpha_min=0.0):
    from sparselm_amd.miqp import L0Profile

    values = np.asarray(values, dtype=float)
    K = len(values) - 1
    supports = np.tril(np.ones((K + 1, K), dtype=bool), -1) & np.isfinite(values)[:, None]
    coefs = np.where(supports, np.arange(1, K + 2)[:, None] * 1.0, 0.0)
    return L0Profile(values, supports, coefs, np.arange(K + 1) * 0.5, alpha_min,
                     {"nodes": 0, "launches": 1, "q_all": float(np.min(values)), "status": "optimal", "proven_optimal": True, "box_tol": 1e-12})


def test_profile_object_answers_from_the_table():
    prof = hand_made([0.0, -1.0, -5.0, -5.5, -9.0])
    for bound in range(5):
        coef, intercept, active = prof.best_subset(bound)
        assert active.sum() == bound and intercept == 0.5 * bound and (coef[:bound] == bound + 1).all() and not coef[bound:].any()
    assert prof.best_subset(2.9)[2].sum() == 2  # (the estimators floor a fractional bound)
    alphas, sizes = prof.alpha_breakpoints()
    assert sizes.tolist() == [0, 2, 4] and np.allclose(alphas, [2.5, 2.0]) and sizes.tolist() == envelope_sizes(prof.values_)
    for lo, hi, size in ((2.5, 4.0, 0), (2.0, 2.5, 2), (0.0, 2.0, 4)):
        assert prof.regularized(0.5 * (lo + hi))[2].sum() == size
    assert prof.regularized(2.5)[2].sum() == 0 and prof.regularized(2.0)[2].sum() == 2  # ties go to the smaller size
    # what is returned is a copy: the table cannot be changed through it
    prof.best_subset(4)[0][:] = 0.0
    assert prof.coefs_[4].all()
    with pytest.raises(ValueError):
        prof.best_subset(5)
    with pytest.raises(ValueError):
        prof.best_subset(-1)
    with pytest.raises(ValueError):
        prof.regularized(-1e-3)
    with pytest.raises(ValueError):
        prof.regularized(np.nan)
    # unfilled sizes are never answers
    holes = hand_made([0.0, np.inf, -6.0, np.inf, -7.0])
    assert holes.best_subset(1)[2].sum() == 0 and holes.best_subset(3)[2].sum() == 2 and holes.regularized(0.25)[2].sum() == 4
    assert holes.alpha_breakpoints()[1].tolist() == [0, 2, 4]
    # a table pruned for alpha >= alpha_min serves those alphas only
    pruned = hand_made([0.0, -1.0, -5.0, -5.5, -9.0], alpha_min=2.2)
    with pytest.raises(ValueError, match="alpha_min"):
        pruned.best_subset(2)
    with pytest.raises(ValueError, match="alpha_min"):
        pruned.regularized(2.1)
    assert pruned.regularized(2.2)[2].sum() == 2
    alphas, sizes = pruned.alpha_breakpoints()
    assert sizes.tolist() == [0, 2] and np.allclose(alphas, [2.5])  # the breakpoint at 2.0 is below alpha_min


# ---- the public surface -------------------------------------------------------------------------------------------------------
def test_miqp_exports_the_profile_and_model_does_not():
    import sparselm_amd.miqp as miqp
    from sparselm_amd import model
    from sparselm_amd.model import _l0_profile, _miqp

    assert miqp.l0_profile is _l0_profile.l0_profile and miqp.L0Profile is _l0_profile.L0Profile
    assert _l0_profile.__all__ == ["l0_profile", "L0Profile"]
    for name in ("l0_profile", "L0Profile"):
        assert not hasattr(model, name) and name not in model.__all__ and name not in _miqp.__all__ and name not in model.MIQP_ESTIMATORS
    # the estimators and the profile share their preparation: one code path, not a copy
    assert _l0_profile._ProfileProblem._l0_setup is _miqp._ExactL0._l0_setup
    assert _l0_profile._ProfileProblem._l0_dataset is _miqp._ExactL0._l0_dataset


def test_abi_names_the_new_entry_and_keeps_its_version():
    from sparselm_amd import _engine

    assert _engine.ABI_VERSION == 24 and "slm_solve_l0_profile" in _engine.ABI_SYMBOLS
    with open(os.path.join(ROOT, "include", "slm_engine.h")) as fh:
        header = fh.read()
    assert "#define SLM_ABI_VERSION 24" in header and "int slm_solve_l0_profile(" in header and "int slm_solve_l0(" in header
    assert hasattr(_engine.Dataset, "solve_l0_profile")
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "binding.cpp")) as fh:
        binding = fh.read()
    assert "slm_solve_l0_profile(" in binding and 'm.def("solve_l0_profile"' in binding


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to open an engine fails the test: validation errors have to come first."""
    from sparselm_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were validated")

    monkeypatch.setattr(_engine, "get_engine", boom)


def test_bad_input_raises_before_any_device(no_device):
    from sparselm_amd.miqp import l0_profile

    X, y = make_regression(25, 6, n_informative=3, random_state=0)
    for bad in (dict(alpha_min=-1.0), dict(alpha_min=np.inf), dict(alpha_min="low"), dict(eta=-1.0), dict(eta=np.inf), dict(big_M=-1),
                dict(max_groups=-1), dict(max_groups=7), dict(max_groups=2.5), dict(hierarchy=[[1]] * 5),
                dict(hierarchy=[[9], [], [], [], [], []]), dict(groups=[0, 0, 1]), dict(solver_options={"tol": 1e-8}),
                dict(fit_intercept="yes"), dict(tikhonov_w=np.eye(5)), dict(sample_weight=np.ones(24))):
        with pytest.raises(ValueError):
            l0_profile(X, y, **bad)
    with pytest.raises(ValueError):
        l0_profile(X, y[:-1])
    with pytest.raises(TypeError):
        l0_profile(X, y, 3)  # (everything after y is keyword-only)
    # ... and good input gets as far as the device
    with pytest.raises(AssertionError, match="device was touched"):
        l0_profile(X, y, max_groups=3, groups=[0, 0, 1, 1, 2, 2])


# ---- the host side, on the CPU ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_l0_profile_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l0_profile_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "l0_profile_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "l0_profile_host_test: ok" in run.stdout
