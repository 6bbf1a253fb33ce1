"""The l0 local search with an l1 term without a GPU: the public surface, every refusal before a device, the numpy restatement
(tests/_l1l0_local_reference.py) against the penalised restatement at lam = 0 and against a brute force over all supports with a
lasso on each, the certificate, the premises of every GPU case (tests/_l1l0_local_cases.py), and the host twin, its check and its
polish under AddressSanitizer and UndefinedBehaviorSanitizer (tests/l1l0_local_host_test.cpp, a stand-alone program)."""

import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest
from sklearn.datasets import make_regression

import _l0_local_reference as plain
from _l0_local_reference import gram, hard_law
from _l1l0_local_cases import MARGIN_MIN, cases, premise, reference
from _l1l0_local_reference import brute_force, is_l1_swap_inescapable, local_search, objective, polish

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
ENTRY = "slm_solve_l0_local_l1"


@pytest.fixture()
def no_device(monkeypatch):
    """Any attempt to open an engine fails the test: validation errors have to come first."""
    from sparselm_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a device was touched before the arguments were validated")

    monkeypatch.setattr(_engine, "get_engine", boom)


# ---- the public surface -------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_under_abi_24():
    from sparselm_amd import _engine

    assert _engine.ABI_VERSION == 24
    with open(os.path.join(ROOT, "include", "slm_engine.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "binding.cpp")) as fh:
        binding = fh.read()
    assert "#define SLM_ABI_VERSION 24" in header
    assert ENTRY in _engine.ABI_SYMBOLS and f"int {ENTRY}(" in header
    assert f"{ENTRY}(" in binding and f'm.def("{ENTRY[4:]}"' in binding
    decl = header[header.index(f"int {ENTRY}("):]
    decl = " ".join(decl[: decl.index(";")].split())
    args = ("slm_dataset* ds", "int32_t count", "const double* const* row_weights", "const int64_t* n_effs", "int32_t intercept",
            "int32_t n_cells", "const double* alphas", "const double* l1s", "const double* ridges", "double big_M", "int32_t n_starts",
            "const double* starts", "int32_t swaps", "double* beta_out", "double* intercept_out", "double* objective_out", "int32_t* start_out",
            "int32_t* stat_out", "slm_point_info* info")
    at = [decl.index(arg) for arg in args]
    assert at == sorted(at)  # every argument, in this order
    assert "ridges /* [n_cells] or NULL: 0 */" in decl and "4 words per problem" in decl
    comment = header[: header.index(f"int {ENTRY}(")]
    comment = comment[comment.rindex("/*"):]
    for words in ("NOTHING IS PROVEN", "sign(u) max(|u| - lam, 0)", "mode = 10", "never raises F", "Refusals"):
        assert words in comment, words
    assert hasattr(_engine.Dataset, "solve_l0_local_l1")
    # the ctypes signature: the dataset, twelve arguments, five outputs, the records
    assert len(_engine.load_library().slm_solve_l0_local_l1.argtypes) == 19
    # the entries that were there are still there
    for name in ("slm_solve_l0_local", "slm_solve_l0_local_descent", "slm_solve_l0_local_folds", "slm_solve_l0_local_subsets",
                 "slm_solve_l0_local_groups", "slm_solve_l0_l1"):
        assert name in _engine.ABI_SYMBOLS and f"int {name}(" in header
    assert header.count("slm_solve_l0_local_l1") >= 5  # the four older entries point at it


def test_export_lists_and_signatures():
    import sparselm_amd.miqp as miqp
    from sparselm_amd.model import _l0_local, _l0_local_cv, _l0_local_groups, _l0_local_subsets, _l1l0_local, _l1l0_local_cv

    assert _l1l0_local.__all__ == ["l1l0_local_search", "L1L0LocalPath"]
    assert _l1l0_local_cv.__all__ == ["l1l0_local_cv", "L1L0LocalCV"]
    for name, mod in (("l1l0_local_search", _l1l0_local), ("L1L0LocalPath", _l1l0_local), ("l1l0_local_cv", _l1l0_local_cv),
                      ("L1L0LocalCV", _l1l0_local_cv)):
        assert getattr(miqp, name) is getattr(mod, name) and name not in miqp.__all__
    assert miqp.__all__ == ["BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L1L0", "L2L0"]
    assert _l0_local.__all__ == ["l0_local_search", "L0LocalPath"] and _l0_local_cv.__all__ == ["l0_local_cv", "L0LocalCV"]
    assert _l0_local_subsets.__all__ == ["l0_local_subsets", "L0LocalSubsets"]
    assert _l0_local_groups.__all__ == ["l0_local_group_search", "L0LocalGroupPath"]
    assert miqp.L1L0LocalPath.proven_optimal_ is False and miqp.L1L0LocalCV.proven_optimal_ is False
    params = inspect.signature(miqp.l1l0_local_search).parameters
    assert list(params) == ["X", "y", "alphas", "etas", "ridge", "big_M", "fit_intercept", "sample_weight", "starts", "max_rounds",
                            "solver_options"]
    assert all(v.kind is inspect.Parameter.KEYWORD_ONLY for k, v in params.items() if k not in ("X", "y"))
    assert params["alphas"].default is inspect.Parameter.empty and params["etas"].default is inspect.Parameter.empty
    assert [params[k].default for k in list(params)[4:]] == [0.0, 100, False, None, None, 2, None]
    params = inspect.signature(miqp.l1l0_local_cv).parameters
    assert list(params) == ["X", "y", "alphas", "etas", "ridge", "cv", "big_M", "fit_intercept", "sample_weight", "starts", "max_rounds",
                            "scoring", "solver_options"]
    assert [params[k].default for k in list(params)[4:]] == [0.0, 5, 100, False, None, None, 2, "neg_root_mean_squared_error", None]
    for doc in (_l1l0_local.__doc__, _l1l0_local_cv.__doc__):
        assert "NOTHING IS PROVEN" in doc
    assert "l1l0_local_search" in _l0_local.__doc__ and "l1l0_local_cv" in _l0_local_cv.__doc__


def test_the_result_carries_every_table():
    from sparselm_amd.miqp import L1L0LocalPath

    z = np.zeros((2, 1))
    coefs = np.array([[[0.0, 2.0, 0.0]], [[1.0, 2.0, 0.0]]])
    res = L1L0LocalPath([0.1, 0.2], [0.05], coefs, [[0.5], [0.25]], z, z, 1, z[None], z, z, np.ones((2, 1), bool), ridge=0.01)
    for name in ("alphas_", "etas_", "ridge_", "coefs_", "intercepts_", "supports_", "objectives_", "losses_", "rounds_", "round_objectives_",
                 "swaps_", "sweeps_", "converged_"):
        assert hasattr(res, name), name
    assert res.ridge_ == 0.01 and res.supports_.sum() == 3 and res.proven_optimal_ is False
    np.testing.assert_array_equal(res.predict(np.eye(3), 1), [1.25, 2.25, 0.25])


def test_one_kernel_body_three_kernels_and_the_docs():
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "l0_local_kernels.hpp")) as fh:
        kernels = fh.read()
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "l0_local_body.inc")) as fh:
        body = fh.read()
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "l0_host.hpp")) as fh:
        host = fh.read()
    assert kernels.count('#include "l0_local_body.inc"') == 2 and "struct L0LsL1Args : L0LsArgs" in kernels
    assert "static_assert(!(CARD && L1)" in body and "static_assert(!(CARD && L1)" in host
    assert body.count("l0_ls_coord_of<L1>(") == 3  # the descent, g_i and g_j of the swap scan
    for text in (kernels, body):
        assert "asm" not in text and "atomicAdd" not in text and "__shared__" not in text and "__syncthreads" not in text
    assert "constexpr L0LsCoord l0_ls_coord_l1(double u, double d, double big_M, double lam)" in host
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "engine_l0.hip")) as fh:
        unit = fh.read()
    assert f'extern "C" int {ENTRY}(' in unit and "L0_LOCAL_L1" in unit
    body = unit[unit.index("int solve_l0_local_folds_impl("):]
    assert body.index("l0_l1l_check(") < body.index("hipSetDevice")  # the refusals come before a device
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        design = fh.read()
    assert "**Local search with an l1 term**" in design and "profiles/l1l0_local.txt" in design
    for title in ("**Local search**", "**Local search over folds**", "**Local subsets**"):
        para = design[design.index(title):]
        para = para[para.index("*Not built:*"):]
        para = para[: para.index("\n\n")].split("  (")[0]  # (the list itself: the pointers behind it name the new section)
        assert "l1 term" not in para.replace("the l1 term in this cardinality form", ""), title
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert "l1l0_local_search" in fh.read()
    assert os.path.exists(os.path.join(ROOT, "profiles", "l1l0_local.txt")) and os.path.exists(os.path.join(ROOT, "tools", "l1l0_local_timing.py"))


# ---- refusals, all before a device ------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_any_device(no_device):
    from sparselm_amd.miqp import l1l0_local_cv, l1l0_local_search

    X, y = make_regression(25, 6, n_informative=3, random_state=0)
    ok = dict(alphas=[0.1], etas=[0.05])
    for bad in (dict(alphas=[-1.0]), dict(alphas=[np.nan]), dict(alphas=[np.inf]), dict(alphas=[]), dict(alphas=[[0.1]]),
                dict(etas=[-1.0]), dict(etas=[np.inf]), dict(etas=[np.nan]), dict(etas=[]), dict(ridge=-1.0), dict(ridge=np.nan),
                dict(ridge=[0.0, 0.1]), dict(ridge=None), dict(big_M=-1), dict(max_rounds=-1), dict(max_rounds=1.5),
                dict(solver_options={"max_nodes": 5}), dict(solver_options={"swaps": 1}), dict(solver_options=[("swaps", True)]),
                dict(fit_intercept="yes"), dict(sample_weight=np.ones(24)), dict(starts=np.zeros((2, 5))),
                dict(alphas=[0.1, 0.2], starts=np.zeros((1, 1, 2, 6))), dict(big_M=1.0, starts=np.full((1, 6), 1.5)),
                dict(starts=np.full((1, 6), np.nan)),
                dict(alphas=np.full(5000, 0.1), etas=[0.0, 0.1]),                       # 10 000 cells x 4 starts of a round
                dict(alphas=np.full(5000, 0.1), starts=np.zeros((1, 6)), max_rounds=0)):  # 5 000 cells x 2 starts
        with pytest.raises(ValueError):
            l1l0_local_search(X, y, **{**ok, **bad})
        with pytest.raises(ValueError):
            l1l0_local_cv(X, y, cv=3, **{**ok, **bad})
    for bad in (dict(cv=16), dict(cv=1), dict(scoring="r2")):
        with pytest.raises(ValueError):
            l1l0_local_cv(X, y, **ok, **bad)
    with pytest.raises(ValueError):
        l1l0_local_search(X, y[:-1], **ok)
    with pytest.raises(TypeError):
        l1l0_local_search(X, y, alphas=[0.1])  # etas has no default: it is the l1 weight, not l0_local_search's ridge
    with pytest.raises(TypeError):
        l1l0_local_search(X, y, [0.1], [0.05])
    with pytest.raises(TypeError):
        l1l0_local_search(X, y, groups=[0, 0, 1, 1, 2, 2], **ok)  # no groups with the l1 term
    with pytest.raises(NotImplementedError, match="1024"):
        l1l0_local_search(np.zeros((3, 1025)), np.zeros(3), **ok)


def test_the_engine_names_every_refusal_itself():
    """The C entry refuses each of these before it touches a device, each in its own words (the order and the codes are checked
    by tests/l1l0_local_host_test.cpp on ``l0_l1l_check``; both routes by the GPU tests)."""
    with open(os.path.join(ROOT, "sparse-lm_amd", "csrc", "engine_l0.hip")) as fh:
        unit = fh.read()
    body = unit[unit.index("int solve_l0_local_folds_impl("):]
    body = body[body.index("const L0LocalGroups* lg, const double* l1s) {"):]
    body = body[: body.index("hipSetDevice")]
    for words in ("l1s[%lld] must be finite and >= 0", "ridges[%lld] must be finite and >= 0", "alphas[%lld] must be finite and >= 0",
                  "takes up to %d columns", "not built for groups", "not built for row-sharded datasets", "big_M must be >= 0",
                  "n_cells must be >= 1", "n_starts must be >= 1", "must be at most %d problems", "lies outside the box", "count must be 1 .. %d",
                  "row_weights[%d][%lld] must be finite and >= 0", "the last column must be alone in the last group"):
        assert words in body, words


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_lam_zero_is_the_penalised_restatement(seed):
    X, y = hard_law(seed)
    G, c, yy, _, _ = gram(X, y)
    start = np.zeros(14)
    start[[0, 5, 9]] = [0.5, -0.25, 1.0]
    for rel in (0.3, 0.1, 0.03):
        alpha = rel * float(np.var(y))
        for st in (None, start):
            for swaps in (True, False):
                a = plain.local_search(G, c, alpha, 100.0, yy, start=st, swaps=swaps)
                b = local_search(G, c, alpha, 0.0, 100.0, yy, start=st, swaps=swaps)
                np.testing.assert_array_equal(a["beta"], b["beta"])
                assert (a["swaps"], a["sweeps"], a["status"], a["changes"]) == (b["swaps"], b["sweeps"], b["status"], b["changes"])
                assert a["F"] == b["F"]


HITS = {"full": 0, "descent": 0, "cases": 0, "swapped": 0, "margin": np.inf}


@pytest.mark.parametrize("seed", range(12))
def test_never_below_brute_force_on_the_hard_law(seed):
    """hard_law(seed, n=30, p=10, k=3), alpha in {0.2, 0.05, 0.01} var y, lam in {0.02, 0.1}: never below the optimum, swaps never
    worse than the descent alone, every accepted swap lowered F, the certificate holds.  The hit count is printed, not asserted
    (over the twelve seeds: the full rule 48 of 72, the descent alone 23, 35 cases took swaps, the smallest margin 1.1e-4)."""
    X, y = hard_law(seed, n=30, p=10, k=3)
    G, c, yy, _, _ = gram(X, y)
    for rel in (0.2, 0.05, 0.01):
        for lam in (0.02, 0.1):
            alpha = rel * float(np.var(y))
            exact, _ = brute_force(G, c, alpha, lam, 100.0)
            tol = 1e-9 * max(abs(exact), alpha)
            runs = {}
            for swaps in (False, True):
                run = local_search(G, c, alpha, lam, 100.0, yy, swaps=swaps)
                beta = polish(G, c, lam, 100.0, run["beta"])
                F = objective(G, c, alpha, lam, beta)
                assert run["status"] == 0 and run["lowered"] and F <= run["F"] + tol
                assert abs(run["F"] - objective(G, c, alpha, lam, run["beta"])) <= tol
                assert F >= exact - tol  # never below the optimum
                ok, why = is_l1_swap_inescapable(G, c, alpha, lam, 100.0, beta, 1e-8, swaps=swaps)
                assert ok, why
                runs[swaps] = F
            assert runs[True] <= runs[False] + tol  # swaps start from the descent's fixed point
            HITS["cases"] += 1
            HITS["full"] += abs(runs[True] - exact) <= tol
            HITS["descent"] += abs(runs[False] - exact) <= tol
            HITS["swapped"] += run["swaps"] > 0
            HITS["margin"] = min(HITS["margin"], run["margin"])
    print(f"so far: the full rule at the optimum in {HITS['full']} of {HITS['cases']}, the descent alone in {HITS['descent']}, "
          f"{HITS['swapped']} took swaps, smallest margin {HITS['margin']:.2e}")


def test_certificate_rejects_what_is_not_a_minimum():
    X, y = hard_law(5, n=30, p=10, k=3)
    G, c, yy, _, _ = gram(X, y)
    alpha, lam = 0.05 * float(np.var(y)), 0.02
    descent = polish(G, c, lam, 100.0, local_search(G, c, alpha, lam, 100.0, yy, swaps=False)["beta"])
    full = polish(G, c, lam, 100.0, local_search(G, c, alpha, lam, 100.0, yy)["beta"])
    assert is_l1_swap_inescapable(G, c, alpha, lam, 100.0, descent, 1e-8, swaps=False)[0]
    assert not is_l1_swap_inescapable(G, c, alpha, lam, 100.0, descent, 1e-8, swaps=True)[0]  # (a swap helps at this seed)
    assert is_l1_swap_inescapable(G, c, alpha, lam, 100.0, full, 1e-8, swaps=True)[0]
    off = full.copy()
    off[np.flatnonzero(off)[0]] *= 1.01
    assert not is_l1_swap_inescapable(G, c, alpha, lam, 100.0, off, 1e-8, swaps=False)[0]
    assert not is_l1_swap_inescapable(G, c, alpha, lam, 100.0, np.zeros(10), 1e-8, swaps=False)[0]  # some column's gain is above alpha
    # the least-squares fit on the support is not the lasso's point: the l1 term moves every coefficient
    S = np.flatnonzero(full)
    ls = np.zeros(10)
    ls[S] = np.linalg.solve(G[np.ix_(S, S)], c[S])
    assert not is_l1_swap_inescapable(G, c, alpha, lam, 100.0, ls, 1e-8, swaps=False)[0]
    assert not is_l1_swap_inescapable(G, c, alpha, lam, 0.5 * np.abs(full).max(), full, 1e-8)[0]  # outside a smaller box


@pytest.mark.parametrize("name", sorted(cases()))
def test_the_premises_of_every_gpu_case(name):
    ok, text = premise(name)
    print(name, text)
    assert ok, text
    assert all(cell["margin"] >= MARGIN_MIN and cell["status"] == 0 for cell in reference(name))


def test_the_gpu_cases_are_the_shapes_the_kernel_can_go_wrong_at():
    ref = {name: reference(name) for name in cases()}
    assert sum(cell["swaps"] for cell in ref["slots130"]) >= 1  # one cell at p = 130 swaps
    for name in ("p1024_zero", "p1024_wrong_start"):
        live = np.flatnonzero(ref[name][0]["beta"])
        assert set(live // 64) == set(range(16))  # all sixteen slots are live
    assert int(np.sum(np.abs(ref["box"][0]["beta"]) == 0.6)) == 4  # four coefficients on the bound
    assert not any(cell["beta"].any() for cell in ref["lam_above_max_c"])
    assert ref["second_start"][0]["start"] == 1 and ref["second_start_reversed"][0]["start"] == 0
    assert any(cell["swaps"] >= 1 for cell in ref["hard_law_swaps"]) and any(cell["swaps"] == 2 for cell in ref["hard_law_two_swaps"])
    assert not any(cell["swaps"] for cell in ref["hard_law_descent"])
    k = cases()["rows_below_columns"]
    assert k["X"].shape[0] < k["X"].shape[1] and not k["ridges"].any()


# ---- the host twin, on the CPU ------------------------------------------------------------------------------------------------
def export_cases(path):
    """Small cases of the restatement for the stand-alone program: every start of every cell of the cases with p <= 130."""
    count = 0
    with open(path, "w") as fh:
        for name in sorted(cases()):
            k = cases()[name]
            p = k["X"].shape[1]
            if p > 130:
                continue
            for e, cell in enumerate(reference(name)):
                starts = [None] if k["starts"] is None else list(k["starts"][e])
                for s, start in enumerate(starts):
                    run = local_search(cell["H"], cell["c"], k["alphas"][e], k["l1s"][e], k["big_M"], cell["yy"], start=start, swaps=k["swaps"])
                    assert run["status"] == 0 and run["margin"] >= MARGIN_MIN
                    G = cell["H"] - 2.0 * k["ridges"][e] * np.eye(p)
                    head = [float(v) for v in (k["alphas"][e], k["l1s"][e], k["ridges"][e], k["big_M"], cell["yy"])]
                    fh.write(f"{p} {p + 3} " + " ".join(repr(v) for v in head) + f" {int(k['swaps'])} {int(start is not None)} {run['swaps']} "
                             f"{run['sweeps']} {float(run['F'])!r}\n")
                    for row in G:
                        fh.write(" ".join(repr(float(v)) for v in row) + "\n")
                    fh.write(" ".join(repr(float(v)) for v in cell["c"]) + "\n")
                    if start is not None:
                        fh.write(" ".join(repr(float(v)) for v in start) + "\n")
                    fh.write(" ".join(str(int(v != 0.0)) for v in run["beta"]) + "\n")
                    count += 1
    return count


@pytest.mark.parametrize("sanitize", [False, True])
def test_l1l0_local_host(tmp_path, sanitize):
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "l1l0_local_host_test"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"] if sanitize else []
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                            os.path.join(ROOT, "tests", "l1l0_local_host_test.cpp"), "-o", str(exe)], capture_output=True, text=True)
    if sanitize and build.returncode != 0 and "sanitize" in build.stderr.lower():
        pytest.skip("this toolchain has no sanitizer runtime")
    assert build.returncode == 0, build.stderr
    exported = export_cases(tmp_path / "cases.txt")
    assert exported >= 30
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "l1l0_local_host_test: ok" in run.stdout and f"exported: {exported} cases" in run.stdout
