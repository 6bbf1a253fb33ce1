"""The on-chip solver (`small_solve_kernel`, csrc/small_kernels.hpp; `PathCall::run_on_chip`, csrc/engine_path.hip) against
the oracle at every shape where it changes path -- the case table of tests/_on_chip_cases.py, whose shapes
tests/test_on_chip_shapes_cpu.py ties to the constants of the sources.

The reference throughout is `oracle.fista` at tol 1e-14 on the rows and weights the lane sees; every accepted point is also
certified from numpy's own X^T (w (X b - y)) / n_eff.  The on-chip calls run at tol 1e-12 and the bounds are those of
test_on_chip_gpu.py::test_reference_sized_fits_match_the_oracle: coefficients within 1e-9 max|ref| where the minimiser is
unique, objective <= f(ref) (1 + 1e-12) + 1e-14 everywhere, KKT residual < 1e-8 max|g|, the reported `kkt` within
1e-8 max(1, max|g|) of numpy's, group norms to rtol 1e-12.

A point the kernel does not settle sends the whole call to the general path, which would hide a kernel that stopped
converging at one width: parts (a)-(c) therefore assert `mode == 2` on every point (and `mode != 2` for the first row count
beyond the chip's bound).  Part (d), the direct solves on a face, asserts correctness whichever route answered and prints
the mode."""

import numpy as np
import pytest

import _on_chip_cases as oc
from sparselm_amd import _engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return _engine.get_engine(0)


def _specs(lanes):
    return [dict(points=lane["points"], a=lane.get("a"), row_weight=lane["row_weight"], n_eff=lane["n_eff"]) for lane in lanes]


def _solve(ds, lanes, want_group_norms=True):
    """One on-chip call for the lanes; the results copied out of the call's blocks."""
    res = ds.solve_lanes(_specs(lanes), tol=oc.CHIP_TOL, flags=_engine.FLAG_ON_CHIP, want_group_norms=want_group_norms)
    return [dict(betas=r.betas.copy(), group_norms=None if r.group_norms is None else r.group_norms.copy(), n_iter=r.n_iter,
                 kkt=r.kkt, mode=r.mode, converged=r.converged, grad_launches=r.grad_launches) for r in res]


def _check_lane(case, lane, got, ref):
    """The bounds of the module's docstring for every point of one lane."""
    p = case["X"].shape[1]
    assert got["converged"], case["tag"]
    for k in range(len(lane["points"])):
        beta, want = got["betas"][k], ref["betas"][k]
        where = (case["tag"], k)
        f_got, f_ref = oc.lane_objective(case, lane, k, beta), oc.lane_objective(case, lane, k, want)
        kkt, gmax = oc.certificate(case, lane, k, beta)
        err = float(np.max(np.abs(beta - want)))
        print(f"{case['tag']} point {k}: mode {got['mode'][k]} n_iter {got['n_iter'][k]} coef err {err:.2e} of {np.max(np.abs(want)):.2e} "
              f"f - f_ref {f_got - f_ref:.2e} kkt {kkt:.2e} reported {got['kkt'][k]:.2e} max|g| {gmax:.2e}")
        assert f_got <= f_ref * (1 + 1e-12) + 1e-14, where
        if lane["compare"] == "coef":
            assert ref["unique"], where
            np.testing.assert_allclose(beta, want, rtol=0, atol=1e-9 * np.max(np.abs(want)), err_msg=str(where))
        assert kkt < 1e-8 * gmax, where
        assert abs(got["kkt"][k] - kkt) <= 1e-8 * max(1.0, gmax), where
        if got["group_norms"] is not None:
            _, _, _, gidx, G = oc.lane_penalties(case, lane, k)
            np.testing.assert_allclose(got["group_norms"][k], np.sqrt(np.bincount(gidx, weights=beta**2, minlength=G)), rtol=1e-12,
                                       atol=1e-15, err_msg=str(where))
    assert got["betas"].shape == (len(lane["points"]), p)


def _run_case(eng, case):
    refs = oc.reference(case)
    with eng.dataset(case["X"], case["y"]) as ds:
        if case["groups"] is not None:
            ds.set_groups(case["groups"], int(case["groups"].max()) + 1)
        got = _solve(ds, case["lanes"])
    for lane, g, ref in zip(case["lanes"], got, refs):
        _check_lane(case, lane, g, ref)
        if case["expect"] == "chip":
            assert np.all(g["mode"] == 2) and g["grad_launches"] == 1, (case["tag"], g["mode"], g["grad_launches"])
        elif case["expect"] == "general":
            assert np.all(g["mode"] != 2), (case["tag"], g["mode"])
    return got


@pytest.mark.parametrize("p", oc.WIDTHS)
def test_every_width_where_the_product_or_the_gram_build_changes_path(eng, p):
    """(a) n = 2 p + 7, two-point warm paths of a lasso at 0.3 alpha_max, a group penalty on permuted groups of five and a
    sparse-group penalty with a ridge: one and four wavefronts in the product (32 / 33), one and two positions per lane
    (64 / 65), helper ranges with a remainder (65, 87, 97) and without (96, 128), one, two and three blocks per thread in the
    Gram build (87 / 88, 123 / 124), the y column at the end of a block row (127) and alone in one (128), p = 1 and 2.  Every
    point is settled on chip, in one launch."""
    for case in oc.cases("width", p):
        _run_case(eng, case)


def _row_shapes():
    return [(p, n) for p in oc.ROW_WIDTHS for n in oc.row_counts(p)[0] + (oc.row_counts(p)[1],)]


@pytest.mark.parametrize("p,n", _row_shapes())
def test_every_row_count_where_the_gram_build_changes_path(eng, p, n):
    """(b) n = 1, 2, 3 (fewer rows than staging wavefronts), one chunk of the stage less a row, exactly, plus a row, two
    chunks and three rows, n * ld = 131072 (the chip's last shape) and the first n beyond it (the general path: mode != 2);
    lasso and sparse-group.  n < 2 p: objective and certificate; n >= 2 p: coefficients as well.  Every row count the chip
    takes asserts `mode == 2` under both penalties.  (One input was replaced under a stated limit of the kernel: at 1 x 128 the
    sparse-group point at (0.1 alpha_max, 0.15 group alpha_max) spends its 320 products and eight Newton steps on groups
    sliding to zero and goes to the general path; n = 1, 2, 3 run that penalty at twice the strength -- `row_cases`.)"""
    todo = [case for case in oc.cases("rows", p) if case["X"].shape[0] == n]
    assert len(todo) == 2
    for case in todo:
        _run_case(eng, case)


@pytest.mark.parametrize("p,n", oc.weight_shapes())
def test_row_weights_at_the_chunk_edges(eng, p, n):
    """(c) three lanes of one call: a fold mask with its n_eff, general weights in (0, 2) with a seventh of them zero, and a
    mask that leaves fewer rows than columns (a face larger than the rows that carry weight must be survived: the kernel's
    `face_now <= n` counts all rows) -- the weights enter as sqrt(w) where the rows are staged, over a chunk edge."""
    for case in oc.cases("weights", p, n):
        _run_case(eng, case)


def test_faces_of_every_residue_mod_four_and_beyond_the_factor(eng):
    """(d) AR(1) columns (rho = 0.95) with the whole width in the support: faces of 40, 41, 42 and 43 unknowns for the direct
    solve's blocks of four columns, 128 unknowns where the factor holds 65, a group penalty at 42.  Right whichever route
    answered; the modes are printed."""
    for case in oc.cases("faces"):
        got = _run_case(eng, case)
        print(f"FACE {case['tag']}: mode {got[0]['mode'].tolist()} n_iter {got[0]['n_iter'].tolist()}")


@pytest.fixture(scope="module")
def route_data(eng):
    X, y, groups, calls = oc.route_calls()
    with eng.dataset(X, y) as ds:
        ds.set_groups(groups, int(groups.max()) + 1)
        yield ds, X, y, groups, calls


@pytest.mark.parametrize("name", ["snapshot+staged", "fetched+staged", "fetched+copied", "group-norms"])
def test_results_travel_back_lane_by_lane_on_every_route(route_data, name):
    """(e) run_on_chip hands results back on four routes -- coefficients staged in pinned memory (total points * p <= 32768,
    no group norms) or by copy commands, records in the snapshot (<= 64 points) or fetched -- and a wrong lane offset on any of
    them moves another lane's vector: lanes of different lengths, alphas and l1 weights; each lane of the call equals, bit
    for bit, the same lane in a call of its own (betas, n_iter, kkt, group norms); the first, a middle and the last lane
    against the oracle."""
    ds, X, y, groups, calls = route_data
    lanes, want_gn = calls[name]
    together = _solve(ds, lanes, want_group_norms=want_gn)
    assert len(together) == len(lanes)
    for i, (lane, got) in enumerate(zip(lanes, together)):
        assert np.all(got["mode"] == 2) and got["grad_launches"] == 1, (name, i, got["mode"])
        alone = _solve(ds, [lane], want_group_norms=want_gn)[0]
        assert np.all(alone["mode"] == 2), (name, i)
        assert np.array_equal(got["betas"], alone["betas"]), (name, i)
        assert np.array_equal(got["n_iter"], alone["n_iter"]) and np.array_equal(got["kkt"], alone["kkt"]), (name, i)
        if want_gn:
            assert np.array_equal(got["group_norms"], alone["group_norms"]), (name, i)
        else:
            assert got["group_norms"] is None
    for i in (0, len(lanes) // 2, len(lanes) - 1):
        case = dict(tag=f"route-{name}-{i}", X=X, y=y, groups=groups, lanes=[lanes[i]], expect="chip")
        _check_lane(case, lanes[i], together[i], oc.reference(case)[0])
