"""The case table of the on-chip solver's shape tests (tests/_on_chip_cases.py), kept honest without a GPU: the shapes sit
on the edges of `small_solve_kernel` and `PathCall::run_on_chip` as long as the constants of csrc/small_kernels.hpp,
csrc/engine_internal.hpp and csrc/engine_path.hip are the ones the table was derived for -- a changed constant fails here
rather than leaving shapes that pass while meaning nothing -- and every compared case has a converged, fast and (where
coefficients are compared) unique reference."""

import numpy as np
import pytest

import _on_chip_cases as oc


def test_the_constants_are_the_ones_the_table_was_derived_for():
    c = oc.CONSTANTS
    assert c["SM_PMAX"] == 128 and c["SM_THREADS"] == 256 and c["SM_LDS_BYTES"] == 156 * 1024
    assert c["ONE_WAVE_MAX"] == 32 and c["WIDE_ABOVE"] == 64 and c["GRAM_MAXB"] == 3
    assert c["kSmallOutDoubles"] == 32768 and c["kSnapInfos"] == 64 and c["CHIP_DOUBLES"] == 131072
    assert max(oc.WIDTHS) == c["SM_PMAX"] and max(oc.ROW_WIDTHS) == c["SM_PMAX"]


def test_widths_sit_on_the_edges_of_the_product():
    lay = {p: oc.layout(p) for p in oc.WIDTHS}
    # one wavefront, no helpers, up to 32; a second position per lane beyond 64
    assert [p for p in oc.WIDTHS if lay[p]["one_wave"]] == [1, 2, 31, 32]
    assert [p for p in oc.WIDTHS if lay[p]["wide"]] == [65, 87, 88, 95, 96, 97, 123, 124, 127, 128]
    assert not lay[33]["one_wave"] and not lay[64]["wide"] and not lay[63]["wide"]
    # helper wavefronts: a single row for helper 2 and none for helper 3 at 33
    assert lay[33]["ranges"] == [(0, 16), (16, 32), (32, 33), (33, 33)]
    # the last helper with rows has a range that is no multiple of eight at 65, 87 and 97 (the remainder loop of sm_partial)
    last = {p: [hi - lo for lo, hi in lay[p]["ranges"] if hi > lo][-1] for p in (65, 87, 97, 96, 128)}
    assert last[65] == 17 and last[87] == 15 and last[97] == 1
    assert lay[65]["ranges"][3] == (65, 65)
    # ... and 96 and 128 divide evenly
    assert [hi - lo for lo, hi in lay[96]["ranges"]] == [24] * 4 and [hi - lo for lo, hi in lay[128]["ranges"]] == [32] * 4
    for p in oc.WIDTHS:  # the four ranges tile 0..p
        r = lay[p]["ranges"]
        assert r[0][0] == 0 and r[-1][1] == p and all(r[i][1] == r[i + 1][0] for i in range(3))


def test_widths_sit_on_the_edges_of_the_gram_build():
    lay = {p: oc.layout(p) for p in oc.WIDTHS}
    assert [lay[p]["nblocks"] for p in (87, 88, 123, 124, 128)] == [253, 276, 496, 528, 561]
    assert [lay[p]["nb"] for p in (87, 88, 123, 124, 127, 128)] == [22, 23, 31, 32, 32, 33]
    # a second block per thread starts at 88, a third at 124; three is what the kernel's registers hold
    assert [lay[p]["blocks_per_thread"] for p in (87, 88, 123, 124, 128)] == [1, 2, 2, 3, 3]
    assert max(v["blocks_per_thread"] for v in lay.values()) == oc.CONSTANTS["GRAM_MAXB"]
    # the y column (position p): alone in the last block row at 128, in the last slot of its block row at 127
    assert 128 % 4 == 0 and 128 // 4 == lay[128]["nb"] - 1
    assert 127 % 4 == 3 and 127 // 4 == lay[127]["nb"] - 1


# the table of the issue: p -> (ld, rows per chunk, largest n)
CHUNKS = {16: (16, 982, 8192), 32: (32, 523, 4096), 33: (48, 521, 2730), 64: (64, 230, 2048), 65: (80, 228, 1638),
          87: (96, 137, 1365), 88: (96, 129, 1365), 96: (96, 104, 1365), 97: (112, 102, 1170), 123: (128, 35, 1024),
          124: (128, 32, 1024), 127: (128, 26, 1024), 128: (128, 24, 1024)}


def test_row_counts_sit_on_the_chunk_edges_and_on_the_bound():
    for p, (ld, rpc, n_max) in CHUNKS.items():
        lay = oc.layout(p)
        assert (lay["ld"], lay["rows_per_chunk"], lay["n_max"]) == (ld, rpc, n_max), p
    bound = oc.CONSTANTS["CHIP_DOUBLES"]
    for p in oc.ROW_WIDTHS:
        lay = oc.layout(p)
        counts, beyond = oc.row_counts(p)
        rpc = lay["rows_per_chunk"]
        assert counts == (1, 2, 3, rpc - 1, rpc, rpc + 1, 2 * rpc + 3, lay["n_max"])
        assert all(n * lay["ld"] <= bound for n in counts) and beyond * lay["ld"] > bound and (beyond - 1) * lay["ld"] <= bound
        assert (2 * rpc + 3) % rpc == 3 and lay["n_max"] > 2 * rpc  # several chunks, a short last one
        built = {c["X"].shape[0] for c in oc.cases("rows", p)}
        assert built == set(counts) | {beyond}
        assert {c["expect"] for c in oc.cases("rows", p) if c["X"].shape[0] == beyond} == {"general"}
    # 131072 doubles exactly where ld divides it
    assert [oc.layout(p)["n_max"] * oc.layout(p)["ld"] for p in (16, 64, 128)] == [bound] * 3
    # part (c): one row beyond a chunk at 33, chunks and a short last one at 97 and 128; the last two are shapes of part (b)
    shapes = oc.weight_shapes()
    assert shapes == ((33, 522), (97, 207), (128, 1024))
    for p, n in shapes:
        assert n > p and n % oc.layout(p)["rows_per_chunk"] != 0 and n > oc.layout(p)["rows_per_chunk"]
    assert 207 in oc.row_counts(97)[0] and 1024 in oc.row_counts(128)[0]


def test_the_face_cap_at_full_width():
    assert oc.layout(128)["face_cap"] == 65
    assert all(oc.layout(p)["face_cap"] >= p for p in oc.WIDTHS if p <= 111) and oc.layout(112)["face_cap"] < 112
    assert all(oc.layout(p)["face_cap"] >= p for p in oc.FACE_WIDTHS)
    assert sorted(p % 4 for p in oc.FACE_WIDTHS) == [0, 1, 2, 3]


def test_the_result_routes():
    c = oc.CONSTANTS
    (n, p) = oc.ROUTE_SHAPE
    assert p == c["SM_PMAX"] and n * oc.layout(p)["ld"] <= c["CHIP_DOUBLES"]
    X, y, groups, calls = oc.route_calls()
    assert X.shape == (n, p)
    pts = {name: oc.total_points(lanes) for name, (lanes, _) in calls.items()}
    staged = {name: pts[name] * p <= c["kSmallOutDoubles"] and not gn for name, (_, gn) in calls.items()}
    in_snapshot = {name: pts[name] <= c["kSnapInfos"] for name in calls}
    assert staged == {"snapshot+staged": True, "fetched+staged": True, "fetched+copied": False, "group-norms": False}
    assert in_snapshot == {"snapshot+staged": True, "fetched+staged": False, "fetched+copied": False, "group-norms": False}
    assert pts["fetched+copied"] * p == 64 * 5 * 128 == 40960 and len(calls["fetched+copied"][0]) == 64
    assert len(calls["group-norms"][0]) == 16 and calls["group-norms"][1]
    for name, (lanes, _) in calls.items():
        assert len({len(lane["points"]) for lane in lanes}) > 1, name  # different path lengths
        assert len({lane["points"][0] for lane in lanes}) == len(lanes), name  # different alphas


def _check_references(case):
    p = case["X"].shape[1]
    refs = oc.reference(case)
    assert sum(r["seconds"] for r in refs) < 1.0, (case["tag"], [r["seconds"] for r in refs])
    for lane, ref in zip(case["lanes"], refs):
        assert ref["converged"], case["tag"]
        if lane["compare"] == "coef":
            assert ref["unique"], case["tag"]  # (or the case would have to be compared by objective only)
        for k in range(len(lane["points"])):
            kkt, gmax = oc.certificate(case, lane, k, ref["betas"][k])
            assert kkt < 1e-8 * gmax, (case["tag"], k, kkt, gmax)  # the bound asked of the kernel is one the reference meets
        assert ref["betas"].shape == (len(lane["points"]), p)


@pytest.mark.parametrize("part", ["width", "rows", "weights", "faces"])
def test_every_compared_case_has_a_converged_unique_and_quick_reference(part):
    if part == "width":
        todo = [c for p in oc.WIDTHS for c in oc.cases("width", p)]
    elif part == "rows":
        todo = [c for p in oc.ROW_WIDTHS for c in oc.cases("rows", p)]
    elif part == "weights":
        todo = [c for p, n in oc.weight_shapes() for c in oc.cases("weights", p, n)]
    else:
        todo = list(oc.cases("faces"))
    for case in todo:
        _check_references(case)
    if part == "rows":  # which are compared how
        for case in todo:
            n, p = case["X"].shape
            assert case["lanes"][0]["compare"] == ("coef" if n >= 2 * p else "objective")
    if part == "weights":  # the third lane's mask leaves fewer rows than columns, and so fewer than a full face
        for case in todo:
            n, p = case["X"].shape
            few, general = case["lanes"][2], case["lanes"][1]
            assert n > p and 0 < few["n_eff"] < p and few["compare"] == "objective"
            w = general["row_weight"]
            assert np.sum(w == 0.0) == n // 7 and np.all(w < 2.0) and np.all(w >= 0.0) and general["n_eff"] is None
            fold = case["lanes"][0]
            assert fold["n_eff"] == int(fold["row_weight"].sum()) > p


def test_the_faces_are_as_large_as_the_issue_asks():
    """The direct solves: the oracle's support is the whole width at 40..43 (a face size per residue mod 4) and above the
    factor's 65 unknowns at 128."""
    for case in oc.cases("faces"):
        p = case["X"].shape[1]
        support = int(np.count_nonzero(oc.reference(case)[0]["betas"][0]))
        if p == 128:
            assert support > oc.layout(128)["face_cap"] == 65, support
        else:
            assert support == p, (case["tag"], support)


def test_the_route_lanes_checked_against_the_oracle_have_quick_references():
    X, y, groups, calls = oc.route_calls()
    for name, (lanes, _) in calls.items():
        for i in (0, len(lanes) // 2, len(lanes) - 1):
            case = dict(tag=f"route-{name}-{i}", X=X, y=y, groups=groups, lanes=[lanes[i]], expect="chip")
            _check_references(case)
