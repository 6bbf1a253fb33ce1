"""The exact l0 search BELOW its ticket prefix (``l0_search_kernel``, csrc/l0_kernels.hpp) against the brute force of
tests/_l0_reference.py.

The first ``min(groups, 16)`` groups of the search order are decided by a wavefront's ticket; tests/test_l0_gpu.py stays at
12 groups and so never runs the depth-first search proper: coming back from an include, turning it into an exclude,
climbing, the state restored from lane g, the bound on the descent, the hierarchy across the boundary, dependent columns
met below it, and a register-resident factor of more than a dozen rows.  The problems here are DESIGNED so that the optimum
needs groups whose search rank is 16 or more (hidden suppressor pairs ``u + eps v``, ``u - eps v`` with ``y ~ v``: each
column alone says little about y, the two together explain it; decoys ``z + tau y / std y`` score higher and fill the
prefix), and every test asserts that premise on the reference -- ``search_rank`` restates the documented order from X --
next to the premises of test_l0_gpu.py (gap >= 1e-6, kappa <= 1e4) before it compares anything.  The comparison and its
tolerances are that file's own (``compare``, ``compare_singular``).

Every reference enumerates at most 60,000 supports (asserted); penalised problems are closed by the reference's own bound
(``brute_force(max_size=)`` -> ``closed``, asserted).  Every engine call must come back proven optimal under the default
budget."""

import functools
import types
from math import comb

import numpy as np
import pytest

from _l0_reference import brute_force, objective_of, search_rank
from test_l0_gpu import COEF_RTOL, GAP_MIN, KAPPA_MAX, OBJ_RTOL, assert_parents_active, compare, compare_singular

pytestmark = pytest.mark.gpu

PREFIX = 16  # L0_PREFIX: groups decided by the ticket
MAX_SUPPORTS = 60000


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---- the design -------------------------------------------------------------------------------------------------------------
def decoy(rng, y, tau, width=1):
    """``Z + tau y / std y`` with Z Gaussian and made orthogonal to y: its marginal score is then tau^2 var y / (1 + tau^2)
    whatever the draw, so decoys outrank the hidden columns by construction and not by luck."""
    Z = rng.standard_normal((len(y), width))
    Z -= np.outer(y, y @ Z) / float(y @ y)
    return Z + tau * (y / np.std(y))[:, None]


@functools.lru_cache(maxsize=None)
def suppressor(ng, n=60, pairs=2, width=1, eps=0.15, tau=0.25, amps=(1.0, 0.8, 0.6), noise=0.05, scale=1.0, dependent=0.0, carrier=0.0, proxy=0.0,
               seed=0):
    """``2 * pairs`` hidden groups of ``width`` columns, ``U_h + eps V_h`` and ``U_h - eps V_h``, and decoy groups
    ``Z_j + tau y / std y`` up to ``ng`` groups; ``y = sum_h amps[h] V_h 1 + noise``.  The hidden directions are orthonormal
    (columns of norm sqrt n), so that a hidden column's marginal score is eps^2 amps^2 / (1 + eps^2) up to the noise.
    ``dependent = gamma > 0`` adds two directions a, b with ``y += 0.8 (a - b)``, the two-column group P = {a, b} and the
    one-column group D = {a + b + gamma (a - b)}: D depends on P, P scores 0.64 and D about 1.28 gamma^2.  ``carrier = b > 0``
    adds a Gaussian group C with ``y += b C 1 / sqrt width``: signal of its own that no other group carries.  ``proxy = e > 0``
    adds the column ``y + e r`` (r orthogonal to y, norm sqrt n): alone it is within e^2 / 2 of the value of all columns.
    Groups and columns are shuffled; X is multiplied by ``scale``.  Returns (X, y, groups or None, hidden: the labels of the pair groups,
    the labels of the two groups after the pairs -- (P, D), or (C or the proxy, the first decoy) -- or None)."""
    rng = np.random.default_rng(seed)
    k = 2 * pairs * width
    B = np.linalg.qr(rng.standard_normal((n, k + 2)))[0] * np.sqrt(n)
    U, V, ab = B[:, : pairs * width], B[:, pairs * width:k], B[:, k:]
    y = noise * rng.standard_normal(n)
    for h in range(pairs):
        y = y + amps[h] * V[:, h * width:(h + 1) * width].sum(axis=1)
    blocks = []
    for h in range(pairs):
        sl = slice(h * width, (h + 1) * width)
        blocks += [U[:, sl] + eps * V[:, sl], U[:, sl] - eps * V[:, sl]]
    if dependent:
        a, b = ab.T
        y = y + 0.8 * (a - b)
        blocks += [np.column_stack([a, b]), (a + b + dependent * (a - b))[:, None]]
    if carrier:
        C = rng.standard_normal((n, width))
        y = y + carrier * C.sum(axis=1) / np.sqrt(width)
        blocks.append(C)
    if proxy:
        r = rng.standard_normal(n)
        r -= y * (y @ r) / float(y @ y)
        blocks.append((y + proxy * r * np.sqrt(n) / np.linalg.norm(r))[:, None])
    while len(blocks) < ng:
        blocks.append(decoy(rng, y, tau, width))
    label = rng.permutation(ng)  # block g of the list above becomes the group of label label[g]
    groups = np.concatenate([np.full(blk.shape[1], label[g]) for g, blk in enumerate(blocks)])
    order = rng.permutation(len(groups))
    X, groups = scale * np.column_stack(blocks)[:, order], groups[order]
    if len(groups) == ng:  # single columns: column j is group j
        X, groups = X[:, np.argsort(groups)], None
    hidden = np.sort(label[: 2 * pairs])
    frozen(X, y, hidden)
    return X, y, groups, hidden, (int(label[2 * pairs]), int(label[2 * pairs + 1])) if dependent or carrier or proxy else None


@functools.lru_cache(maxsize=None)
def suppressor_ref(ng, K, big_M=np.inf, **design):
    X, y, groups, _, _ = suppressor(ng, **design)
    return brute_force(X, y, groups=groups, K=K, big_M=big_M)


def winner_ranks(ref, rank):
    return np.sort(rank[np.flatnonzero(ref["active"])])


def assert_below_prefix(ref, rank, ng, at_least=2):
    """The rank premise: the winner needs groups that only the depth-first search can reach."""
    ranks = winner_ranks(ref, rank)
    print(f"supports {ref['n_supports']}, winner's search ranks {ranks.tolist()}")
    assert ref["n_supports"] <= MAX_SUPPORTS
    if ng >= PREFIX + 2:
        assert np.count_nonzero(ranks >= PREFIX) >= at_least
    elif ng == PREFIX + 1:
        assert PREFIX in ranks
    else:
        assert (ranks < PREFIX).all()  # the control: everything sits in the prefix


# ---- 1. the prefix boundary, cardinality-bounded ---------------------------------------------------------------------------
BOUNDED = {  # (ng, K): the design's arguments
    (16, 4): {}, (17, 4): {}, (18, 5): dict(noise=0.2),  # (more noise: the fifth column's gain is then no near-tie between decoys)
    (20, 4): {}, (24, 4): {},
    (32, 3): dict(pairs=1, tau=0.3), (48, 3): dict(pairs=1, tau=0.3, n=80), (64, 2): dict(pairs=1, tau=0.3, n=100),
}


@pytest.mark.parametrize("ng,K", sorted(BOUNDED))
def test_prefix_boundary_bounded(ng, K):
    from sparselm_amd.model import BestSubsetSelection

    X, y, _, hidden, _ = suppressor(ng, **BOUNDED[ng, K])
    ref = suppressor_ref(ng, K, **BOUNDED[ng, K])
    assert set(hidden) <= set(np.flatnonzero(ref["active"]))  # the pairs together explain y
    assert_below_prefix(ref, search_rank(X, y), ng)
    est = BestSubsetSelection(sparse_bound=K, big_M=1000).fit(X, y)
    compare(est, ref, X, y)


# ---- 2. the prefix boundary, penalised -------------------------------------------------------------------------------------
REL_ALPHA = 0.05  # alpha = REL_ALPHA * ||y||^2 / (2n): far above what a decoy gains, far below what a pair column gains
# X times 5: the hidden columns' coefficients are amps / (2 eps scale), and at scale 1 the ridge term eta ||beta||^2 with the
# issue's eta = 0.1 would cost more than the pairs gain (the optimum would then sit in the prefix)
PENALISED = dict(scale=5.0)


@functools.lru_cache(maxsize=None)
def penalised_ref(ng, eta, K=None):
    X, y, _, _, _ = suppressor(ng, **PENALISED)
    alpha = REL_ALPHA * float(y @ y) / (2 * len(y))
    return alpha, brute_force(X, y, alpha=alpha, eta=eta, K=K, max_size=None if K is not None else 5 if ng <= 18 else 4)


@pytest.mark.parametrize("ng", [18, 20, 24])
@pytest.mark.parametrize("name", ["RegularizedL0", "L2L0"])
def test_prefix_boundary_penalised(name, ng):
    from sparselm_amd import model

    X, y, _, _, _ = suppressor(ng, **PENALISED)
    eta = 0.1 if name == "L2L0" else 0.0
    alpha, ref = penalised_ref(ng, eta)
    assert ref["closed"] and 0 < ref["active"].sum() < ng
    assert_below_prefix(ref, search_rank(X, y, eta=eta), ng)
    est = getattr(model, name)(alpha=alpha, big_M=1000, **({"eta": eta} if eta else {})).fit(X, y)
    compare(est, ref, X, y, alpha=alpha, eta=eta)


PROXY = dict(proxy=0.5)


@functools.lru_cache(maxsize=None)
def proxy_problem():
    """20 columns: the four hidden ones, a proxy ``y + e r`` and 15 decoys.  The proxy alone is the greedy seed, with the value
    q_z + alpha; the four hidden columns together reach q_4 ~ q_all.  alpha = 0.29 (q_z - q_all) puts the seed between
    q_all + 4 alpha and q_all + 5 alpha: the bound ``q_all + alpha (|S| + 1) >= incumbent`` must still let a node with three
    groups take its fourth, and a bound one level too eager would cut exactly the optimum."""
    X, y, _, hidden, (z, _) = suppressor(20, **PROXY)
    n = len(y)
    q_all = float(np.sum((X @ np.linalg.lstsq(X, y, rcond=None)[0] - y) ** 2) - y @ y) / (2 * n)
    q_z = brute_force(X[:, [z]], y, K=1)["objective"]
    alpha = 0.29 * (q_z - q_all)
    return X, y, hidden, z, q_all, q_z, alpha, brute_force(X, y, alpha=alpha, max_size=4)


def test_bound_lets_the_last_level_through():
    from sparselm_amd.model import RegularizedL0

    X, y, hidden, z, q_all, q_z, alpha, ref = proxy_problem()
    rank = search_rank(X, y)
    assert ref["closed"] and set(np.flatnonzero(ref["active"])) == set(hidden) and rank[z] == 0
    assert q_all + 4 * alpha < q_z + alpha <= q_all + 5 * alpha  # the seed sits inside the last level's margin
    assert_below_prefix(ref, rank, 20, at_least=4)
    est = RegularizedL0(alpha=alpha, big_M=1000).fit(X, y)
    compare(est, ref, X, y, alpha=alpha)
    assert est.solver_info_["seed_objective"] <= q_z + alpha + 1e-9 * abs(q_z) and est.solver_info_["objective"] < est.solver_info_["seed_objective"]


def test_penalty_and_bound_together():
    """alpha and K both active, through the dataset call: K below the size of the penalised winner."""
    from sparselm_amd import _engine

    ng, K = 20, 3
    X, y, _, _, _ = suppressor(ng, **PENALISED)
    alpha, unbounded = penalised_ref(ng, 0.0)
    assert unbounded["closed"] and unbounded["active"].sum() > K  # the bound binds
    _, ref = penalised_ref(ng, 0.0, K=K)
    unpenalised = brute_force(X, y, K=K)
    assert ref["closed"] and 0 < ref["active"].sum() < unpenalised["active"].sum() == K  # ... and so does the penalty
    assert_below_prefix(ref, search_rank(X, y), ng)
    with _engine.get_engine().dataset(X, y) as ds:
        beta, support, info = ds.solve_l0(alpha=alpha, max_groups=K, big_M=1000.0)
    est = types.SimpleNamespace(coef_=beta, solver_info_=info, active_groups_=np.array([(support >> i) & 1 for i in range(ng)], dtype=bool))
    compare(est, ref, X, y, alpha=alpha)


# ---- 3. hierarchy across the boundary --------------------------------------------------------------------------------------
HIER = dict(ng=20, K=5, design=dict(pairs=3))  # three pairs: the weakest one stays out of the free optimum and ranks last


@functools.lru_cache(maxsize=None)
def hierarchy_ref(need):
    X, y, _, _, _ = suppressor(HIER["ng"], **HIER["design"])
    return brute_force(X, y, K=HIER["K"], big_M=1000, hierarchy=[list(v) for v in need] if need is not None else None)


@pytest.mark.parametrize("case", ["prefix_needs_deep", "deep_needs_excluded_prefix", "later_and_earlier", "chain_of_three"])
def test_hierarchy_across_the_boundary(case):
    from sparselm_amd.model import BestSubsetSelection

    ng, K = HIER["ng"], HIER["K"]
    X, y, _, _, _ = suppressor(ng, **HIER["design"])
    rank = search_rank(X, y)
    at = np.argsort(rank)  # at[r]: the column of search rank r
    free = hierarchy_ref(None)
    won = set(np.flatnonzero(free["active"]))
    need = [[] for _ in range(ng)]
    if case == "prefix_needs_deep":  # a prefix group of the free optimum needs a deep group that is not in it
        src = next(j for j in at[:PREFIX] if j in won)
        dst = next(j for j in at[PREFIX:] if j not in won)
        need[src] = [dst]
    elif case == "deep_needs_excluded_prefix":  # a deep group of the free optimum needs a prefix group that is not in it
        src = next(j for j in at[PREFIX:] if j in won)
        dst = next(j for j in at[:PREFIX] if j not in won)
        need[src] = [dst]
    elif case == "later_and_earlier":  # rank 17 needs rank 19 (met later), rank 19 needs rank 16 (met earlier)
        need[at[17]] = [at[19]]
        need[at[19]] = [at[16]]
        assert at[17] in won and at[19] not in won
    else:  # rank 16 needs rank 18, rank 18 needs rank 19: all three below the prefix
        need[at[16]] = [at[18]]
        need[at[18]] = [at[19]]
        assert at[16] in won and not {at[18], at[19]} <= won
    ref = hierarchy_ref(tuple(tuple(int(v) for v in row) for row in need))
    assert not np.array_equal(ref["active"], free["active"])  # the hierarchy changed the answer
    assert ref["n_supports"] <= MAX_SUPPORTS and free["n_supports"] <= MAX_SUPPORTS
    print(f"free optimum's search ranks {winner_ranks(free, rank).tolist()}, with the hierarchy {winner_ranks(ref, rank).tolist()}")
    assert np.count_nonzero(winner_ranks(ref, rank) >= PREFIX) >= 1
    est = BestSubsetSelection(sparse_bound=K, hierarchy=need, big_M=1000).fit(X, y)
    compare(est, ref, X, y)
    assert_parents_active(est.active_groups_, need, list(range(ng)))


# ---- 4. many rows of the factor ----------------------------------------------------------------------------------------------
WIDE = dict(n=160, pairs=1, width=16, carrier=2.0)


def four_by_sixteen():
    """Four groups of 16 columns, n = 160: a hidden pair of groups, a group with signal of its own, and a decoy.  The decoy
    has the best marginal score and the greedy seed starts with it, so the 32- and 48-column optima are the search's to find."""
    X, y, groups, hidden, (carrier, decoy_label) = suppressor(4, **WIDE)
    return X, y, groups, hidden, carrier, decoy_label


@pytest.mark.parametrize("K", [2, 4])
def test_sixteen_column_groups_bounded(K):
    from sparselm_amd.model import BestSubsetSelection

    X, y, groups, hidden, _, _ = four_by_sixteen()
    ref = brute_force(X, y, groups=groups, K=K, big_M=1000)
    columns = int(np.isin(groups, np.flatnonzero(ref["active"])).sum())
    print(f"supports {ref['n_supports']}, columns held by the winner {columns}")
    assert columns == 16 * K and set(hidden) <= set(np.flatnonzero(ref["active"]))  # (K = 4: the whole 64-column factor)
    est = BestSubsetSelection(groups=groups, sparse_bound=K, big_M=1000).fit(X, y)
    compare(est, ref, X, y)
    print(f"objective {est.solver_info_['objective']:.6e}, seed {est.solver_info_['seed_objective']:.6e}")
    assert est.solver_info_["objective"] <= est.solver_info_["seed_objective"]
    assert np.count_nonzero(est.coef_) == columns


def test_sixteen_column_groups_penalised():
    from sparselm_amd.model import RegularizedL0

    X, y, groups, hidden, carrier, decoy_label = four_by_sixteen()
    # alpha between what the decoy still gains beside the other three and what the carrier gains beside the pair: 48 columns win
    full, three = brute_force(X, y, groups=groups, K=4), brute_force(X, y, groups=groups, K=3)
    two = brute_force(X, y, groups=groups, K=2)
    alpha = 0.5 * ((three["objective"] - full["objective"]) + (two["objective"] - three["objective"]))
    ref = brute_force(X, y, groups=groups, alpha=alpha, big_M=1000)
    columns = int(np.isin(groups, np.flatnonzero(ref["active"])).sum())
    print(f"alpha {alpha:.4e}, supports {ref['n_supports']}, columns held by the winner {columns}")
    assert columns == 48 and not ref["active"][decoy_label] and ref["active"][carrier]
    est = RegularizedL0(groups=groups, alpha=alpha, big_M=1000).fit(X, y)
    compare(est, ref, X, y, alpha=alpha)
    print(f"objective {est.solver_info_['objective']:.6e}, seed {est.solver_info_['seed_objective']:.6e}")
    assert est.solver_info_["objective"] <= est.solver_info_["seed_objective"]


@functools.lru_cache(maxsize=None)
def twenty_and_singletons(both=False):
    """Two groups of 20 columns and 22 single columns (p = 62, 24 groups), n = 160: the first wide group carries signal
    (``both``: the second one too, and more of it, so that the two precede the pair in the search order and the pair's
    columns become rows 40 and 41 of the factor), two of the single columns are a hidden suppressor pair, the other twenty
    are decoys."""
    rng = np.random.default_rng(22)
    n = 160
    wide = rng.standard_normal((n, 40))
    uv = np.linalg.qr(rng.standard_normal((n, 2)))[0] * np.sqrt(n)
    y = wide[:, :20] @ (rng.uniform(0.1, 0.2, 20) * rng.choice([-1.0, 1.0], 20)) + 1.0 * uv[:, 1] + 0.05 * rng.standard_normal(n)
    if both:
        wide -= uv @ (uv.T @ wide) / n  # (orthogonal to the hidden directions: the pair's scores stay eps^2, below the wide groups')
        y = y + wide @ (rng.uniform(0.3, 0.45, 40) * rng.choice([-1.0, 1.0], 40))
    singles = [uv[:, 0] + 0.15 * uv[:, 1], uv[:, 0] - 0.15 * uv[:, 1]]
    singles += [decoy(rng, y, 0.3)[:, 0] for _ in range(20)]
    lab = rng.permutation(24)  # labels: lab[0], lab[1] the wide groups, lab[2], lab[3] the pair
    X = np.empty((n, 62))
    groups = np.empty(62, dtype=int)
    order = rng.permutation(62)
    blocks = [(lab[0], wide[:, :20]), (lab[1], wide[:, 20:])] + [(lab[2 + i], s[:, None]) for i, s in enumerate(singles)]
    at = 0
    for label, blk in blocks:
        for k in range(blk.shape[1]):
            X[:, order[at]] = blk[:, k]
            groups[order[at]] = label
            at += 1
    frozen(X, y, groups)
    return (X, y, groups, int(lab[0]), (int(lab[2]), int(lab[3]))) + ((int(lab[1]),) if both else ())


@functools.lru_cache(maxsize=None)
def twenty_and_singletons_ref(big_M=np.inf):
    X, y, groups, _, _ = twenty_and_singletons()
    return brute_force(X, y, groups=groups, K=3, big_M=big_M)


def test_twenty_column_group_with_deep_singletons():
    from sparselm_amd.model import BestSubsetSelection

    X, y, groups, wide, pair = twenty_and_singletons()
    ref = twenty_and_singletons_ref()
    rank = search_rank(X, y, groups=groups)
    assert ref["active"][wide] and any(ref["active"][g] and rank[g] >= PREFIX for g in pair)
    assert_below_prefix(ref, rank, 24, at_least=1)
    print(f"columns held by the winner {int(np.isin(groups, np.flatnonzero(ref['active'])).sum())}")
    est = BestSubsetSelection(groups=groups, sparse_bound=3, big_M=1000).fit(X, y)
    compare(est, ref, X, y)


def test_two_twenty_column_groups_and_the_pair():
    """K = 4: both wide groups and the hidden pair, 42 columns.  The pair's second column is appended as row 41 of a factor
    whose row 40 is its partner: only a forward substitution that is right at rows 40 and beyond sees what the two gain
    together."""
    from sparselm_amd.model import BestSubsetSelection

    X, y, groups, wide, pair, wide2 = twenty_and_singletons(both=True)
    ref = brute_force(X, y, groups=groups, K=4, big_M=1000)
    rank = search_rank(X, y, groups=groups)
    print(f"ranks: wide groups {rank[wide]}, {rank[wide2]}, pair {[int(rank[g]) for g in pair]}")
    assert set(np.flatnonzero(ref["active"])) == {wide, wide2, *pair}
    assert max(rank[wide], rank[wide2]) < min(rank[g] for g in pair) and min(rank[g] for g in pair) >= PREFIX
    assert_below_prefix(ref, rank, 24)
    est = BestSubsetSelection(groups=groups, sparse_bound=4, big_M=1000).fit(X, y)
    compare(est, ref, X, y)
    assert np.count_nonzero(est.coef_) == 42


THREES = dict(ng=21, K=4, design=dict(width=3, n=160, tau=0.3))


def test_twenty_one_groups_of_three():
    from sparselm_amd.model import BestSubsetSelection

    X, y, groups, hidden, _ = suppressor(THREES["ng"], **THREES["design"])
    ref = suppressor_ref(THREES["ng"], THREES["K"], **THREES["design"])
    assert set(hidden) <= set(np.flatnonzero(ref["active"]))
    assert_below_prefix(ref, search_rank(X, y, groups=groups), THREES["ng"])
    est = BestSubsetSelection(groups=groups, sparse_bound=THREES["K"], big_M=1000).fit(X, y)
    compare(est, ref, X, y)


# ---- 5. the box at many columns and below the prefix ------------------------------------------------------------------------
def test_box_binds_below_the_prefix():
    from sparselm_amd.model import BestSubsetSelection

    X, y, _, _, _ = suppressor(20)
    big_M = 0.6 * float(np.max(np.abs(suppressor_ref(20, 4)["coef"])))
    ref = suppressor_ref(20, 4, big_M=big_M)
    assert np.isclose(np.max(np.abs(ref["coef"])), big_M, rtol=1e-9, atol=0)  # it binds
    assert_below_prefix(ref, search_rank(X, y), 20)
    est = BestSubsetSelection(sparse_bound=4, big_M=big_M).fit(X, y)
    compare(est, ref, X, y)
    assert np.max(np.abs(est.coef_)) <= big_M


def test_box_binds_at_many_columns():
    from sparselm_amd.model import BestSubsetSelection

    X, y, groups, wide, pair = twenty_and_singletons()
    big_M = 0.6 * float(np.max(np.abs(twenty_and_singletons_ref()["coef"])))
    ref = twenty_and_singletons_ref(big_M=big_M)
    assert np.isclose(np.max(np.abs(ref["coef"])), big_M, rtol=1e-9, atol=0)  # it binds
    rank = search_rank(X, y, groups=groups)
    assert ref["active"][wide]
    assert_below_prefix(ref, rank, 24, at_least=1)
    est = BestSubsetSelection(groups=groups, sparse_bound=3, big_M=big_M).fit(X, y)
    compare(est, ref, X, y)
    assert np.max(np.abs(est.coef_)) <= big_M


def test_box_changes_the_winner_at_many_columns():
    """A box tight enough to take the hidden pair's large coefficients away: the unboxed order of the supports is then
    wrong, and only boxed values -- the back-substitution that notices the box and the descent inside it, at 22 columns
    and more -- give the reference's winner."""
    from sparselm_amd.model import BestSubsetSelection

    X, y, groups, wide, pair = twenty_and_singletons()
    free = twenty_and_singletons_ref()
    big_M = 0.12 * float(np.max(np.abs(free["coef"])))  # (about 0.40: above every coefficient of the wide group, far below the pair's 3.3)
    ref = twenty_and_singletons_ref(big_M=big_M)
    # it binds on the unboxed winner, so hard that another support wins -- one that lies inside the box
    assert np.max(np.abs(free["coef"])) > big_M > np.max(np.abs(ref["coef"]))
    assert not np.array_equal(ref["active"], free["active"]) and ref["active"][wide]
    print(f"supports {ref['n_supports']}, unboxed winner's search ranks {winner_ranks(free, search_rank(X, y, groups=groups)).tolist()}, boxed "
          f"{winner_ranks(ref, search_rank(X, y, groups=groups)).tolist()}")
    est = BestSubsetSelection(groups=groups, sparse_bound=3, big_M=big_M).fit(X, y)
    compare(est, ref, X, y)
    assert np.max(np.abs(est.coef_)) <= big_M


# ---- 6. dependent columns below the prefix --------------------------------------------------------------------------------
def test_exact_copy_below_the_prefix():
    """19 columns of the design and, as column 19, an exact copy of the hidden column of search rank 17: the copy ties with
    it and takes rank 18.  Two supports then tie exactly, so the reference is the brute force WITHOUT the copy (the optimum's
    value and fitted values are the same) and the engine's support is compared after mapping the copy onto its original."""
    from sparselm_amd.model import BestSubsetSelection

    X19, y, _, hidden, _ = suppressor(19)
    base = search_rank(X19, y)
    orig = int(np.flatnonzero(base == 17)[0])
    assert orig in hidden
    X = np.column_stack([X19, X19[:, orig]])
    rank = search_rank(X, y)
    assert rank[orig] == 17 and rank[19] == 18
    ref = suppressor_ref(19, 4)
    assert ref["gap"] >= GAP_MIN and ref["kappa"] <= KAPPA_MAX and ref["active"][orig] and ref["n_supports"] <= MAX_SUPPORTS
    est = BestSubsetSelection(sparse_bound=4, big_M=1000).fit(X, y)
    info = est.solver_info_
    print(f"reference objective {ref['objective']:.12e}, engine {info['objective']:.12e}, nodes {info['nodes']}, active "
          f"{np.flatnonzero(est.active_groups_)}")
    assert info["proven_optimal"] and info["lower_bound"] == info["objective"]
    assert not (est.coef_[orig] != 0 and est.coef_[19] != 0) and not (est.active_groups_[orig] and est.active_groups_[19])
    folded = est.active_groups_[:19].copy()
    folded[orig] |= est.active_groups_[19]
    np.testing.assert_array_equal(folded, ref["active"])
    assert abs(info["objective"] - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])
    assert abs(objective_of(X, y, est.coef_, int(est.active_groups_.sum())) - ref["objective"]) <= OBJ_RTOL * abs(ref["objective"])
    fit_ref = X19 @ ref["coef"]
    assert np.max(np.abs(X @ est.coef_ - fit_ref)) <= COEF_RTOL * np.max(np.abs(fit_ref))


DEPENDENT = dict(dependent=0.118)  # D's score 1.28 gamma^2 = 0.018: between the two pairs' 0.022 and 0.014


def dependent_group():
    """20 groups, 21 columns: P = {a, b} in the prefix, D (which depends on P) and the four hidden columns below it."""
    X, y, groups, hidden, (P, D) = suppressor(20, **DEPENDENT)
    return X, y, groups, P, D, hidden


@functools.lru_cache(maxsize=None)
def dependent_group_ref(needed):
    X, y, groups, P, D, hidden = dependent_group()
    hierarchy = None
    if needed:  # the hidden column met last before D needs it
        rank = search_rank(X, y, groups=groups)
        hierarchy = [[] for _ in range(20)]
        hierarchy[int(max((h for h in hidden if rank[h] < rank[D]), key=lambda h: rank[h]))] = [D]
    return brute_force(X, y, groups=groups, K=5, big_M=1000, hierarchy=hierarchy), hierarchy


@pytest.mark.parametrize("needed", [False, True])
def test_dependent_group_below_the_prefix(needed):
    """Unneeded, D's include brings no column and is dropped: the search must go on to its exclude branch, where the
    hidden columns of later rank wait.  Needed by a winning group, D must stay and cost its slot."""
    from sparselm_amd.model import BestSubsetSelection

    X, y, groups, P, D, hidden = dependent_group()
    rank = search_rank(X, y, groups=groups)
    ref, hierarchy = dependent_group_ref(needed)
    free, _ = dependent_group_ref(False)
    print(f"rank of P {rank[P]}, of D {rank[D]}, of the hidden columns {rank[hidden].tolist()}")
    assert rank[P] < PREFIX <= rank[D] and ref["active"][P]
    assert_below_prefix(ref, rank, 20)
    if needed:
        child = next(i for i, row in enumerate(hierarchy) if row)
        assert ref["active"][D] and ref["active"][child] and PREFIX <= rank[child] < rank[D] and not free["active"][D]
        assert ref["active"].sum() == 5 and not np.array_equal(ref["active"], free["active"])  # D took a slot
    else:
        assert not ref["active"][D]
        assert any(ref["active"][h] and rank[h] > rank[D] for h in hidden)  # a winner lies beyond D's exclude branch
    est = BestSubsetSelection(groups=groups, sparse_bound=5, hierarchy=hierarchy, big_M=1000).fit(X, y)
    compare_singular(est, ref, X, y) if needed else compare(est, ref, X, y)
    if needed:
        assert_parents_active(est.active_groups_, hierarchy, list(range(20)))
        assert not est.coef_[groups == D].any()  # the dependent column stays at zero


def test_fewer_rows_than_columns_below_the_prefix():
    from sparselm_amd.model import BestSubsetSelection

    design = dict(n=14, tau=0.5, noise=0.02)
    X, y, _, hidden, _ = suppressor(20, **design)
    ref = suppressor_ref(20, 4, **design)
    assert set(hidden) <= set(np.flatnonzero(ref["active"]))
    assert_below_prefix(ref, search_rank(X, y), 20)
    est = BestSubsetSelection(sparse_bound=4, big_M=1000).fit(X, y)
    compare(est, ref, X, y)


# ---- 7. every support is visited once -------------------------------------------------------------------------------------
def expected_nodes(ng, K):
    """``nodes`` counts include attempts that pass the hierarchy (csrc/l0_kernels.hpp).  With nothing to prune but the
    cardinality: a ticket whose prefix has c groups makes min(c, K) attempts inside the prefix (it ends at the first level it
    reaches with K groups held), and, when c < K, one attempt below the prefix for every non-empty set of at most K - c of the
    remaining ng - 16 groups -- the attempt that completes that set."""
    rest = ng - PREFIX
    return sum(comb(PREFIX, c) * (min(c, K) + sum(comb(rest, s) for s in range(1, K - c + 1))) for c in range(PREFIX + 1))


@pytest.mark.parametrize("ng", [17, 20])
def test_every_support_is_visited_once(ng):
    from sparselm_amd.model import BestSubsetSelection

    K, n = 3, 60
    rng = np.random.default_rng(30 + ng)
    X = rng.standard_normal((n, ng))
    y = X @ rng.standard_normal(ng) + rng.standard_normal(n)
    ref = brute_force(X, y, K=K, big_M=1000)
    r_all = X @ np.linalg.lstsq(X, y, rcond=None)[0] - y
    q_all = float(r_all @ r_all - y @ y) / (2 * n)
    # the bound q_all + alpha (|S| + 1) >= incumbent cannot fire: alpha = 0 and q_all is below every value the search can hold
    assert q_all < ref["objective"] * (1 + 1e-9) and np.linalg.matrix_rank(X) == ng and ref["n_supports"] <= MAX_SUPPORTS
    fits = [BestSubsetSelection(sparse_bound=K, big_M=1000).fit(X, y) for _ in range(2)]
    compare(fits[0], ref, X, y)
    print(f"nodes {fits[0].solver_info_['nodes']}, {fits[1].solver_info_['nodes']}; expected {expected_nodes(ng, K)}")
    assert fits[0].solver_info_["nodes"] == fits[1].solver_info_["nodes"] == expected_nodes(ng, K)
