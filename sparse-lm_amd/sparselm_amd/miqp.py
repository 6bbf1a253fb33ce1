"""The reference's five mixed-integer estimators (``sparselm.model``'s ``BestSubsetSelection``,
``RidgedBestSubsetSelection``, ``RegularizedL0``, ``L1L0``, ``L2L0``) in one place, all solved exactly by the depth-first
search over supports on the GPU.

``from sparselm_amd.miqp import L1L0`` is the import path of ``L1L0``.  ``sparselm_amd.model`` exports the other four
(``model.MIQP_ESTIMATORS``), as before.

``l0_profile`` / ``L0Profile`` (``model/_l0_profile.py``) are here too, beside ``__all__``'s five estimator names: one search
that returns the best support of every size, from which best subset at every bound and the regularised optimum at every
``alpha`` are read off.  ``l0_profile_cv`` / ``L0ProfileCV`` (``model/_l0_cv.py``) do that for every fold of a cross-validation and for
all rows from one launch, and read a whole grid off the tables.  ``l1l0_profile`` / ``L1L0Profile`` (``model/_l1l0_profile.py``) are the
profile under an l1 term: ``L1L0`` at every ``alpha`` from one search per ``eta``, up to 128 columns with
``solver_options={"wide": True}``.  ``l1l0_profile_cv`` / ``l2l0_profile_cv`` / ``L0ProfileGridCV`` (``model/_l0_grid_cv.py``) cross-validate
``L1L0`` and ``L2L0`` over (alpha, eta): every (fold, eta) profile from one launch, the grid read off the tables.

``l0_local_search`` / ``L0LocalPath`` (``model/_l0_local.py``) are NOT exact: coordinate descent with hard thresholding and
one-for-one swaps for the ``RegularizedL0`` / ``L2L0`` objective over a whole (alpha, eta) grid from one launch per round, for up
to 1024 columns -- beyond the 128 at which every search above stops.  They prove nothing and say so (``proven_optimal_`` is False).
``l0_local_cv`` / ``L0LocalCV`` (``model/_l0_local_cv.py``) cross-validate that search: every fold's grid and the grid of all rows from
one launch per round.  ``l0_local_subsets`` / ``L0LocalSubsets`` (``model/_l0_local_subsets.py``) are that search in the
CARDINALITY form -- an incumbent for ``BestSubsetSelection`` / ``RidgedBestSubsetSelection`` at every ``sparse_bound`` of a list,
the approximate twin of ``l0_profile`` up to 1024 columns -- and ``l0_local_subsets_cv`` / ``L0LocalSubsetsCV``
(``model/_l0_local_subsets_cv.py``) cross-validate the size.  ``l0_local_group_search`` / ``L0LocalGroupPath``
(``model/_l0_local_groups.py``) are the local search WITH ``groups=`` AND ``hierarchy=`` -- the estimators' arguments, for the few hundred
to a thousand grouped columns of a cluster expansion: a group descent and one-for-one group swaps on
``1/2 b^T (G + 2 eta I) b - c^T b + alpha |cl(S)|``; they prove nothing, and the screen of the descent can miss a group.
``l0_local_group_cv`` / ``L0LocalGroupCV`` (``model/_l0_local_groups_cv.py``) cross-validate it, one launch per round.
``l1l0_local_search`` / ``L1L0LocalPath`` (``model/_l1l0_local.py``) are the local search WITH AN L1 TERM, the approximate answer to
``L1L0`` beyond its 64 columns: ``1/2 b^T (G + 2 ridge I) b - c^T b + eta ||b||_1 + alpha ||b||_0`` over an ``(alpha, eta)`` grid, ``eta``
the l1 weight as in ``L1L0``; ``l1l0_local_cv`` / ``L1L0LocalCV`` (``model/_l1l0_local_cv.py``) cross-validate it.  Nothing is proven.
``l0_local_bound`` / ``L0LocalBound`` (``model/_l0_local_bound.py``) are the LOCAL BOUND, the half the local search lacks: a PROVEN lower
bound on the objective of ``l0_local_search`` at every cell of its ``(alpha, eta)`` grid, up to 1024 columns, from one launch;
``L0LocalBound.gap(path)`` is the proven relative gap per cell.  Tight with a ridge or a box that binds, weak at ``eta = 0`` under a loose
``big_M``.
``l0_local_prove`` / ``L0LocalProof`` (``model/_l0_local_prove.py``) are the LOCAL PROOF: branch and bound on that bound, pruned against the
local search's incumbent, one launch a round for the nodes of every cell; a cell whose tree closes is PROVEN OPTIMAL -- with a ridge or
a box that binds it does, at ``eta = 0`` with more columns than rows it does not, and the proven gap reached is returned.
``l0_local_group_prove`` / ``L0LocalGroupProof`` (``model/_l0_local_group_prove.py``) are that proof WITH GROUPS AND A HIERARCHY: branch
and bound over group nodes for ``l0_local_group_search``'s objective, the hierarchy in the branching; it closes with a ridge or a box
that binds and not at ``eta = 0`` under a loose box or with deep hierarchies whose free groups are cheap.
"""

from .model._l0_cv import L0ProfileCV, l0_profile_cv  # noqa: F401  (the profiles of every CV fold from one launch; outside __all__)
from .model._l0_grid_cv import L0ProfileGridCV, l1l0_profile_cv, l2l0_profile_cv  # noqa: F401  (CV over (alpha, eta) from one launch; outside __all__)
from .model._l0_local import L0LocalPath, l0_local_search  # noqa: F401  (approximate, up to 1024 columns; outside __all__)
from .model._l0_local_bound import L0LocalBound, l0_local_bound  # noqa: F401  (a proven lower bound for the local search's grid; outside __all__)
from .model._l0_local_prove import L0LocalProof, l0_local_prove  # noqa: F401  (branch and bound on the local bound: proven optimal where the tree closes; outside __all__)
from .model._l0_local_group_prove import L0LocalGroupProof, l0_local_group_prove  # noqa: F401  (the local proof with groups and a hierarchy; outside __all__)
from .model._l0_local_cv import L0LocalCV, l0_local_cv  # noqa: F401  (the local search of every CV fold from one launch per round; outside __all__)
from .model._l0_local_groups import L0LocalGroupPath, l0_local_group_search  # noqa: F401  (the local search with groups and a hierarchy; outside __all__)
from .model._l0_local_groups_cv import L0LocalGroupCV, l0_local_group_cv  # noqa: F401  (its cross-validation, one launch per round; outside __all__)
from .model._l0_local_subsets import L0LocalSubsets, l0_local_subsets  # noqa: F401  (approximate best subsets of every size; outside __all__)
from .model._l0_local_subsets_cv import L0LocalSubsetsCV, l0_local_subsets_cv  # noqa: F401  (their cross-validation, one launch per round; outside __all__)
from .model._l0_profile import L0Profile, l0_profile  # noqa: F401  (not estimators: outside __all__, which tests pin)
from .model._l1l0 import L1L0
from .model._l1l0_local import L1L0LocalPath, l1l0_local_search  # noqa: F401  (the local search with an l1 term, up to 1024 columns; outside __all__)
from .model._l1l0_local_cv import L1L0LocalCV, l1l0_local_cv  # noqa: F401  (its cross-validation, one launch per round; outside __all__)
from .model._l1l0_profile import L1L0Profile, l1l0_profile  # noqa: F401  (L1L0 at every alpha from one search; outside __all__)
from .model._miqp import L2L0, BestSubsetSelection, RegularizedL0, RidgedBestSubsetSelection

__all__ = ["BestSubsetSelection", "RidgedBestSubsetSelection", "RegularizedL0", "L1L0", "L2L0"]
