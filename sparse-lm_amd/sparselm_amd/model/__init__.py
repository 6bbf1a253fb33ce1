"""The reference's estimators under its public names.

The reference exports 16 estimators from ``sparselm.model``.  Served here:

* the ten Lasso-family ones plus OLS (``__all__``: ``_lasso.py``, ``_adaptive_lasso.py``) -- convex problems, solved by the
  proximal-gradient engine;
* four of the mixed-integer ones (``MIQP_ESTIMATORS``: ``BestSubsetSelection``, ``RidgedBestSubsetSelection``,
  ``RegularizedL0``, ``L2L0`` -- ``_miqp.py``) -- solved EXACTLY by a depth-first search over supports on the GPU
  (``slm_solve_l0``) for up to 64 columns and 64 groups, where the reference needs Gurobi or SCIP behind cvxpy.

``from sparselm_amd.model import L2L0`` works; the four are kept out of ``__all__`` because they share neither the
penalty interface of the Lasso family, which is what ``__all__`` enumerates (they take linear constraints too, through ``add_constraints`` alone,
solved inside the search: ``slm_solve_l0_constrained``).  The fifth, ``L1L0``,
is served by the same search in its l1 mode; its import path is ``sparselm_amd.miqp.L1L0`` (``sparselm_amd.miqp`` exports
all five), and it is not a name of this module.
"""

from . import _adaptive_lasso as _adaptive
from . import _lasso as _plain
from . import _miqp

__all__ = list(_plain.__all__) + list(_adaptive.__all__)
globals().update({name: getattr(_plain, name) for name in _plain.__all__})
globals().update({name: getattr(_adaptive, name) for name in _adaptive.__all__})

MIQP_ESTIMATORS = tuple(_miqp.__all__)
globals().update({name: getattr(_miqp, name) for name in _miqp.__all__})
