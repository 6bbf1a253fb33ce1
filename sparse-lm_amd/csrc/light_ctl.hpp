// The control block of the certified partial passes (light_kernels.hpp), in a header of its own: the tail kernels
// (tail_kernels.hpp) keep its per-lane slack and epoch in step with the base gradient they store.
#pragma once
#include <stdint.h>

#include "../../include/slm_engine.h"

namespace slm {

constexpr int LT_CAP = 1024;  // borderline columns one attempt may read (0.8 MB each at n = 100k)
constexpr int LT_LANES = 8;   // live lanes one attempt serves: their points and their moves share sixteen MFMA columns

// Invariant, per lane l: the base gradient gprev is exact on every column j with stamp[j] == epoch[l] (on every column when
// epoch[l] == 0) and within c_j slack[l] of the true gradient at zprev elsewhere.  slack / epoch change only where gprev
// does: the tail kernel sets them to 0 / 0 when it stores a gradient of a pass over X, to the attempt's pending values when
// it accepts a point on the hybrid gradient of a light pass, and leaves them on a rejected candidate -- and for every lane
// the pass does not serve.
struct LightCtl {
  int32_t ok;        // the attempt of this pass stands: the kernels of the pass over X behind it return at once
  int32_t n_cols;    // borderline columns listed (lt_idx)
  int32_t n_live;    // live lanes of the attempt ...
  int32_t lane_of[LT_LANES];  // ... and which they are
  int32_t attempts;  // over the solve
  int32_t used;      // ... of which stood (passes over X saved)
  int32_t cols_total;  // borderline columns read by all of them
  int32_t why;       // why the last attempt stood down: 1 too many live lanes, 2 a live lane off W or without the set,
                     // 3 too many borderline columns, 4 W holds a column a lane's hybrid gradient is not exact on (SLM_TRACE=3)
  int32_t id;        // number of the attempt under way (1, 2, ...: `attempts` as light_prepare_kernel counted it)
  int32_t epoch[SLM_MAX_LANES];  // per LANE: the attempt its base gradient g(z) comes from, 0: from a pass over X.  A hybrid
                                 // gradient is exact on the columns that attempt stamped (LightArgs::stamp) -- W and the
                                 // borderline set of its time -- and the working set's model reads g(z) on ALL of W: a lane
                                 // whose W has since taken in a column outside that set goes back to a pass over X (why 4)
  int32_t pend_epoch[SLM_MAX_LANES];  // per LANE: epoch / slack of the hybrid gradient the attempt under way gives a live
  double pend_slack[SLM_MAX_LANES];   // lane -- what the tail commits if it accepts its point on it (light_select_kernel)
  double D[LT_LANES];            // ||X_W (b - z)|| / sqrt(n) of live lane s
  double slack[SLM_MAX_LANES];   // per LANE: what its base gradient g(z) may be off by, in units of c_j, outside the columns
                                 // it is exact on: 0 after a pass over X, + D after every light pass
};

}  // namespace slm
