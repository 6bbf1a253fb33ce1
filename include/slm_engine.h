/*
 * slm_engine.h -- C ABI of the MI355X (gfx950) proximal-gradient fit engine that replaces the
 * cvxpy solve of CederGroupHub/sparse-lm's Lasso-family estimators.
 *
 * Drop-in boundary.  The one reference interface this library stands in for is
 *
 *     CVXRegressor._solve(self, X, y, solver_options) -> beta
 *         src/sparselm/model/_base.py:512-519        (problem.solve(...); return beta.value)
 *     overridden by AdaptiveLasso._solve
 *         src/sparselm/model/_adaptive_lasso.py:206-232  (re-weighting loop around the same solve)
 *
 * called once per fit at src/sparselm/model/_base.py:201 with already validated, centred and
 * re-weighted float64 arrays.  The problem solved is the one the reference assembles in cvxpy:
 *
 *     minimise_beta  1/(2n) ||X beta - y||^2                      (model/_lasso.py:109-121)
 *                  + sum_j a_j |beta_j|                           (Lasso :99-107, SGL :627-639,
 *                                                                  AdaptiveLasso _adaptive_lasso.py:167-175)
 *                  + sum_g b_g ||beta_g||_2                       (GroupLasso :267-275,
 *                                                                  AdaptiveGroupLasso _adaptive_lasso.py:354-362)
 *                  + 1/2 sum_g d_g ||beta_g||_2^2                 (RidgedGroupLasso :795-811)
 *
 * Conventions: plain C types only; every function returns an slm_status (0 = ok); no C++
 * exception crosses the ABI; slm_last_error() returns a thread-local message for the last failure
 * on the calling thread.  All floating-point buffers are IEEE fp64.  A handle is not thread-safe;
 * different handles are.  Host pointers are borrowed only for the duration of a call.
 * There is NO CPU fallback: every entry point needs a visible gfx950 device and fails with
 * SLM_ERR_NO_DEVICE / SLM_ERR_HIP otherwise.
 */
#ifndef SLM_ENGINE_H
#define SLM_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLM_ABI_VERSION 24

typedef enum slm_status {
  SLM_OK = 0,
  SLM_ERR_BAD_ARG = 1,      /* -> ValueError  */
  SLM_ERR_OOM = 2,          /* -> MemoryError */
  SLM_ERR_HIP = 3,          /* -> RuntimeError (HIP runtime / kernel failure) */
  SLM_ERR_NO_DEVICE = 4,    /* -> RuntimeError (no gfx950 device visible) */
  SLM_ERR_COMM = 5,         /* -> RuntimeError (RCCL failure) */
  SLM_ERR_NOT_CONVERGED = 6,/* informational: reported per path point, never returned by solve; slm_solve_l0 returns
                               it (with valid outputs) when its node budget ran out */
  SLM_ERR_NON_FINITE = 7,   /* -> RuntimeError: non-finite value in the iterate (the reference's
                               counterpart is cvxpy's SolverError / "infeasible" RuntimeError,
                               model/_adaptive_lasso.py:216-220) */
  SLM_ERR_UNSUPPORTED = 8
} slm_status;

typedef struct slm_engine slm_engine;   /* one per (process, device): stream, workspace          */
typedef struct slm_dataset slm_dataset; /* device-resident (X, y[, row weights][, groups]) + state */

/* ---- library ------------------------------------------------------------------------------- */
int slm_abi_version(void);
const char* slm_last_error(void);
int slm_device_count(int* count_out);

/*
 * Page-locked host memory for result buffers (betas_out / group_norms_out of the solve calls).  Any host pointer is
 * accepted there; a buffer from here is written by the copy engine directly, while into ordinary memory the HIP
 * runtime first locks the caller's pages and keeps the registration -- freeing such memory afterwards (numpy
 * releasing a 2 MB result array, what the reference's `coef_` assignment of model/_base.py:201-202 amounts to) then
 * stalls the next submissions for milliseconds.  The binding recycles these blocks (sparselm_amd._engine._HostPool).
 */
int slm_host_alloc(size_t bytes, void** out);
int slm_host_free(void* ptr);

/* ---- engine lifecycle ------------------------------------------------------------------------ */
int slm_engine_create(int device_id, slm_engine** out);
int slm_engine_destroy(slm_engine* eng);
/* Blocks until all work queued on the engine's stream has finished. */
int slm_engine_synchronize(slm_engine* eng);
/* The SLM_* environment variables are read once per process, when the library first needs one.
   This reads them again: for tests and A/B tools that change a variable after the library was loaded. */
int slm_reload_knobs(void);
/* Device facts used by bench.py / DESIGN.md: out[0]=compute units, out[1]=LDS bytes per CU,
   out[2]=total HBM bytes, out[3]=free HBM bytes, out[4]=wavefront size, out[5]=clock kHz. */
int slm_engine_device_info(slm_engine* eng, int64_t out[6], char* name_out, int name_len);

/* ---- dataset --------------------------------------------------------------------------------- */
/*
 * Upload the (already preprocessed) design matrix and target the reference hands to _solve
 * (model/_base.py:201).  X is n x p with element (i, j) at X[i*row_stride + j*col_stride]
 * (strides in elements): C-order (col_stride == 1) and F-order (row_stride == 1) are accepted.
 * The engine keeps its own padded row-major copy in HBM; `row_weight` (nullable, length n, >= 0)
 * multiplies each row's squared residual: loss = 1/(2n) sum_i w_i (x_i beta - y_i)^2  -- used
 * for CV-fold masks and sample weights without re-uploading X.
 */
int slm_dataset_create(slm_engine* eng, const double* X, int64_t n, int64_t p, int64_t row_stride,
                       int64_t col_stride, const double* y, const double* row_weight,
                       slm_dataset** out);
/*
 * Same, from buffers that already live in this device's HBM (row-major, leading dimension ld >= p
 * elements).  The data are copied into the engine's padded layout; the caller keeps ownership.
 */
int slm_dataset_create_device(slm_engine* eng, const double* dX, int64_t n, int64_t p, int64_t ld,
                              const double* dy, const double* d_row_weight, slm_dataset** out);
/*
 * Does the uploaded X hold a value that is not finite?  *kind_out: 0 = all finite, bit 0 = a NaN, bit 1 = an infinity.
 * One read of X on the device (tens of microseconds per gigabyte) -- what lets the estimators' `fit` skip the host-side
 * scan of `check_array` on large arrays (the reference's `_validate_data`, model/_base.py:173: 0.145 s for the 4 GB of a
 * 100 000 x 5 000 design, two thirds of a whole fit here) and still raise scikit-learn's ValueError.
 */
int slm_dataset_nonfinite(slm_dataset* ds, int32_t* kind_out);
/*
 * Synthetic regression problem generated on the device (no host array): X_ij ~ N(0,1) iid from a
 * counter-based generator keyed by (seed, row_offset + i, j); y = X coef + noise_sd * N(0,1).
 * `coef` is a host vector of length p.  This is the law of sklearn.datasets.make_regression used by
 * BASELINE.json's configs; `row_offset` lets rank r of a row-sharded job own rows
 * [row_offset, row_offset + n) of one global matrix.
 */
int slm_dataset_create_synthetic(slm_engine* eng, int64_t n, int64_t p, uint64_t seed,
                                 int64_t row_offset, const double* coef, double noise_sd,
                                 slm_dataset** out);
/*
 * A copy of (X, y, row weights) on another engine of the SAME device, device to device: solves on different
 * engines run side by side (the launches between the passes of one beside the passes of the other), which a grid
 * search with more (fold, parameter) units than GPUs uses (sparselm_amd.model_selection.GridSearchCV(streams=...);
 * the reference's counterpart is n_jobs > 1 of model_selection.py:273).  Group structure is set again by the caller.
 */
int slm_dataset_clone(slm_dataset* src, slm_engine* eng, slm_dataset** out);
int slm_dataset_destroy(slm_dataset* ds);
int slm_dataset_shape(slm_dataset* ds, int64_t* n, int64_t* p, int64_t* ld);
/* Copy the engine's X (dense n x p, C-order) and/or y back to the host (either may be NULL). */
int slm_dataset_download(slm_dataset* ds, double* X_out, double* y_out);
/*
 * Centre the engine's copy of (X, y) in place by their row-weighted means -- what sklearn's
 * _preprocess_data does on the host for fit_intercept=True (reference model/_base.py:216-222) --
 * without a centred host copy of X: one pass for the means, one to subtract (about 2 ms for 4 GB).
 * x_mean_out (length p) and y_mean_out receive the means (either may be NULL); the caller forms
 * intercept_ = y_mean - x_mean . coef_ (sklearn LinearModel._set_intercept).
 */
int slm_dataset_center(slm_dataset* ds, double* x_mean_out, double* y_mean_out);
/* Replace the row weights (NULL => all ones).  Invalidates the cached Lipschitz constant. */
int slm_dataset_set_row_weights(slm_dataset* ds, const double* row_weight);
/*
 * Replace the targets (host vector of length n, finite) and keep X and everything derived from it.  Several
 * problems on one design -- the sub-problems of the splitting behind SparseGroupLasso(standardize=True)
 * (reference model/_lasso.py:616-639 with :249-252), whose targets change between solves -- then share one
 * upload.  A centred dataset expects targets that are already centred.
 */
int slm_dataset_set_targets(slm_dataset* ds, const double* y);
/*
 * Group structure: gid[j] in [0, n_groups) is the dense group index of feature j in the
 * reference's order (i-th sorted unique label <-> group i, model/_lasso.py:248).  Groups need not
 * be contiguous.  NULL / never called => every feature is its own group (model/_lasso.py:211-217).
 */
int slm_dataset_set_groups(slm_dataset* ds, const int32_t* gid, int32_t n_groups);
/* lambda_max(X^T W X)/n estimate (device power iteration, cached); safe upper-side margin applied. */
int slm_dataset_lipschitz(slm_dataset* ds, double* L_out);
/*
 * One evaluation of the hot kernel: g = X^T W (X z - y) / n  (g_out: length p, host) and
 * loss = 1/(2n) sum_i w_i (x_i z - y_i)^2 (loss_out nullable).  z == NULL means z = 0, which gives
 * -X^T W y / n (used for alpha_max).  `reps` > 1 repeats the launch and reports the mean kernel
 * time in ms through ms_out (nullable) -- the roofline probe.
 */
int slm_gradient(slm_dataset* ds, const double* z, double* g_out, double* loss_out, int32_t reps,
                 double* ms_out);
/*
 * The same evaluation by a NAMED route of the engine -- how the parity tests reach the kernels of the split pass through
 * the boundary (until ABI 17 they were switched by the environment variables SLM_GRAD_SPLIT / SLM_GRAD_LANES /
 * SLM_GRAD_LANE / SLM_PROBE_LANES, read inside slm_gradient).  opts == NULL: slm_gradient.
 *   route 0: the fused one-read kernel (two passes beyond 10 240 columns);
 *   route 1: the split pass -- residuals of the lane slots from X (rowdot*_mfma_kernel, or the ring kernel), then X^T R for
 *            all lane slots on one read of X (xtr*_mfma_kernel).  n_lanes (1..SLM_MAX_LANES) lanes all stand at z and the
 *            gradient of lane `lane_out` is returned: a lane of the second half is xtr32's second plane, or the vector
 *            units' share of xtr18 / xtr20.  More than one lane needs the column-major copy (built on first use).
 *            Where the dataset has no split pass the call falls back to route 0.
 *   route 2: the opening's sample product -- what a cold shared path hands to its first, provisional tail step: rows
 *            [0, n / SLM_SAMPLE_DIV), z ignored (zero), g_out = -X_s^T y / n_s, loss_out = y_s^T y_s / (2 n_s).  Through the
 *            dataset's fp32 image of those rows (built on first use; csrc/sample_kernels.hpp) where it has one, through the
 *            fp64 rows otherwise: SLM_SAMPLE_F64=1, row weights, no memory, or an entry of X that a float cannot hold.  One
 *            lane, no timed launches (ms_out = 0).  (Added under ABI 24: a new value of `route`, which older libraries refuse
 *            with SLM_ERR_BAD_ARG; no entry, structure or constant changes.)
 *   probe_lanes: lanes of the timed launches behind `reps` / ms_out (<= 0: one); xtr_only: time X^T R alone (route 1).
 * Reference counterpart: the gradient of the smooth term of /root/reference/src/sparselm/model/_lasso.py:109-121.
 */
typedef struct slm_gradient_opts {
  int32_t route;
  int32_t n_lanes;
  int32_t lane_out;
  int32_t probe_lanes;
  int32_t xtr_only;
} slm_gradient_opts;
int slm_gradient_ex(slm_dataset* ds, const double* z, const slm_gradient_opts* opts, double* g_out, double* loss_out,
                    int32_t reps, double* ms_out);

/*
 * Diagnostic: one gradient pass of n_lanes lanes, each with its OWN point, row weights and n_eff -- how the tests check the
 * lane index math of every multi-lane gradient kernel.  For lane l, over the rows used (all, or the first n_rows > 0):
 *   G_out[l] = X^T W_l (X Z[l] - y) / n_eff[l],   loss_out[l] = 1/(2 n_eff[l]) sum_i w_li (x_i . Z[l] - y_i)^2.
 *   route 0: the fused one-read kernel of n_lanes lanes (1..6 by width; the two-pass pair for one lane beyond 10 240 columns);
 *   route 1: the split pass (residuals from X, then X^T R for all lane slots); the column-major copy is built first;
 *   route 2: the covariance route, G_out[l] = G_k z_l - c_k with k = cov_index[l] an entry of slm_dataset_covariance*
 *            (its own n_eff; row_weights, n_eff and n_rows do not apply).
 * Z, G_out: [n_lanes][p] (C-order, host); row_weights: [n_lanes][n] (NULL: the dataset's for every lane); n_eff: [n_lanes]
 * (NULL: the dataset's n).  kernels_out (nullable): the residual and product kernels launched, ';'-separated, e.g.
 * "rowdot_ring_kernel<8,1,5,3>;xtr_mfma_kernel".  SLM_ERR_UNSUPPORTED where the route has no kernel for this call: there
 * is no fallback to another route.
 * Row-sharded datasets (routes 0 and 1): every rank calls with the same lanes; row_weights are THIS rank's rows, n_eff is the
 * job's (NULL: n_global), and the pass ends in the all-reduce a solve's passes end in -- every rank gets the gradient and loss
 * over all rows, bit for bit the same (one collective per call).  Route 2 and n_rows > 0 are SLM_ERR_UNSUPPORTED there (solves
 * take neither covariance passes nor a sample start on sharded rows), before any collective.  No reference counterpart
 * (tests only).
 */
int slm_gradient_lanes(slm_dataset* ds, int32_t route, int32_t n_lanes, const double* Z, const double* row_weights,
                       const double* n_eff, const int32_t* cov_index, int64_t n_rows, double* G_out, double* loss_out,
                       char* kernels_out, int32_t kernels_len);

/*
 * Diagnostic: a working set W built in stages and one gradient pass of n_lanes lanes on it -- how the tests check the kernels
 * that build W's Gram and gathered columns and the residual kernels that read them, against a reference.
 *   cols[0 : k_end[0]] is a fresh selection; build b > 0 appends cols[k_end[b-1] : k_end[b]] (distinct feature indices,
 *   k_end increasing, at most 512 in all).  Each build sets W's control block as the device's selection does (Kreal, K =
 *   max(16, Kreal rounded up to 16), k_new = the previous Kreal, idx = -1 on the padding) and queues what a solve queues after
 *   a selection: ws_gather_kernel (from the column-major copy of X, or from X with SLM_WSL_GATHER_X), the ws_xty kernels
 *   (SLM_WSL_XTY: ws_xty_partial_kernel and ws_xty_apply_kernel, what a dataset without the column-major copy runs;
 *   SLM_WSL_XTY_BUILD: what a solve queues on this dataset -- ws_gather_xty_kernel, which sums X_W^T y while it gathers, and
 *   ws_xty_apply_kernel; with SLM_WSL_GATHER_X the same as SLM_WSL_XTY), ws_gram_kernel, ws_gram_reduce_kernel -- or
 *   ws_gram_cov_kernel under route 2.
 *   Lanes with the same row weights and n_eff share a Gram (a row set); set_of_out[l] is lane l's, n_sets_out their number.
 *   Then one pass: route 1 the split pass (residuals from W for the lanes with on_ws[l] != 0, from X for the others, then X^T R),
 *   route 2 the covariance route (cov_index[l]: the lane's entry of slm_dataset_covariance*; no row weights, no n_eff).  A lane
 *   with on_ws must be zero outside W (SLM_ERR_BAD_ARG otherwise).  G_out[l], loss_out[l] as for slm_gradient_lanes.
 * gram_out: [n_sets][K][K] (nullable); xw_out: [n][K] (nullable; route 1); xty_out: [Kreal + 1] (SLM_WSL_XTY, SLM_WSL_XTY_BUILD):
 * -X_W^T y / n, then y^T y / 2n; with SLM_WSL_XTY_BUILD [Kreal + 2], last the number of entries of lane 0's gradient vector
 * outside W that the builds wrote to (0: they left everything but W's entries and the loss alone).  kernels_out (nullable): every kernel launched, ';'-separated, in order; the covariance
 * product is named "+listed" when every row set reads only W's rows of its Gram.  SLM_ERR_UNSUPPORTED where no kernel serves
 * the call.
 * Row-sharded datasets (route 1): every rank calls with the same lanes, columns and stages; row_weights are THIS rank's rows,
 * n_eff is the job's (NULL: n_global).  Every build stages this rank's part of the Grams, and what a sharded solve queues
 * behind a build follows: the all-reduce of the staging matrix and ws_publish_kernel (named in kernels_out) -- so gram_out is
 * the Gram over all rows, bit for bit the same on every rank; xw_out holds this rank's rows; the pass ends in the gradients'
 * all-reduce.  The row sets are agreed among the ranks (two lanes are one set where their weights agree on EVERY rank's rows:
 * one small all-reduce), so set_of_out and n_sets_out are the same everywhere.  n_builds + 2 collectives per call.  Route 2,
 * SLM_WSL_XTY and SLM_WSL_XTY_BUILD are SLM_ERR_UNSUPPORTED there (no covariance passes and no sample start on sharded rows),
 * before any collective.  No reference counterpart (tests only).
 */
#define SLM_WSL_GATHER_X 1u  /* gather from the row-major X, not the column-major copy */
#define SLM_WSL_XTY 2u       /* queue the ws_xty kernels with every build (the refinement after a row-sample pass) */
#define SLM_WSL_XTY_BUILD 4u /* X_W^T y with every build the way a solve gets it: out of the gather where it reads the column-major copy */
typedef struct slm_ws_lanes_opts {
  int32_t route;             /* 1: split pass, 2: covariance entries */
  int32_t n_lanes;           /* 1 .. SLM_MAX_LANES */
  const double* Z;           /* [n_lanes][p] */
  const int32_t* on_ws;      /* [n_lanes], NULL: no lane */
  const double* row_weights; /* [n_lanes][n], NULL: the dataset's */
  const double* n_eff;       /* [n_lanes], NULL: n */
  const int32_t* cov_index;  /* [n_lanes], route 2 */
  const int32_t* cols;       /* [k_end[n_builds - 1]] */
  const int32_t* k_end;      /* [n_builds] */
  int32_t n_builds;
  uint32_t flags;            /* SLM_WSL_* */
} slm_ws_lanes_opts;
int slm_working_set_lanes(slm_dataset* ds, const slm_ws_lanes_opts* opts, double* G_out, double* loss_out, int32_t* set_of_out,
                          int32_t* n_sets_out, double* gram_out, double* xw_out, double* xty_out, char* kernels_out,
                          int32_t kernels_len);

/*
 * Diagnostic: the working-set MODEL SOLVER alone, on a model the caller supplies -- how the tests check that it minimises
 *   m(x) = gprev_W . (x - zprev)_W + 1/2 (x - zprev)_W^T G (x - zprev)_W + pen(x)
 * on W and writes its point back as documented.  No X is read: the dataset carries p, ld, the groups and nothing else.
 *   cols[0 : kreal] are W's feature indices (distinct, kreal <= 512; on a dataset with groups: whole groups, each contiguous).
 *   gram is [n_sets][K][K], K = max(16, kreal rounded up to 16), zero on the padding; lane l uses gram[set_of[l]].
 *   Per lane: the expansion point zprev, its gradient gprev, the start z, the penalty vectors a0 [p], b0 / d0 [G] (G = p without
 *   groups), ONE path point (sa, sb, sd), tol and mode (0: accelerated lane, 1: spectral lane).  Lane l's path point has
 *   number l (what last_point is compared with).
 * The control blocks are set as ws_select_kernel and a solve leave them (valid, K, Kreal, idx = -1 on the padding, pos, gs, gl);
 * beta and everything else the solver is to write is filled with NaN; then exactly the launches of a pass's refinement are
 * queued (ws_solve_kernel<GROUPED, 0>, then <GROUPED, 1> with SLM_WMS_DIRECT; SLM_WS_ONE_SOLVER / SLM_WS_BB as in a solve).
 * Inputs must be finite, except gram and gprev under SLM_WMS_NONFINITE.  SLM_ERR_BAD_ARG for anything else,
 * SLM_ERR_UNSUPPORTED for row-sharded datasets.  No reference counterpart (tests only).
 */
#define SLM_WMS_DIRECT 1u     /* direct steps allowed (WsArgs::nt set: the second launch) */
#define SLM_WMS_HARD 2u       /* "start hard": WsCtl::hard_lane (and hard) preset */
#define SLM_WMS_INVALID 4u    /* WsCtl::valid = 0 */
#define SLM_WMS_BUILDING 8u   /* WsCtl::building = 1 */
#define SLM_WMS_DISABLED 16u  /* WsCtl::disabled = 1 */
#define SLM_WMS_STALE 32u     /* WsCtl::stale = 1 */
#define SLM_WMS_NONFINITE 64u /* gram and gprev may hold NaN / infinity */
typedef struct slm_ws_model_opts {
  int32_t n_lanes;           /* 1 .. SLM_MAX_LANES */
  int32_t kreal;             /* 1 .. 512 */
  const int32_t* cols;       /* [kreal] */
  int32_t n_sets;            /* 1 .. n_lanes */
  uint32_t flags;            /* SLM_WMS_* */
  const double* gram;        /* [n_sets][K][K] */
  const int32_t* set_of;     /* [n_lanes], NULL: all 0 */
  const double* zprev;       /* [n_lanes][p] */
  const double* gprev;       /* [n_lanes][p] */
  const double* z;           /* [n_lanes][p] */
  const double* a0;          /* [n_lanes][p] */
  const double* b0;          /* [n_lanes][G] */
  const double* d0;          /* [n_lanes][G] */
  const double* points;      /* [n_lanes][3]: sa, sb, sd */
  const double* tol;         /* [n_lanes] */
  const int32_t* mode;       /* [n_lanes] */
  const double* Lw;          /* [n_sets] WsCtl::Lw preset, NULL: 0 (the power iteration runs) */
  const int32_t* repeats;    /* [n_lanes] WsCtl::repeats preset, NULL: 0 */
  const int32_t* last_point; /* [n_lanes] WsCtl::last_point preset, NULL: -1 */
  const int32_t* last_cols;  /* [n_lanes] WsCtl::last_cols preset, NULL: 0 */
} slm_ws_model_opts;
typedef struct slm_ws_model_out {
  double* z;              /* [n_lanes][p] */
  double* beta;           /* [n_lanes][p] */
  int32_t* served;        /* [n_lanes] WsCtl::served */
  double* mu;             /* [n_lanes] PathCtl::mu (preset -1) */
  int32_t* zsup;          /* [n_lanes] PathCtl::zsup (preset -1) */
  double* t;              /* [n_lanes] PathCtl::t (preset 7) */
  int32_t* have_base;     /* [n_lanes] PathCtl::have_base (preset 1) */
  int32_t* zzero;         /* [n_lanes] PathCtl::zzero (preset 1) */
  int32_t* want_full;     /* [n_lanes] WsCtl::want_full as left behind */
  int32_t* repeats;       /* [n_lanes] */
  int32_t* hard_lane;     /* [n_lanes] */
  int32_t* last_point;    /* [n_lanes] */
  double* Lw;             /* [n_sets] */
  int32_t* counters;      /* [8]: refined, inner_iters, newton_steps, newton_fails, newton_nopd, newton_factors, newton_unknowns,
                             hard_next */
  char* kernels;          /* every kernel launched, ';'-separated, in order (nullable) */
  int32_t kernels_len;
} slm_ws_model_out;
int slm_working_set_model_solve(slm_dataset* ds, const slm_ws_model_opts* opts, slm_ws_model_out* out);

/*
 * Weighted squared error of m coefficient vectors, as many per pass over X as the fused kernel
 * table has lanes for this p:
 *   sse_out[k] = sum_i w_i (x_i . Z[k] - y_i)^2        (Z: m x p, C-order, host)
 * row_weight (length n, host, nullable => the dataset's) is typically the TEST mask of a CV fold, so
 * that hold-out scores come from the resident X instead of a host GEMM (the reference scores with
 * estimator.predict on X[test], model_selection.py:305-315).
 */
int slm_eval_sse(slm_dataset* ds, const double* Z, int32_t m, const double* row_weight, double* sse_out);

/*
 * The same for coefficient vectors that are zero outside n_cols <= 512 columns (the solutions of a
 * regularisation path): cols[n_cols] are those columns, Zs is m x n_cols (C-order, host).  The columns
 * are gathered once on the device and every vector then costs n x n_cols doubles instead of a share of
 * a pass over X.  SLM_ERR_UNSUPPORTED if n_cols > 512 (callers then use slm_eval_sse).
 */
int slm_eval_sse_sparse(slm_dataset* ds, const int32_t* cols, int32_t n_cols, const double* Zs, int32_t m,
                        const double* row_weight, double* sse_out);

/*
 * Diagnostic: x = H^-1 rhs for one dense symmetric positive definite m x m matrix (row-major, host,
 * m <= 512) with the one-workgroup blocked Cholesky the working-set model solver uses for its direct
 * steps (csrc/newton_kernels.hpp); mu_out (nullable) receives its estimate of lambda_min(H).
 * SLM_ERR_BAD_ARG when H is not numerically positive definite.  No reference counterpart (the
 * factorisations live inside the solvers cvxpy calls, model/_base.py:516-518); used by the tests.
 */
int slm_dense_spd_solve(slm_engine* eng, const double* H, int32_t m, const double* rhs, double* x_out,
                        double* mu_out);

/* ---- solve ----------------------------------------------------------------------------------- */
typedef struct slm_penalty {
  const double* a; /* length p, per-coefficient l1 weight; NULL => all ones            */
  const double* b; /* length G, per-group l2 weight;       NULL => all ones            */
  const double* d; /* length G, per-group ridge weight;    NULL => all ones            */
} slm_penalty;

/* Penalty at path point k is (sa*a, sb*b, sd*d).  `extrap` (k >= 2 only; 0 = plain warm start)
   starts point k from beta_{k-1} + extrap * (beta_{k-1} - beta_{k-2}): a secant prediction along
   the path (exact for the piecewise-linear Lasso path between kinks when
   extrap = (alpha_k - alpha_{k-1}) / (alpha_{k-1} - alpha_{k-2})).  It only moves the starting
   point; the solution of point k is unaffected. */
typedef struct slm_path_point {
  double sa, sb, sd, extrap;
} slm_path_point;

#define SLM_FLAG_NO_RESTART 1u   /* disable the gradient-scheme momentum restart        */
#define SLM_FLAG_PROFILE 2u      /* bracket every 2nd gradient launch with HIP events     */
#define SLM_FLAG_COLD_START 4u   /* do not warm-start point k+1 from point k             */
#define SLM_FLAG_FRESH_L 8u      /* re-estimate the Lipschitz constant even if cached     */
#define SLM_FLAG_FISTA_ONLY 16u  /* never use spectral steps (plain FISTA with restart)  */
#define SLM_FLAG_WORKING_SET 32u     /* Gram-assisted working-set refinement between passes even for
                                        small X (default: only when one pass over X costs more than
                                        the refinement, n*ld >= 2^26)                              */
#define SLM_FLAG_NO_WORKING_SET 64u  /* never refine: every iterate comes from a pass over X        */
#define SLM_FLAG_ON_CHIP 128u        /* the caller accepts the on-chip solver for problems whose Gram matrix fits a
                                        workgroup's LDS (p <= 128, n * ld <= 2^17 -- the sizes of the reference's own
                                        tests and README, tests/conftest.py:17-19, README.md:42-55): ONE launch per call,
                                        a workgroup per lane, accelerated proximal steps + conjugate gradients / Anderson
                                        acceleration on X^T W X / n held in LDS (small_kernels.hpp).  Same minimiser and the
                                        same meaning of `tol`; slm_point_info.mode is 2, n_iter counts matrix-vector products,
                                        slm_solve_stats.grad_launches is 1.  Ignored together with the flags that ask for
                                        a particular iteration (1, 2, 16, 32, 64); a point it does not settle hands the
                                        call to the general path.  Up to SLM_MAX_CELLS lanes whatever p.              */

#define SLM_FLAG_COVARIANCE 256u      /* passes take their gradients from the Grams of the call's row sets where
                                        slm_dataset_covariance() has built every one of them: G z - c, 8 p^2 bytes per row
                                        set and pass instead of a read of X (cov_kernels.hpp).  Same iteration, same
                                        results to rounding; ignored where a Gram is missing, on row-sharded datasets and
                                        for calls the on-chip solver takes                                            */

#define SLM_FLAG_NO_MODEL_GRAM 512u   /* lanes whose solutions outgrow the working set's 512 columns finish with plain
                                        steps (two reads of X each) instead of rounds on the model Gram -- for
                                        measurements: the results agree to the tolerance either way              */

#define SLM_FLAG_PROFILE_UNIT 1024u   /* with SLM_FLAG_PROFILE: the bracket of HIP events opens before the residual kernels of
                                        the split pass -- the whole gradient unit (residuals + X^T R), not the launch that
                                        streams X alone (bench.py: roofline.frac)                                   */

typedef struct slm_solve_opts {
  double tol;          /* relative distance to the minimiser a point is accepted at: stop when the KKT
                          residual ||G(z)||_2 (prox-gradient mapping) <= tol * mu * ||beta||_2, mu the
                          strong-convexity estimate of the face (slm_point_info.mu); <= 0 => 1e-8 */
  int32_t max_iter;    /* per path point; <= 0 => 10000                                  */
  int32_t check_every; /* iterations queued between host polls; <= 0 => automatic        */
  double L;            /* Lipschitz constant to use; <= 0 => slm_dataset_lipschitz()     */
  uint32_t flags;
} slm_solve_opts;

typedef struct slm_point_info {
  int32_t n_iter;    /* gradient evaluations spent on this point                         */
  int32_t status;    /* SLM_OK or SLM_ERR_NOT_CONVERGED                                  */
  double resid;      /* ||beta+ - z||_2 at exit                                          */
  double beta_norm;  /* ||beta||_2                                                       */
  double loss;       /* 1/(2n)||X z - y||_W^2 at the last gradient point                 */
  double L;          /* inverse step in use at exit (Lipschitz constant in FISTA mode)   */
  int32_t mode;      /* 1 = spectral (Barzilai-Borwein) steps, 0 = FISTA (after fallback), 2 = the on-chip
                        solver (SLM_FLAG_ON_CHIP)                            */
  int32_t rejects;   /* spectral candidates rejected so far in this solve                */
  double kkt;        /* KKT residual at exit: ||(z - prox_s(z - s grad f(z))) / s||_2 -- zero exactly at
                        the minimiser (the certificate SURVEY 8c-3 names; the reference's solver reports
                        its own through cvxpy's solver_stats, model/_base.py:516-518)               */
  double mu;         /* strong-convexity estimate the point was accepted with: kkt / mu bounds the
                        distance to the minimiser (smallest eigenvalue of the face Hessian from the model
                        solver's Cholesky factor, or the smallest curvature measured along the steps)  */
} slm_point_info;

typedef struct slm_solve_stats {
  int64_t grad_launches;  /* gradient kernels that did work                              */
  int64_t grad_timed;     /* how many of them were bracketed by events (SLM_FLAG_PROFILE) */
  double grad_ms_total;   /* sum of the device durations of the timed ones               */
  double wall_ms;         /* host wall clock of the call                                 */
  double lipschitz_ms;    /* part of wall_ms spent estimating L (0 if cached / given)    */
  int64_t ws_builds;      /* working sets selected and their Grams built from scratch       */
  int64_t ws_appends;     /* times columns were appended to the working set instead        */
  int64_t ws_refined;     /* iterates moved by the working-set refinement, all lanes       */
  int64_t ws_misses;      /* times an iterate left the working set (columns get appended)  */
  int64_t ws_columns;     /* columns in the working set at the end of the solve            */
  int64_t ws_inner_iters; /* proximal-gradient iterations of the model solver, all refinements */
  int64_t ws_direct_steps;/* direct (Cholesky) steps of the model solver: exact minimisation over the
                             face of the iterate, taken when the iteration is slow (ill-conditioned faces) */
  int64_t mg_rounds;      /* (lane, pass) pairs in which a lane beyond the working set took its next point from
                             the model Gram (an fp16 product of the whole of X^T W X / n: mg_kernels.hpp) instead
                             of a plain step; 0: the model Gram was not used                              */
  int64_t mg_inner_iters; /* proximal-gradient iterations on the model Gram, all lanes (one read of the
                             8 p^2-byte matrix each, for sixteen lanes)                                    */
  int64_t mg_rejected;    /* proposals from the model Gram that the true objective rejected              */
  double mg_build_ms;     /* host wall clock spent building the model Gram inside this call (0: it was
                             there already, or not used)                                                  */
  int64_t light_passes;   /* (ABI 19) re-verifications after a miss that were CERTIFIED PARTIAL passes instead of passes over
                             X (csrc/light_kernels.hpp): exact gradient on the working set and on the borderline columns,
                             a Cauchy-Schwarz certificate for the rest; not counted in grad_launches            */
  int64_t light_columns;  /* borderline columns those passes read from the column-major copy, in all */
} slm_solve_stats;

/*
 * Warm-started regularisation path: for k = 0..n_points-1 minimise the objective with penalty
 * (sa_k a, sb_k b, sd_k d), each point started from the previous solution (the first from
 * beta0, NULL => 0).  The whole path runs as one device-resident state machine; the host only
 * queues iterations and polls a flag.  betas_out: n_points x p (C-order, host);
 * group_norms_out: n_points x G (nullable); infos: n_points (nullable); stats nullable.
 * n_points == 1 is the plain _solve().
 *
 * Two things the solves of a dataset do with what the data already told them (working-set solves on a large X; every
 * reported point is verified by a gradient over all rows under the unchanged rule either way):
 *  - carried start: when beta0 of every lane is, bit for bit, the solution the dataset's LAST solve reported for that
 *    lane -- over the same rows and row weights; the penalty may differ: the rounds of an Adaptive* estimator
 *    (model/_adaptive_lasso.py:206-232), a refit -- the solve starts at the point whose gradient the engine still holds
 *    (within the tolerance of beta0) and does not run its first pass over the data.  SLM_NO_CARRY=1 turns it off.
 *  - sample start: a path on several lanes without a warm start opens on the first quarter of the rows -- enough to
 *    rank the features for the first working set, on which the model's linear term is then formed exactly from the
 *    gathered columns; nothing is accepted on the estimate.  SLM_NO_SAMPLE_START=1 opens on all rows.
 */
int slm_solve_path(slm_dataset* ds, const slm_penalty* pen, const slm_path_point* points,
                   int32_t n_points, const slm_solve_opts* opts, const double* beta0,
                   double* betas_out, double* group_norms_out, slm_point_info* infos,
                   slm_solve_stats* stats);

/*
 * Several independent problems ("lanes") on ONE pass over X per iteration: lane l has its own
 * penalty, path, warm start and -- optionally -- its own row weights (a CV-fold mask) and 1/n
 * scaling.  The fused gradient kernel streams X once and produces all lanes' gradients, so B lanes
 * cost the HBM traffic of one.  Used for the alpha sub-paths of one long path, for the folds of a
 * cross-validation, or both.  n_lanes <= SLM_MAX_LANES; SLM_ERR_UNSUPPORTED if no kernel variant
 * covers (p, n_lanes) -- callers then fall back to fewer lanes.  How many lanes a pass can serve:
 * the fused kernels go up to 4 at p = 5000 (6 up to 3072 columns: z and the accumulators of every
 * lane live in registers); on rows of up to 5120 columns working-set solves, and any solve on a large X
 * (n * ld >= 2^26 doubles), use the split pass, whose two halves -- residuals, then X^T R -- run on the
 * matrix cores for sixteen lanes per read of X.  slm_dataset_max_lanes() tells.  Working-set solves on such rows take up
 * to SLM_MAX_LANES = 32 lanes: two halves of sixteen, whose X^T R is ONE read of X for all thirty-two (a row of X in
 * registers is multiplied by both halves' residuals: 0.60-0.71 ms against 0.57 at 100k x 5k); calls of 17 to 20 lanes cost
 * what sixteen cost (lanes 17..20 ride on the vector units beside the sixteen on the matrix cores); covariance passes
 * take thirty-two as well (both halves' points against one read of every Gram); row-sharded solves stay at sixteen.
 */
#define SLM_MAX_LANES 32
/* ... and of a call the on-chip solver takes (SLM_FLAG_ON_CHIP on a dataset of p <= 128, n * ld <= 2^17): a workgroup per
 * lane, so the cells of a small grid search -- (candidate, fold) pairs, 50 in the reference's README example -- go in ONE
 * call.  slm_dataset_max_lanes() tells which of the two limits applies; a point the kernel does not settle sends the call
 * to the general path in chunks of SLM_MAX_LANES. */
#define SLM_MAX_CELLS 64
typedef struct slm_lane {
  const slm_penalty* pen;         /* NULL => all-ones base vectors                              */
  const slm_path_point* points;   /* this lane's warm-started path                              */
  int32_t n_points;
  const double* beta0;            /* length p warm start, NULL => 0                             */
  const double* row_weight;       /* length n, NULL => the dataset's row weights                */
  int64_t n_eff;                  /* 1/n_eff scaling of loss and gradient; <= 0 => dataset's    */
  double* betas_out;              /* n_points x p                                               */
  double* group_norms_out;        /* n_points x G, nullable                                     */
  slm_point_info* infos;          /* n_points, nullable                                         */
} slm_lane;

int slm_solve_lanes(slm_dataset* ds, const slm_lane* lanes, int32_t n_lanes,
                    const slm_solve_opts* opts, slm_solve_stats* stats);
/*
 * The re-weighting loop of the Adaptive* estimators inside ONE call (reference: AdaptiveLasso._solve,
 * src/sparselm/model/_adaptive_lasso.py:206-232 -- solve, renew the penalty weights from the solution, :364-374 for the
 * group norms, stop when the weights no longer move or after max_iter solves; the reference re-enters cvxpy once per
 * round).  Lane l's points are its rounds (n_points = max_iter, normally all (1, 1, 1)): after round k the weights become
 *     a_j <- coef_scale * (numerator / (|beta_j| + eps))            j < n_coef     (coef_scale != 0)
 *     b_g <- group_scale[g] * (numerator / (||beta_g||_2 + eps))    g < n_group    (group_scale != NULL)
 * -- the default update functions of the reference, operation for operation -- and the rounds end once the 2-norm of the
 * change of the weights is <= tol.  betas_out / group_norms_out / infos hold one row per round; rounds that were not run
 * have infos[k].n_iter == 0 and mode == 3, and rounds_out[l] says how many were.  Only for problems the on-chip solver
 * takes (the reference-sized ones): SLM_ERR_UNSUPPORTED otherwise, or when a round was not settled on chip -- the
 * caller then runs the loop itself over slm_solve_lanes, which is what it did before this call existed.
 */
typedef struct slm_reweight {
  double coef_scale;
  const double* group_scale;   /* length n_group, nullable */
  double numerator;
  double eps;
  double tol;
  int32_t n_coef;              /* leading coefficients that carry adaptive weights (an intercept column stays out) */
  int32_t n_group;
} slm_reweight;
int slm_solve_lanes_reweighted(slm_dataset* ds, const slm_lane* lanes, const slm_reweight* rules, int32_t n_lanes,
                               const slm_solve_opts* opts, slm_solve_stats* stats, int32_t* rounds_out);
/* How many lanes one slm_solve_lanes call on this dataset can take with these solve flags (callers
 * size their batches of CV folds / grid rows with it instead of probing for SLM_ERR_UNSUPPORTED). */
int slm_dataset_max_lanes(slm_dataset* ds, uint32_t flags, int32_t* max_lanes_out);
/* The lane count slm_solve_path_lanes takes for a path of n_points when the caller passes n_lanes = 0 (ABI 17: until then
   n_lanes = 0 was clamped to one lane, the strictly sequential warm-started path; callers that want that pass 1). */
int slm_dataset_path_lanes(slm_dataset* ds, int32_t n_points, uint32_t flags, int32_t* lanes_out);

/*
 * ONE warm-started path walked by n_lanes lanes that share each pass over X: the path is cut into
 * n_lanes contiguous ranges (the first warm-started from beta0, the others cold); a lane that runs
 * out of points takes over the upper half of what the busiest lane has left, so the lanes finish
 * together whatever the per-point cost profile is.  Same outputs as slm_solve_path.
 * n_lanes = 0 leaves the count to the engine (ABI 17), which weighs passes against their price: sixteen; eighteen or
 * twenty where that saves a pass of a path over a large X (a 50-point path: three passes instead of four when no point
 * meets a feature outside the working set); up to thirty-two for paths in contiguous ranges (group penalties: 50 points
 * on twenty-five lanes, two passes).  slm_dataset_path_lanes() tells.
 */
int slm_solve_path_lanes(slm_dataset* ds, const slm_penalty* pen, const slm_path_point* points,
                         int32_t n_points, int32_t n_lanes, const slm_solve_opts* opts,
                         const double* beta0, double* betas_out, double* group_norms_out,
                         slm_point_info* infos, slm_solve_stats* stats);

/*
 * SparseGroupLasso(standardize=True) -- the reference's lambda1 ||b||_1 + lambda2 sum_g w_g ||X_g b_g||_2
 * (src/sparselm/model/_lasso.py:616-639 with the standardised group norms of :249-252), which is no proximal penalty
 * on b -- by operator splitting with ALL sweeps in one launch (small_split_kernels.hpp), for problems the on-chip solver
 * takes (p <= 128, n * ld <= 131072, no row weights, not sharded, the groups' factors fitting LDS; otherwise
 * SLM_ERR_UNSUPPORTED and the caller runs the sweeps itself over slm_solve_lanes, sparselm_amd/model/_split.py):
 *   minimise 1/(2n)||X b - y||^2 + sum_j a[j] |b_j| + sum_g b[g] ||X_g b_g||_2 .
 * Stops when the primal residual ||M b - gamma|| and the dual residual are below opts->tol relative to their scales
 * (the rule of _split.py); the b-steps are solved to tol_inner (<= 0: min(tol, 1e-10)).  max_sweeps <= 0: 500.
 * warm != 0 continues from the splitting variables of the previous call on this dataset (the re-weighting loop of the
 * adaptive estimator) instead of rebuilding them from beta0.  info->n_iter = sweeps, info->rejects = matrix-vector
 * products of the b-steps, info->kkt / info->mu = primal / dual residual, info->L = rho at exit, info->status =
 * SLM_OK or SLM_ERR_NOT_CONVERGED (outputs are the last iterate).
 */
int slm_solve_standardized_sgl(slm_dataset* ds, const double* a, const double* b, const slm_solve_opts* opts,
                               double tol_inner, int32_t max_sweeps, const double* beta0, int32_t warm,
                               double* beta_out, double* group_norms_out, slm_point_info* info);

/*
 * Linear constraints lo <= A b <= hi on the l1 estimators (the reference's add_constraints, src/sparselm/model/_base.py:
 * 469-510; Lasso, AdaptiveLasso, OrdinaryLeastSquares with a = 0):
 *   minimise 1/(2n)||X b - y||^2 + sum_j a[j] |b_j|   subject to   lo <= A b <= hi
 * by an over-relaxed ADMM splitting with ALL sweeps in one launch (small_constrained_kernels.hpp).  A: m x p, row-major,
 * finite; lo / hi: m entries each, lo <= hi (equalities lo == hi; +-infinity allowed).  The on-chip solver takes
 * p <= 128, n * ld <= 131072, m <= 512, unweighted and unsharded datasets with singleton groups; anything else is
 * SLM_ERR_UNSUPPORTED and the caller runs the sweeps itself (sparselm_amd/model/_constrained.py).  A non-finite entry of
 * A or a row with lo > hi is SLM_ERR_BAD_ARG before anything is launched.  Stops when the primal residual ||A b - s|| and
 * the dual residual rho ||A^T (s - s_prev)|| are below opts->tol relative to their scales; the b-steps are solved to
 * tol_inner (<= 0: min(tol, 1e-10)).  max_sweeps <= 0: 500.  warm != 0 continues from the splitting variables (s, u, rho)
 * of the previous call on this dataset with the same m (the re-weighting rounds of AdaptiveLasso) instead of starting
 * from beta0.  lambda_out (m entries, may be NULL): the multipliers, 0 in grad f + d penalty + A^T lambda, > 0 only where
 * hi binds and < 0 only where lo binds.  info->n_iter = sweeps, info->rejects = matrix-vector products, info->kkt /
 * info->mu = primal / dual residual, info->L = rho at exit, info->loss = 1/(2n)||X b - y||^2, info->status = SLM_OK or
 * SLM_ERR_NOT_CONVERGED (outputs are the last iterate).
 */
int slm_solve_constrained(slm_dataset* ds, const double* a, const double* A, int32_t m, const double* lo, const double* hi,
                          const slm_solve_opts* opts, double tol_inner, int32_t max_sweeps, const double* beta0, int32_t warm,
                          double* beta_out, double* lambda_out, slm_point_info* info);

/*
 * (ABI 24) The exact l0 estimators -- the reference's mixed-integer family BestSubsetSelection, RidgedBestSubsetSelection,
 * RegularizedL0 and L2L0 (src/sparselm/model/_miqp/_best_subset.py:95-124, 215-248; _regularized_l0.py:115-144, 502-530),
 * which it hands to Gurobi / SCIP through cvxpy -- by a depth-first search over supports on chip (csrc/l0_kernels.hpp).
 * The reference's objectives divided by 2n (_miqp/_base.py:126-127, _regularized_l0.py:157-161, _base.py:544-546): with
 * G = X^T W X / n and c = X^T W y / n of the dataset (its row weights, its centring),
 *   minimise over supports S (sets of the dataset's GROUPS, slm_dataset_set_groups) and beta with supp beta in cols(S),
 *   |beta_j| <= big_M:      1/2 beta^T (G + 2 eta T) beta - c^T beta + alpha |S|
 *   subject to  |S| <= max_groups   and   i in S => need[i] subset of S.
 * T: p x p, row-major (only its symmetric part acts), NULL: the identity.  need: one mask per group over the groups (bit h
 * of need[i]: group i may only be active when group h is), NULL: no hierarchy.  max_nodes <= 0: the engine's default budget.
 * Up to 64 columns and 64 groups (SLM_ERR_UNSUPPORTED beyond, and on row-sharded datasets).  Negative or non-finite alpha
 * / eta, negative big_M, a need bit at or beyond the group count: SLM_ERR_BAD_ARG before anything is launched.  The
 * dataset's Gram is the one slm_dataset_covariance keeps (built on first use).
 * beta_out [p]: the winner's coefficients, recomputed once on the host from the Gram on its support (so they do not depend
 * on which wavefront found it); support_out: bit i = group i active; *lower_bound_out: the proven lower bound of the
 * objective, equal to it when the search finished; *nodes_out: group inclusions tried.  info->loss = 1/(2n)||X beta - y||_W^2,
 * info->n_iter = launches, info->kkt = the objective above, info->mu = the objective of the greedy seed, info->L = the
 * unconstrained quadratic value on all columns (the bound's q_all), info->mode = 4, info->status = SLM_OK or
 * SLM_ERR_NOT_CONVERGED.  When the node budget runs out every wavefront drains, the outputs hold the incumbent and the call
 * returns SLM_ERR_NOT_CONVERGED.
 */
int slm_solve_l0(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T /* p*p or NULL */,
                 double big_M, const uint64_t* need /* n_groups masks or NULL */, int64_t max_nodes /* <=0: default */,
                 double* beta_out, uint64_t* support_out, double* lower_bound_out, int64_t* nodes_out,
                 slm_point_info* info);

/*
 * (added under ABI 24: a new symbol beside slm_solve_l0, no existing entry, structure or constant changes, so the version
 * stays 24 -- a caller that needs it looks the symbol up.)  The reference's L1L0 (_regularized_l0.py:258-410, objective
 * :395-410, divided by 2n) by the same search in its l1 mode (csrc/l0_kernels.hpp, template parameter L1):
 *   minimise over supports S (sets of the dataset's GROUPS) and beta with supp beta in cols(S), |beta_j| <= big_M:
 *       1/2 beta^T G beta - c^T beta + eta_l1 ||beta||_1 + alpha |S|     subject to  i in S => need[i] subset of S
 * -- no cardinality bound and no ridge term.  A support's value is a lasso inside the box: the register Cholesky value
 * q(S) <= f(S) is an exact lower-bound filter in front of a cyclic coordinate descent with a soft-threshold over ALL
 * columns of the support (a dependent column can lower the value under an l1 term).  eta_l1 == 0 runs the very code of
 * slm_solve_l0(ds, alpha, n_groups, 0, NULL, ...).  The contract is slm_solve_l0's: up to 64 columns and 64 groups
 * (SLM_ERR_UNSUPPORTED beyond, and on row-sharded datasets); negative or non-finite alpha / eta_l1, negative big_M, a need
 * bit at or beyond the group count: SLM_ERR_BAD_ARG before anything is launched; SLM_ERR_NOT_CONVERGED with the incumbent
 * in the outputs when the node budget ran out.  beta_out: the winner's coefficients, recomputed once on the host by the
 * same descent and polished (the free non-zero coordinates solved exactly on their sign pattern, kept when signs and box
 * hold).  info as for slm_solve_l0, with info->L = the proven lower bound on the value of all columns that the subtree
 * bound used (the lasso dual value at a feasible point where that is above q_all) and info->rejects = descents run.
 */
int slm_solve_l0_l1(slm_dataset* ds, double alpha, double eta_l1, double big_M, const uint64_t* need /* n_groups masks or NULL */,
                    int64_t max_nodes /* <=0: default */, double* beta_out, uint64_t* support_out, double* lower_bound_out,
                    int64_t* nodes_out, slm_point_info* info);

/*
 * (added under ABI 24: a new symbol beside slm_solve_l0, no existing entry, structure or constant changes, so the version
 * stays 24 -- a caller that needs it looks the symbol up.)  The exact l0 PROFILE: one search (csrc/l0_kernels.hpp, template
 * parameter PROFILE) returns, for every size k = 0 .. max_groups, the best admissible support of exactly k groups for
 *       q(S) = min over beta, supp beta in cols(S), |beta_j| <= big_M, of  1/2 beta^T (G + 2 eta T) beta - c^T beta
 * (G, c, T, need as for slm_solve_l0).  q(S) depends on neither alpha nor the bound, so with Q_k = value_out[k] the table
 * answers best subset for every bound K' <= max_groups (min over k <= K' of Q_k) and RegularizedL0 / L2L0 for every
 * alpha >= alpha_min (min over k of Q_k + alpha k).  alpha_min > 0 prunes: below a node of cnt groups nothing is searched when
 * q_all + alpha_min (cnt + 1) >= min(0, min over k <= cnt of Q_k + alpha_min k), which no support strictly better at any
 * alpha >= alpha_min can lie behind -- the table then serves those alphas only, and its entries need not be the best of
 * their size.  The table is complete only for alpha_min = 0; the search then visits about as many nodes as there are
 * admissible supports of at most max_groups groups (meant for up to ~30 groups, or a small max_groups).
 * Outputs, max_groups + 1 entries each (a negative max_groups counts as 0): beta_out [(max_groups + 1) * p], row k the
 * coefficients of size k, recomputed once on the host from the Gram on its support; support_out[k]: bit i = group i active;
 * value_out[k] = Q_k.  Entry 0 is the empty support (value 0).  An entry nobody filled -- a size above the group count, one the
 * hierarchy admits no support of, one the pruning never reached -- holds +inf, an all-ones mask and zero coefficients.
 * *nodes_out: group inclusions tried.  info->n_iter = launches (1), info->L = q_all, info->mode = 4, info->kkt = the
 * regularised optimum at alpha_min, info->mu = the best-subset optimum at max_groups, info->status = SLM_OK or
 * SLM_ERR_NOT_CONVERGED; info->loss is not set.  Limits and argument errors are slm_solve_l0's: up to 64 columns and 64 groups
 * (SLM_ERR_UNSUPPORTED beyond, and on row-sharded datasets); negative or non-finite alpha_min / eta, negative big_M, a need
 * bit at or beyond the group count: SLM_ERR_BAD_ARG before anything is launched; SLM_ERR_NOT_CONVERGED with the table of
 * incumbents when the node budget ran out.  There is no l1 term here (L1L0's support value depends on its own eta) and no
 * linear constraints.
 */
int slm_solve_l0_profile(slm_dataset* ds, double alpha_min, int32_t max_groups, double eta, const double* T /* p*p or NULL */,
                         double big_M, const uint64_t* need /* n_groups masks or NULL */, int64_t max_nodes /* <=0: default */,
                         double* beta_out /* [(max_groups+1)*p] */, uint64_t* support_out /* [max_groups+1] */,
                         double* value_out /* [max_groups+1] */, int64_t* nodes_out, slm_point_info* info);

/*
 * (added under ABI 24: two new symbols beside slm_solve_l0 and slm_solve_l0_profile, no existing entry, structure or constant
 * changes, so the version stays 24 -- a caller that needs them looks the symbols up.)  The WIDE exact l0 search: the problems,
 * arguments, outputs and argument errors of slm_solve_l0 and slm_solve_l0_profile for up to 128 columns and 128 groups
 * (SLM_ERR_UNSUPPORTED beyond, with a message that names 128, and on row-sharded datasets), on the kernel's wide
 * instantiations (csrc/l0_kernels.hpp, template parameter WIDE).  Both run the wide kernel at ANY admissible size, narrow ones
 * included; a problem within slm_solve_l0's limits gives the same coefficients, support and objective, bit for bit, on either.
 * Every mask is two 64-bit words, the low one first (bit g of the 128-bit integer): need holds 2 words per group,
 * support_out 2 words (the profile: 2 per size, all ones in both on an entry nobody filled).  There is no wide l1 mode.
 * Capacity: the Cholesky factor keeps 64 rows, so a support holds at most 64 INDEPENDENT columns (columns that depend on
 * the included ones are skipped as always and do not count).  An include that would bring a 65th is refused and its subtree
 * is not searched.  With c_min the smallest number of groups held where that happened, every support left out has at least
 * c_min + 1 groups and a quadratic value >= q_all, so its objective is at least q_all + alpha (c_min + 1).
 * slm_solve_l0_wide: when no include was refused nothing differs from slm_solve_l0.  Otherwise *lower_bound_out =
 * min(objective, q_all + alpha (c_min + 1)) -- and q_all when the node budget ran out, as before -- and the call is proven
 * optimal (SLM_OK) iff the search finished and objective <= q_all + alpha (c_min + 1); if not it returns
 * SLM_ERR_NOT_CONVERGED with valid outputs, like an exhausted budget.  info->rejects = c_min + 1, or 0 when no include was
 * refused; info->resid = 1 when the node budget ran out, else 0; the other fields as for slm_solve_l0.  The greedy seed only
 * takes groups that fit the 64 rows.
 * slm_solve_l0_profile_wide: lane k - 1 keeps size k, so max_groups <= 64; and there is no dynamic rule -- the call is
 * refused with SLM_ERR_UNSUPPORTED (the message names 64) when the max_groups largest groups together hold more than 64
 * columns, so that no include can be refused and the table keeps its meaning.
 */
int slm_solve_l0_wide(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T /* p*p or NULL */,
                      double big_M, const uint64_t* need /* 2 words per group, low word first, or NULL */,
                      int64_t max_nodes /* <=0: default */, double* beta_out, uint64_t* support_out /* [2] */,
                      double* lower_bound_out, int64_t* nodes_out, slm_point_info* info);
int slm_solve_l0_profile_wide(slm_dataset* ds, double alpha_min, int32_t max_groups, double eta, const double* T /* p*p or NULL */,
                              double big_M, const uint64_t* need /* 2 words per group, low word first, or NULL */,
                              int64_t max_nodes /* <=0: default */, double* beta_out /* [(max_groups+1)*p] */,
                              uint64_t* support_out /* [(max_groups+1)*2] */, double* value_out /* [max_groups+1] */,
                              int64_t* nodes_out, slm_point_info* info);

/*
 * (added under ABI 24: two new symbols beside slm_solve_l0_l1 and slm_solve_l0_profile, no existing entry, structure or constant
 * changes, so the version stays 24 -- a caller that needs them looks the symbols up.)  The L1 PROFILE: the reference's L1L0 at
 * EVERY alpha from one search (csrc/l0_kernels.hpp, template parameters L1 and PROFILE together).  For one fixed eta_l1 the
 * value of a support,
 *       f(S) = min over beta, supp beta in cols(S), |beta_j| <= big_M, of  1/2 beta^T G beta - c^T beta + eta_l1 ||beta||_1,
 * depends on neither alpha nor the size, so with F_k = value_out[k] = min over admissible S of exactly k groups of f(S) the
 * table answers slm_solve_l0_l1(alpha, eta_l1) for every alpha >= alpha_min (min over k of F_k + alpha k) and, at
 * alpha_min = 0, the cardinality-bounded lasso for every bound K' <= max_groups.  There is no ridge term and no T, as in
 * slm_solve_l0_l1.  The search is the profile's: q(S) <= f(S) filters the candidates of each size, a candidate is valued by
 * the descent of slm_solve_l0_l1 over all columns of its support, and the subtree cut of slm_solve_l0_profile runs with the
 * proven lower bound on f(all columns) of slm_solve_l0_l1 in place of q_all (f is monotone in the support).  The lasso sets
 * coefficients to zero by itself, so the table saturates: from the size that holds every column the lasso on all columns
 * uses, larger sizes tie with it in value and the smaller mask is returned.  Outputs as slm_solve_l0_profile's (row k
 * recomputed on the host by the same descent and polished, as slm_solve_l0_l1 recomputes its winner); info as
 * slm_solve_l0_profile's with info->L = the l1 lower bound used and info->rejects = descents run.  eta_l1 == 0 runs the very
 * code of slm_solve_l0_profile(ds, alpha_min, max_groups, 0, NULL, ...).  Argument errors are those of slm_solve_l0_l1 and
 * slm_solve_l0_profile (SLM_ERR_BAD_ARG before anything is launched; SLM_ERR_UNSUPPORTED beyond the limits and on row-sharded
 * datasets; SLM_ERR_NOT_CONVERGED with the table of incumbents when the node budget ran out).
 * slm_solve_l0_l1_profile: up to 64 columns and 64 groups.  slm_solve_l0_l1_profile_wide: up to 128 columns and 128 groups,
 * masks of two words as in slm_solve_l0_profile_wide, and its two refusals: max_groups <= 64, and the max_groups largest
 * groups together hold at most 64 columns (the messages name 64) -- a support's columns, dependent ones included, then fit
 * the 64 lanes that hold them.  A problem within the narrow limits gives the same bytes on either.  Not here: a ridge term,
 * linear constraints, the exclusion bound.  Batches over row sets and l1 weights: slm_solve_l0_profile_grid (eta_kind 1).
 */
int slm_solve_l0_l1_profile(slm_dataset* ds, double alpha_min, int32_t max_groups, double eta_l1, double big_M,
                            const uint64_t* need /* n_groups masks or NULL */, int64_t max_nodes /* <=0: default */,
                            double* beta_out /* [(max_groups+1)*p] */, uint64_t* support_out /* [max_groups+1] */,
                            double* value_out /* [max_groups+1] */, int64_t* nodes_out, slm_point_info* info);
int slm_solve_l0_l1_profile_wide(slm_dataset* ds, double alpha_min, int32_t max_groups, double eta_l1, double big_M,
                                 const uint64_t* need /* 2 words per group, low word first, or NULL */,
                                 int64_t max_nodes /* <=0: default */, double* beta_out /* [(max_groups+1)*p] */,
                                 uint64_t* support_out /* [(max_groups+1)*2] */, double* value_out /* [max_groups+1] */,
                                 int64_t* nodes_out, slm_point_info* info);

/*
 * (added under ABI 24: a new symbol beside slm_solve_l0_profile, no existing entry, structure or constant changes, so the
 * version stays 24 -- a caller that needs it looks the symbol up.)  The BATCHED l0 profile: the tables of slm_solve_l0_profile
 * for `count` row sets of one dataset -- the training sets of a cross-validation and all rows, say -- from ONE launch
 * (csrc/l0_kernels.hpp, template parameter BATCH), one upload and one read-back.  1 <= count <= 16, what the dataset's Gram
 * store holds.  Row set b is (row_weights[b], n_effs[b]) as a lane of slm_solve_lanes brings them: n weights >= 0 and the
 * divisor of its Gram (<= 0: the dataset's row count); a NULL entry is the dataset's own rows and weights.  When every entry
 * is non-NULL the Grams come from one slm_dataset_covariance_folds call, otherwise from slm_dataset_covariance one by one.
 * intercept != 0: the dataset's LAST column is a column of ones, alone in the LAST group (SLM_ERR_BAD_ARG otherwise); it is
 * not searched but eliminated from every row set's Gram (G <- G - g1 g1^T / G11, c <- c - g1 c1 / G11), which is weighted
 * centring of X and y by that row set's own weighted means, and intercept_out[b][k] = ymean_b - xmean_b^T beta.  (The
 * elimination cancels where a column's |mean| is far above its spread: relative error about 2^-53 (1 + mean^2 / variance).)
 * ps, the number of search columns, is p, or p - 1 with an intercept; the search groups are the dataset's without the last
 * one then.  T (ps * ps), need (one mask per search group), alpha_min, max_groups, eta, big_M as for slm_solve_l0_profile
 * and shared by the problems; max_nodes is the budget of EACH problem.  Problems differ in their Gram alone, hence in search
 * order, q_all and seeds; each has its own tickets, node counter, stop word and incumbents, and a problem whose budget runs
 * out stops alone.  Outputs per problem b as slm_solve_l0_profile's: beta_out [count][max_groups + 1][ps], intercept_out
 * [count][max_groups + 1] (may be NULL; zeros without an intercept), support_out and value_out [count][max_groups + 1],
 * nodes_out [count] (may be NULL), info [count] (may be NULL), info[b].status = SLM_OK or SLM_ERR_NOT_CONVERGED.  Returns
 * SLM_OK iff every problem finished; SLM_ERR_NOT_CONVERGED with ALL outputs valid when any budget ran out.  Limits and
 * argument errors, all before a device is touched: count outside 1 .. 16, a negative or non-finite weight and those of
 * slm_solve_l0_profile (SLM_ERR_BAD_ARG); ps or the search groups above 64, a row-sharded dataset (SLM_ERR_UNSUPPORTED).
 * Not here: wide, constrained or exclusion-bound problems; batches over T.  An l1 term and several eta per call:
 * slm_solve_l0_profile_grid below, of which this entry is the call n_eta = 1, eta_kind = 0.
 */
int slm_solve_l0_profile_batch(slm_dataset* ds, int32_t count, const double* const* row_weights /* [count], entries may be NULL */,
                               const int64_t* n_effs /* [count] */, int32_t intercept, double alpha_min, int32_t max_groups,
                               double eta, const double* T /* ps*ps or NULL */, double big_M,
                               const uint64_t* need /* search-group masks or NULL */, int64_t max_nodes /* per problem; <=0: default */,
                               double* beta_out /* [count][max_groups+1][ps] */, double* intercept_out /* [count][max_groups+1] or NULL */,
                               uint64_t* support_out /* [count][max_groups+1] */, double* value_out /* [count][max_groups+1] */,
                               int64_t* nodes_out /* [count] or NULL */, slm_point_info* info /* [count] or NULL */);

/*
 * (added under ABI 24: a new symbol beside slm_solve_l0_profile_batch, no existing entry, structure or constant changes, so the
 * version stays 24 -- a caller that needs it looks the symbol up.)  The l0 profile GRID: the tables of slm_solve_l0_profile
 * (eta_kind 0) or of slm_solve_l0_l1_profile (eta_kind 1) for `count` row sets of one dataset at n_eta weights each -- a
 * cross-validation of L2L0 or L1L0 over (alpha, eta) -- from ONE launch (csrc/l0_kernels.hpp, template parameter BATCH, with
 * L1 for eta_kind 1), one upload, one Gram per row set and one read-back.  Row sets (row_weights, n_effs, NULL entries,
 * 1 <= count <= 16) and intercept exactly as for slm_solve_l0_profile_batch.  Problem b = r * n_eta + e is row set r with
 * etas[e]:  eta_kind 0: H = G_r + 2 etas[e] T, the problem of slm_solve_l0_profile;  eta_kind 1: H = G_r and etas[e] weighs
 * ||beta||_1, the problem of slm_solve_l0_l1_profile, T must be NULL (an l1 weight of exactly 0 is searched by the l1 kernel
 * with weight 0 and valued on the host as slm_solve_l0_profile values it).  Every output has the leading dimension
 * count * n_eta in that order and holds per problem what the entry it replaces gives: with eta_kind 1 the rows are recomputed
 * by the descent and polished, info[b].L is the l1 lower bound the cut used and info[b].rejects the number of descents.
 * alpha_min, max_groups, T, big_M and need are shared; max_nodes is the budget of EACH problem, a starved problem stops alone.
 * Returns SLM_OK iff every problem finished, SLM_ERR_NOT_CONVERGED with ALL outputs valid otherwise.
 * Size: count * n_eta <= SLM_L0_GRID_MAX = 128 problems.  Each problem gets max(1, 2 CUs / problems) workgroups, so on a device
 * of at least 64 CUs the grid is resident at once.  On a smaller device the call still RUNS: every problem keeps one workgroup,
 * the grid exceeds what the device holds and the surplus workgroups start as others leave -- no workgroup waits on another.
 * Refusals, all before a device is touched: those of slm_solve_l0_profile_batch and of the entry the kind generalises;
 * n_eta < 1, a negative or non-finite etas[e], eta_kind outside {0, 1}, T with eta_kind 1, count * n_eta above the cap (the
 * message names it) (SLM_ERR_BAD_ARG); more than 64 search columns or groups, a row-sharded dataset (SLM_ERR_UNSUPPORTED).
 * Not here: wide, constrained or exclusion-bound problems, a ridge term beside the l1 term, several T.
 */
#define SLM_L0_GRID_MAX 128
int slm_solve_l0_profile_grid(slm_dataset* ds, int32_t count, const double* const* row_weights /* [count], entries may be NULL */,
                              const int64_t* n_effs /* [count] */, int32_t intercept, int32_t n_eta, const double* etas /* [n_eta] */,
                              int32_t eta_kind /* 0 ridge, 1 l1 */, double alpha_min, int32_t max_groups,
                              const double* T /* ps*ps or NULL; NULL with eta_kind 1 */, double big_M,
                              const uint64_t* need /* search-group masks or NULL */, int64_t max_nodes /* per problem; <=0: default */,
                              double* beta_out /* [count*n_eta][max_groups+1][ps] */,
                              double* intercept_out /* [count*n_eta][max_groups+1] or NULL */,
                              uint64_t* support_out /* [count*n_eta][max_groups+1] */, double* value_out /* [count*n_eta][max_groups+1] */,
                              int64_t* nodes_out /* [count*n_eta] or NULL */, slm_point_info* info /* [count*n_eta] or NULL */);

/*
 * (added under ABI 24: two new symbols beside the exact l0 entries, no existing entry, structure or constant changes, so the
 * version stays 24 -- a caller that needs them looks the symbols up.)  The l0 LOCAL SEARCH (csrc/l0_local_kernels.hpp): an
 * APPROXIMATE answer to the regularised l0 problem for up to SLM_L0_LOCAL_PMAX = 1024 columns, where every entry above
 * stops at 128.  It proves nothing: no lower bound comes back, and SLM_OK means "reached its fixed point", never "optimal".
 * For cell e, with G = X^T W X / n_eff, c = X^T W y / n_eff and H = G + 2 etas[e] I,
 *       minimise over beta, |beta_j| <= big_M:   F(beta) = 1/2 beta^T H beta - c^T beta + alphas[e] ||beta||_0
 * -- the units of slm_solve_l0's objective with singleton groups and T = I.  The rule (Hazimeh and Mazumder 2020, "Fast best
 * subset selection: coordinate descent and local combinatorial optimization"): with r = c - H beta and d_j = H_jj, coordinate
 * j given the others has u = r_j + d_j beta_j, b = clip(u / d_j, +-big_M), gain = u b - 1/2 d_j b^2.
 *   1. Descent: j = 0 .. p-1 cyclically, beta_j <- b if gain > alphas[e] (strictly), else 0; a column with
 *      d_j <= 1e-12 max_k d_k stays 0.  A sweep ends the descent when no coordinate entered or left the support and
 *      max_j |delta_j| sqrt(d_j) <= 1e-12 sqrt(yy); 10000 sweeps end it unconverged.
 *   2. Swap scan: for i in the support, ascending, with i removed: g_i = gain(i) and g_j the best gain over j outside the
 *      support (ties: the lowest j); if g_j > g_i + 1e-10 max(|g_i|, alphas[e]), i leaves, j enters at its b, and the rule
 *      returns to 1.  When no i swaps the problem is done; 10000 swaps end it unconverged.
 * Every accepted step lowers F.  slm_solve_l0_local_descent is the same call without step 2: every problem ends at its
 * descent's fixed point, whose F is never below the full rule's from the same start.
 * One launch runs n_cells * n_starts problems, one wavefront each: cell e from starts[(e * n_starts + s) * p ..] (each inside
 * the box; NULL with n_starts = 1: the zero start).  The kernel reads the Gram that slm_dataset_covariance files with the
 * dataset, in place.  Per cell the start with the lowest F wins (ties: the lowest index; start_out, may be NULL), and the
 * host re-solves the winner's support exactly inside the box: beta_out[e] is the minimiser on its support and
 * objective_out[e] its F.  info[e] (may be NULL): status = SLM_OK or SLM_ERR_NOT_CONVERGED (a cap ended the winner), n_iter =
 * its sweeps, rejects = its accepted swaps, resid = its status word (1: a descent ran out of sweeps, 2: the swap cap), mu =
 * its objective before the polish, kkt = the objective after it, loss, beta_norm = ||beta||_2, L = -inf (no bound), mode = 8.
 * Returns SLM_OK, or SLM_ERR_NOT_CONVERGED with ALL outputs valid when some cell's winner reached a cap.
 * Refusals, all before a device is touched, each with its own message: p > 1024, groups that are not singletons, a
 * row-sharded dataset (SLM_ERR_UNSUPPORTED); a negative or non-finite alphas[e] or etas[e], big_M < 0, n_cells < 1,
 * n_starts < 1, n_cells * n_starts > SLM_L0_LOCAL_MAX_PROBLEMS = 8192, a start outside the box (SLM_ERR_BAD_ARG).
 * Not here: groups and a hierarchy, an l1 term, a Tikhonov matrix, constraints.  Row sets (CV folds) in the launch:
 * slm_solve_l0_local_folds, below; a bound on the cardinality: slm_solve_l0_local_subsets, below.  (Groups and a hierarchy:
 * slm_solve_l0_local_groups, below.  An l1 term: slm_solve_l0_local_l1, below.)
 */
#define SLM_L0_LOCAL_PMAX 1024
#define SLM_L0_LOCAL_MAX_PROBLEMS 8192
int slm_solve_l0_local(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas /* [n_cells] each */,
                       double big_M, int32_t n_starts, const double* starts /* n_cells * n_starts * p, or NULL: one zero start */,
                       double* beta_out /* n_cells * p */, double* objective_out /* n_cells */, int32_t* start_out /* winning start */,
                       slm_point_info* info /* n_cells */);
int slm_solve_l0_local_descent(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas, double big_M,
                               int32_t n_starts, const double* starts, double* beta_out, double* objective_out, int32_t* start_out,
                               slm_point_info* info);

/*
 * (added under ABI 24: a new symbol beside slm_solve_l0_local, no existing entry, structure or constant changes, so the version
 * stays 24 -- a caller that needs it looks the symbol up.)  The l0 local search on `count` ROW SETS of one dataset -- the
 * training rows of a cross-validation's folds and all rows -- from ONE launch.  Row sets (row_weights, n_effs, NULL entries,
 * 1 <= count <= 16) and intercept exactly as for slm_solve_l0_profile_batch: with intercept != 0 the dataset is [X | 1], the
 * ones column last and alone in the last group; it is not searched but eliminated from every row set's Gram (the Schur
 * complement: weighted centring of X and y by the row set's own means), so ps = p - 1 columns are searched and the dataset may
 * hold SLM_L0_LOCAL_PMAX + 1 = 1025; else ps = p.  The Grams come from one slm_dataset_covariance_folds call when every entry
 * of row_weights is given, else from one slm_dataset_covariance call per row set; they are found again by fingerprint and
 * never modified (the eliminated copies live in a workspace of the call, count * ps * ld doubles; without an intercept the
 * kernel reads the store in place).  Problem (r * n_cells + e) * n_starts + s is row set r, cell e (alphas[e], etas[e]:
 * shared by the row sets), start s; starts and stat_out are in that order, every other output is [r * n_cells + e].
 * swaps == 0: without the swap scan, as slm_solve_l0_local_descent.  Per (row set, cell) the winner among the starts, its
 * polish (on the eliminated Gram when there is an intercept) and info follow slm_solve_l0_local;
 * intercept_out = ymean_r - xmean_r^T beta (0 without an intercept).  stat_out (may be NULL): sweeps, accepted swaps, status
 * word and non-zeros of EVERY problem, the losing starts included.  With count = 1, row_weights[0] = NULL and no intercept
 * every output equals slm_solve_l0_local's (swaps == 0: _descent's) byte for byte.
 * Returns SLM_OK, or SLM_ERR_NOT_CONVERGED with ALL outputs valid when some winner reached a cap.
 * Refusals, all before a device is touched, each with its own message: those of slm_solve_l0_local (the width counts ps);
 * count outside 1 .. 16, a negative or non-finite weight, an intercept column that is not last and alone (SLM_ERR_BAD_ARG);
 * count * n_cells * n_starts > SLM_L0_LOCAL_MAX_PROBLEMS (the message names the three factors).  A row set that gives the
 * ones column no weight is refused once its Gram is there.
 * Not here: groups, an l1 term, more than 16 row sets.  (A bound on the cardinality: slm_solve_l0_local_subsets.)
 * (Groups and a hierarchy: slm_solve_l0_local_groups.  An l1 term: slm_solve_l0_local_l1.)
 */
int slm_solve_l0_local_folds(slm_dataset* ds, int32_t count, const double* const* row_weights /* [count], entries may be NULL */,
                             const int64_t* n_effs /* [count] */, int32_t intercept, int32_t n_cells, const double* alphas,
                             const double* etas /* [n_cells] each */, double big_M, int32_t n_starts,
                             const double* starts /* count * n_cells * n_starts * ps, or NULL: one zero start */, int32_t swaps,
                             double* beta_out /* count * n_cells * ps */, double* intercept_out /* count * n_cells, or NULL */,
                             double* objective_out /* count * n_cells */, int32_t* start_out /* or NULL */,
                             int32_t* stat_out /* count * n_cells * n_starts * 4: sweeps, swaps, status word, non-zeros of EVERY problem; or NULL */,
                             slm_point_info* info /* count * n_cells, or NULL */);

/*
 * (added under ABI 24: a new symbol beside slm_solve_l0_local_folds, no existing entry, structure or constant changes, so the
 * version stays 24 -- a caller that needs it looks the symbol up.)  LOCAL SUBSETS: the l0 local search in its CARDINALITY form,
 * the approximate twin of slm_solve_l0_profile beyond 128 columns (up to SLM_L0_LOCAL_PMAX = 1024).  Cell e is
 * (sizes[e], etas[e]); with G, c as above and H = G + 2 etas[e] I,
 *       minimise over beta, |beta_j| <= big_M, ||beta||_0 <= sizes[e]:   Q(beta) = 1/2 beta^T H beta - c^T beta
 * -- the units of slm_solve_l0's objective with alpha = 0, singleton groups and T = I.  Nothing is proven.  The rule, with
 * r, d, u, b and gain as for slm_solve_l0_local and tol = 1e-12 sqrt(yy), from a start of ANY support size inside the box:
 *   1. Shrink: while nnz > k, the support column with the smallest g_i = gain(r_i + d_i beta_i, d_i) leaves (ties: the lowest
 *      index).
 *   2. Descent on the support: j over the support cyclically, beta_j <- b; no threshold, no column enters, a coordinate whose
 *      b is exactly 0 leaves.  A sweep ends it when the support stood still and max |delta_j| sqrt(d_j) <= tol; 10000 sweeps
 *      end it unconverged.  A column with d_j <= 1e-12 max d stays out throughout.
 *   3. Grow: if nnz < k, the outside column with the largest gain(r_j, d_j) (ties: the lowest j) enters at its b when
 *      |b| sqrt(d_j) > tol; back to 2.
 *   4. Swap scan, once 3 adds nothing: step 2 of slm_solve_l0_local with alpha = 0; a swap goes back to 2, no swap ends the
 *      problem, 10000 accepted swaps end it unconverged.  swaps == 0 stops after 3: greedy forward selection with re-fitting.
 * Every accepted move lowers Q, apart from 1, which is forced.  A size above ps is legal: the problem ends when nothing more
 * enters.  Row sets, intercept, starts, problem order, the winner per (row set, cell) by (Q, then the lowest start), its polish
 * and info exactly as for slm_solve_l0_local_folds (info: mu = Q before the polish, kkt = objective_out = Q after it);
 * count = 1 with row_weights[0] = NULL and no intercept is the plain single-dataset call.  stat_out (may be NULL): SIX ints per
 * problem -- sweeps, accepted swaps, status word, non-zeros, grows (entries in 3), drops (exits in 1 and 2).
 * Returns SLM_OK, or SLM_ERR_NOT_CONVERGED with ALL outputs valid when some winner reached a cap.
 * Refusals, all before a device is touched, in this order: NULL sizes or etas; a size < 1; a negative or non-finite eta; then
 * those of slm_solve_l0_local_folds for the row sets, the problem counts, big_M, the width, the intercept column, the weights
 * and the box of the starts.
 * Not here: groups, hierarchy, Tikhonov matrix, l1 term, constraints.  (Groups and a hierarchy in the penalised form:
 * slm_solve_l0_local_groups, below; an l1 term in the penalised form: slm_solve_l0_local_l1, below.)
 */
int slm_solve_l0_local_subsets(slm_dataset* ds, int32_t count, const double* const* row_weights /* [count], entries may be NULL */,
                               const int64_t* n_effs /* [count] */, int32_t intercept, int32_t n_cells, const int32_t* sizes,
                               const double* etas /* [n_cells] each */, double big_M, int32_t n_starts,
                               const double* starts /* count * n_cells * n_starts * ps, or NULL: one zero start */, int32_t swaps,
                               double* beta_out /* count * n_cells * ps */, double* intercept_out /* count * n_cells, or NULL */,
                               double* objective_out /* count * n_cells */, int32_t* start_out /* or NULL */,
                               int32_t* stat_out /* count * n_cells * n_starts * 6, or NULL */, slm_point_info* info /* count * n_cells, or NULL */);

/*
 * (added under ABI 24: a new symbol beside slm_solve_l0_local_folds, no existing entry, structure or constant changes, so the
 * version stays 24 -- a caller that needs it looks the symbol up.)  LOCAL SEARCH WITH GROUPS AND A HIERARCHY
 * (csrc/l0_local_group_kernels.hpp): what the three entries above refuse.  The groups are the dataset's
 * (slm_dataset_set_groups) and must be CONTIGUOUS and ASCENDING in column order -- the group index starts at 0 and rises by 0
 * or 1 from a column to the next; the caller orders the columns.  need_ptr / need_idx: the hierarchy as a CSR list of the groups
 * each search group needs directly (need_ptr NULL: none); the host closes it transitively, a group is never in its own closed
 * list, so cycles are legal.  For cell e, with G, c as for slm_solve_l0_local and H = G + 2 etas[e] I,
 *       minimise over beta, |beta_j| <= big_M:   F(beta) = 1/2 beta^T H beta - c^T beta + alphas[e] |cl(S(beta))|
 * S(beta) the groups that hold a non-zero coefficient, cl its closure under the hierarchy: slm_solve_l0's objective with
 * max_groups = n_groups and T = I; with singleton groups and no hierarchy slm_solve_l0_local's F, and its rule.  NOTHING IS
 * PROVEN.  The rule, with r, d, b, gain and tol as for slm_solve_l0_local; per group nz_g (non-zero coefficients), held_g (the
 * groups h != g with nz_h > 0 that need g), z_g = (nz_g > 0 or held_g > 0), and the price of a group that is empty or has just
 * been emptied, m_g = [held_g == 0] (1 + #{h in need*(g): nz_h == 0 and held_h == 0}), what entering adds to |cl(S)|:
 *   1. Group descent, g = 0 .. n_groups-1 cyclically.  A group with z_g = 1 gets a step, an inactive one only when it passes the
 *      screen C_g = sum_{j in g, d_j > 0} gain(r_j, d_j) > alpha m_g / 4.  THE SCREEN IS A HEURISTIC: a block's gain has no bound
 *      in terms of its coordinates' gains, so it can miss a group that would have paid.  The step: up to 8 passes beta_j <- b_j
 *      over the group's columns (ascending, no threshold; d_j <= 1e-12 max d stays 0), ended by a pass with
 *      max |delta| sqrt(d) <= tol; then v_g = 1/2 beta_g^T (r_g + r'_g), r' = r + sum_{j in g} H[:, j] beta_j; the group is kept iff
 *      v_g > alpha m_g (strictly), else beta_g <- 0 and r <- r'.  A sweep ends the descent when no group entered or left and
 *      max |delta| sqrt(d) <= tol over the kept steps; 10000 sweeps end it unconverged.
 *   2. Group swap scan (swaps != 0): i ascending over the groups with nz_i > 0 and held_i == 0.  With i removed (v_i, m_i), the
 *      candidate j is the empty group other than i with the largest C_j - alpha m_j (ties: the lowest j); it is fitted from zero
 *      by the inner passes (v_j); if v_j - alpha m_j > v_i - alpha m_i + 1e-10 max(|v_i|, alpha) the swap stands and the rule
 *      returns to 1, else beta and r are restored exactly.  No swap ends the problem; 10000 accepted swaps end it unconverged.
 * A start may have any support, closed or not.  Every accepted move lowers F.  Row sets, intercept (the ones column last and
 * alone in the last group: it and its group are not searched, so need_ptr has (groups - 1) + 1 entries), starts, problem order
 * and the winner per (row set, cell) by (F, then the lowest start) as for slm_solve_l0_local_folds.  The winner is re-solved
 * exactly inside the box on ALL columns of the groups in cl(S) (a group that is only held is free to use);
 * objective_out = quad + alphas[e] |cl(S)| of the coefficients that go back; group_support_out (may be NULL): cl(S), one int per
 * search group.  stat_out (may be NULL): SIX ints per problem -- sweeps, accepted swaps, status word, |cl(S)|, non-zero columns,
 * group trials (fits of a group that was not in cl(S), and of swap candidates).  info as for slm_solve_l0_local_folds, mode = 9.
 * Returns SLM_OK, or SLM_ERR_NOT_CONVERGED with ALL outputs valid when some winner reached a cap.
 * Refusals, all before a device is touched, each with its own message: those of slm_solve_l0_local_folds except the one about
 * groups; groups that are not contiguous or not ascending (SLM_ERR_UNSUPPORTED: the caller must order the columns); a need_ptr
 * that does not start at 0 or falls, a need_idx outside the search groups (SLM_ERR_BAD_ARG); a row-sharded dataset.
 * Not here: groups in the cardinality form, an l1 term beside groups (without groups: slm_solve_l0_local_l1, below), a Tikhonov
 * matrix, constraints, seeding the exact search.
 */
int slm_solve_l0_local_groups(slm_dataset* ds, int32_t count, const double* const* row_weights /* [count], entries may be NULL */,
                              const int64_t* n_effs /* [count] */, int32_t intercept, int32_t n_cells, const double* alphas,
                              const double* etas /* [n_cells] each */, double big_M,
                              const int32_t* need_ptr /* search groups + 1, or NULL */, const int32_t* need_idx, int32_t n_starts,
                              const double* starts /* count * n_cells * n_starts * ps, or NULL: one zero start */, int32_t swaps,
                              double* beta_out /* count * n_cells * ps */, double* intercept_out /* count * n_cells, or NULL */,
                              double* objective_out /* count * n_cells */, int32_t* start_out /* or NULL */,
                              int32_t* group_support_out /* count * n_cells * search groups, or NULL: cl(S) */,
                              int32_t* stat_out /* 6 per problem: sweeps, swaps, status word, |cl(S)|, non-zero columns, group trials; or NULL */,
                              slm_point_info* info /* count * n_cells, or NULL */);

/*
 * (added under ABI 24: a new symbol beside slm_solve_l0_local_folds, no existing entry, structure or constant changes, so the
 * version stays 24 -- a caller that needs it looks the symbol up.)  LOCAL SEARCH WITH AN L1 TERM (l0_local_l1_kernel,
 * csrc/l0_local_kernels.hpp): the approximate answer to slm_solve_l0_l1 (the reference's L1L0) beyond its 64 columns, up to
 * SLM_L0_LOCAL_PMAX = 1024.  Cell e is (alphas[e], l1s[e], ridges[e]); with G, c as for slm_solve_l0_local and
 * H = G + 2 ridges[e] I,
 *       minimise over beta, |beta_j| <= big_M:   F(beta) = 1/2 beta^T H beta - c^T beta + l1s[e] ||beta||_1 + alphas[e] ||beta||_0
 * -- with ridges[e] = 0 the units of slm_solve_l0_l1's objective (eta_l1 = l1s[e]) with singleton groups.  NOTHING IS PROVEN.
 * The rule is slm_solve_l0_local's with ONE change, the coordinate: with lam = l1s[e], u = r_j + d_j beta_j,
 *       s = sign(u) max(|u| - lam, 0),   b = clip(s / d_j, +-big_M),   gain = u b - 1/2 d_j b^2 - lam |b|
 * (what F without the alpha term falls by when beta_j goes from 0 to b).  The descent keeps b iff gain > alphas[e]; the swap scan
 * compares these gains by the same rule; dead columns, the stopping rules and both caps are unchanged.  With l1s[e] = 0 every
 * decision is slm_solve_l0_local_folds's (the objectives agree to rounding, not byte for byte: a multiply-add may contract
 * otherwise).  Row sets, intercept, starts, problem order, the winner per (row set, cell) by (F, then the lowest start), stat_out
 * (FOUR ints per problem) and info exactly as for slm_solve_l0_local_folds, mode = 10.  The winner is polished on the rows of
 * its support alone: the soft-threshold descent to its last digit, then the exact solve on its sign pattern
 * (H_FF x = c_F - lam sign(b_F) - H_FB b_B: free F, bound B), taken only when every sign and the box hold; a coefficient the
 * polish brings to zero goes back as zero, objective_out is F of the coefficients that go back (alpha on THEIR non-zeros), and
 * the polish never raises F.
 * Returns SLM_OK, or SLM_ERR_NOT_CONVERGED with ALL outputs valid when some winner reached a cap.
 * Refusals, all before a device is touched, in this order: NULL alphas or l1s; a negative or non-finite l1s[e]; a negative or
 * non-finite ridges[e] where ridges is given; then those of slm_solve_l0_local_folds, in its order.
 * Not here: groups or a hierarchy with the l1 term, the cardinality form with it, a Tikhonov matrix, constraints, seeding the
 * exact search, more than 16 row sets.
 */
int slm_solve_l0_local_l1(slm_dataset* ds, int32_t count, const double* const* row_weights /* [count], entries may be NULL */,
                          const int64_t* n_effs /* [count] */, int32_t intercept, int32_t n_cells, const double* alphas,
                          const double* l1s /* [n_cells] each */, const double* ridges /* [n_cells] or NULL: 0 */, double big_M,
                          int32_t n_starts, const double* starts /* count * n_cells * n_starts * ps, or NULL: one zero start */,
                          int32_t swaps, double* beta_out /* count * n_cells * ps */, double* intercept_out /* count * n_cells, or NULL */,
                          double* objective_out /* count * n_cells */, int32_t* start_out /* or NULL */,
                          int32_t* stat_out /* 4 words per problem: sweeps, swaps, status word, non-zeros (or NULL) */,
                          slm_point_info* info /* count * n_cells, or NULL */);

/*
 * (added under ABI 24: a new symbol beside slm_solve_l0_local, no existing entry, structure or constant changes, so the version
 * stays 24 -- a caller that needs it looks the symbol up.)  LOCAL BOUND (l0_local_bound_kernel, csrc/l0_local_bound_kernels.hpp):
 * the half slm_solve_l0_local lacks -- for every cell e = (alphas[e], etas[e]) a PROVEN LOWER BOUND on the objective that entry
 * minimises, for up to SLM_L0_LOCAL_PMAX = 1024 columns, one wavefront per cell, one launch.  With G, c as for
 * slm_solve_l0_local and the box |beta_j| <= big_M,
 *       F(beta) = 1/2 beta^T (G + 2 etas[e] I) beta - c^T beta + alphas[e] ||beta||_0.
 * The indicator is relaxed by the perspective of the ridge term with the big-M link; that leaves a separable convex penalty phi
 * whose conjugate is phi*(t) = max(0, h(t) - alpha), h(t) = t^2 / (4 eta) for |t| <= 2 eta M, else |t| M - eta M^2 (eta = 0:
 * |t| M).  For EVERY vector u, with t = c - G u (the plain G),
 *       L(u) = -1/2 u^T G u - sum over all p columns of max(0, h(t_j) - alpha)   <=   min F:
 * IT IS A BOUND FOR EVERY u.  The kernel looks for the u that makes it tightest, the minimiser of the relaxation
 * P(b) = 1/2 b^T G b - c^T b + sum phi(b_j), by cyclic coordinate descent from starts[e] (clipped into the box; NULL: zero),
 * stops a cell when P - L <= gap_tol max(|P|, alphas[e]) or after max_sweeps sweeps (<= 0: 10000), rebuilds t from u alone and
 * writes lower_out[e] = max(L(u), L(0)), primal_out[e] = P(u), u_out[e] = u, stat_out[2e] = sweeps, stat_out[2e + 1] = the
 * status word (1: the sweeps ran out before the gap closed).  The values are bounds WHATEVER the status: the status says only
 * whether the relaxation was closed.  A column whose G_jj <= 1e-12 max G_kk keeps u_j = 0 and is still counted in the sum.
 * WHERE IT IS WEAK: the bound is tight with a ridge (eta > 0) or a box that binds, and weak at eta = 0 under a loose big_M,
 * where phi is (alpha / big_M) |b|, next to nothing (DESIGN 4d "Local bound" has the measured gaps).  big_M = 0: lower = 0
 * without a launch.  info[e]: L = lower_out[e], mu = primal_out[e], kkt = mu - L, n_iter = sweeps, resid = the status word,
 * mode = 11.
 * Returns SLM_OK, or SLM_ERR_NOT_CONVERGED with ALL outputs valid when a cell ran out of sweeps.
 * Refusals, all before a device is touched, each with its own message, in this order: NULL ds, alphas, etas or lower_out;
 * n_cells < 1; n_cells > SLM_L0_LOCAL_MAX_PROBLEMS; big_M < 0; a negative or non-finite alphas[e] or etas[e]; gap_tol < 0
 * (SLM_ERR_BAD_ARG); more than 1024 columns (SLM_ERR_UNSUPPORTED); a non-finite start (SLM_ERR_BAD_ARG); groups that are not
 * singletons; a row-sharded dataset (SLM_ERR_UNSUPPORTED).
 * Not here: groups and a hierarchy, the cardinality form, the l1 entry, row sets (folds), a Tikhonov matrix, strengthening
 * eta = 0 by extracting a diagonal from G, using the bound to prune or to seed the exact search.
 */
int slm_solve_l0_local_bound(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas /* [n_cells] each */,
                             double big_M, const double* starts /* n_cells * p, or NULL */, int32_t max_sweeps /* <=0: default */,
                             double gap_tol /* <0: BAD_ARG; 0: run to max_sweeps */, double* lower_out /* n_cells */,
                             double* primal_out /* n_cells, or NULL */, double* u_out /* n_cells * p, or NULL */,
                             int32_t* stat_out /* n_cells * 2: sweeps, status word; or NULL */, slm_point_info* info /* n_cells or NULL */);

/*
 * (added under ABI 24: two new symbols beside slm_solve_l0_local_bound, no existing entry, structure or constant changes, so the
 * version stays 24 -- a caller that needs them looks the symbols up.)  LOCAL PROOF (l0_local_node_kernel,
 * csrc/l0_local_node_kernels.hpp; the tree: l0_prove_tree, csrc/l0_host.hpp): branch and bound on the local bound, which turns
 * "within 25 %" into PROVEN OPTIMAL where the tree closes.  A NODE gives every column one of three states -- FREE, IN (the column
 * pays alphas[e] whether its coefficient is zero or not) or OUT (beta_j = 0) -- as two masks of 16 words of 64 bits each: bit
 * (j & 63) of word (j >> 6) is column j.  With G, c, F and h as for slm_solve_l0_local_bound and t = c - G u, for EVERY vector u
 *       L_node(u) = -1/2 u^T G u - sum over FREE of max(0, h(t_j) - alpha) - sum over IN of (h(t_j) - alpha)
 *                <=  min { F(beta) : |beta_j| <= big_M, beta_OUT = 0, IN columns pay alpha whether zero or not }.
 * slm_solve_l0_local_nodes bounds ONE BATCH of n_nodes <= 8192 nodes in one launch, one wavefront per node; node i belongs to
 * cell cell[i] of the call's n_cells cells, starts from starts[i] (clipped into the box; NULL: zero) and writes
 * lower_out[i] = max(L_node(u), L_node(0), parent_lower[i]) (parent_lower NULL: none), primal_out[i] = P_node(u), the relaxation's
 * value, upper_out[i] = F(u) = 1/2 u^T (G + 2 eta I) u - c^T u + alpha nnz(u), an upper bound of the cell because u lies in the
 * box, u_out[i] = u and stat_out[2i], stat_out[2i + 1] = sweeps and the status word (1: the sweeps ran out; the values are bounds
 * all the same).  A node stops at P - L <= gap_tol max(|P|, alpha) or after max_sweeps sweeps (<= 0: 10000).  info[i]: L =
 * lower, mu = primal, kkt = upper, n_iter = sweeps, resid = the status word, mode = 12.  Returns SLM_OK, or
 * SLM_ERR_NOT_CONVERGED with ALL outputs valid when a node ran out of sweeps.  Refusals, all before a device is touched, each
 * with its own message, in this order: NULL ds, alphas, etas, cell, a mask or lower_out; n_cells < 1; n_cells > 8192; n_nodes
 * < 1; n_nodes > 8192; big_M < 0; a negative or non-finite alphas[e] or etas[e]; gap_tol < 0 (SLM_ERR_BAD_ARG); more than 1024
 * columns (SLM_ERR_UNSUPPORTED); a cell[i] outside the call's cells; a column both IN and OUT; a parent_lower[i] that is a NaN or
 * +infinity (-infinity is "none"); a non-finite start (SLM_ERR_BAD_ARG); groups that are not singletons; a row-sharded dataset (SLM_ERR_UNSUPPORTED).  big_M = 0: everything zero
 * without a launch.
 */
int slm_solve_l0_local_nodes(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas /* [n_cells] each */,
                             double big_M, int32_t n_nodes, const int32_t* cell /* n_nodes */, const uint64_t* in_mask /* n_nodes * 16 */,
                             const uint64_t* out_mask /* n_nodes * 16 */, const double* parent_lower /* n_nodes, or NULL */,
                             const double* starts /* n_nodes * p, or NULL */, int32_t max_sweeps /* <=0: default */,
                             double gap_tol /* <0: BAD_ARG */, double* lower_out /* n_nodes */, double* primal_out /* n_nodes, or NULL */,
                             double* upper_out /* n_nodes, or NULL */, double* u_out /* n_nodes * p, or NULL */,
                             int32_t* stat_out /* n_nodes * 2, or NULL */, slm_point_info* info /* n_nodes or NULL */);

/*
 * (ABI 24, see above.)  slm_solve_l0_local_prove grows THE WHOLE TREE for every cell of a grid.  Per cell: the incumbent is
 * incumbents[e] (NULL, or a value not below 0: the empty support at 0); the root has empty masks; a round pops the `width` open
 * nodes of lowest bound and splits each into an IN child and an OUT child on the FREE column whose z_j = min(|u_j| / tauc, 1) is
 * closest to 1/2 (ties: the lowest index; where every z_j is 0 or 1, the largest |u_j|, then the largest |t_j|), both started
 * from the parent's u; the children of ALL cells of a round are ONE launch of at most 8192 nodes.  A child whose F(u) is below
 * the incumbent replaces it, polished on its support where that is lower still.  A node is dropped when best - lower <= rel_gap
 * max(|best|, alpha).  Node relaxations run at gap_tol = rel_gap / 100 and max_sweeps (<= 0: 10000).  A cell ends status_out[e]
 * = 0, PROVEN OPTIMAL to rel_gap, when no node is open, and 1 at max_nodes bound evaluations; either way lower_out[e] = min(best,
 * the lowest open bound) is proven.  beta_out[e], objective_out[e]: the incumbent; nodes_out[e], rounds_out[e]: bound
 * evaluations and launches the cell took part in.  The certificate, where leaf_capacity > 0 and the five leaf arrays are given:
 * every dropped node's cell, two masks, u and bound, the first leaf_capacity of them; *leaf_count counts them all.  info[e]: kkt
 * = mu = the objective, L = the proven bound, n_iter = rounds, rejects = nodes, resid = the status, mode = 13.
 * WHERE THE TREE CLOSES: with a ridge (eta > 0) or a box that binds; at eta = 0 with more columns than rows it does not, and the
 * call returns the proven gap it reached.  Returns SLM_OK, or SLM_ERR_NOT_CONVERGED with ALL outputs valid when a cell hit
 * max_nodes.  Refusals, all before a device is touched, each with its own message, in this order: NULL ds, alphas, etas, beta_out,
 * objective_out or lower_out; n_cells < 1; n_cells > 8192; big_M < 0; a negative or non-finite alphas[e] or etas[e]; rel_gap
 * outside [1e-10, 1]; max_nodes < 1; width < 1 (SLM_ERR_BAD_ARG); more than 1024 columns (SLM_ERR_UNSUPPORTED); an incumbent
 * outside the box or non-finite (SLM_ERR_BAD_ARG); groups that are not singletons; a row-sharded dataset (SLM_ERR_UNSUPPORTED).
 * big_M = 0: no launch, everything zero, proven.
 * Not here: groups and a hierarchy (slm_solve_l0_local_group_prove, below), the cardinality form, the l1 entry, row sets (folds), a Tikhonov matrix, strengthening
 * eta = 0 by extracting a diagonal from G, feeding the bound into the exact search over supports.
 */
int slm_solve_l0_local_prove(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas /* [n_cells] each */,
                             double big_M, const double* incumbents /* n_cells * p, or NULL */, double rel_gap, int32_t max_nodes,
                             int32_t width, int32_t max_sweeps /* <=0: default */, int64_t leaf_capacity /* 0: no certificate */,
                             double* beta_out /* n_cells * p */, double* objective_out /* n_cells */, double* lower_out /* n_cells */,
                             int32_t* nodes_out, int32_t* rounds_out, int32_t* status_out /* n_cells each, or NULL */,
                             int32_t* leaf_cell /* leaf_capacity */, uint64_t* leaf_in, uint64_t* leaf_out /* leaf_capacity * 16 each */,
                             double* leaf_u /* leaf_capacity * p */, double* leaf_lower /* leaf_capacity */,
                             int64_t* leaf_count /* or NULL */, slm_point_info* info /* n_cells or NULL */);

/*
 * (added under ABI 24: two new symbols beside slm_solve_l0_local_prove, no existing entry, structure or constant changes, so the
 * version stays 24 -- a caller that needs them looks the symbols up.)  LOCAL PROOF WITH GROUPS AND A HIERARCHY
 * (l0_local_group_node_kernel, csrc/l0_local_group_node_kernels.hpp; the tree: l0_prove_tree with a group map, csrc/l0_host.hpp):
 * branch and bound for slm_solve_l0_local_groups' objective F(beta) = 1/2 beta^T (G + 2 eta I) beta - c^T beta + alpha |cl(S(beta))|.
 * The dataset's groups must be contiguous and ascending in column order; need_ptr / need_idx are the direct need lists in CSR form
 * over the groups (NULL: no hierarchy).  A NODE gives every GROUP one state -- FREE, IN (it pays alpha whether zero or not) or
 * OUT (beta_g = 0) -- as two masks of 16 words of 64 bits: bit (g & 63) of word (g >> 6) is group g.  With h as for
 * slm_solve_l0_local_bound and t = c - G u, for EVERY vector u
 *       L_node(u) = -1/2 u^T G u - sum over FREE g of max(0, sum_{j in g} h(t_j) - alpha) - sum over IN g of (sum_{j in g} h(t_j) - alpha)
 *                <=  min of F over the node;
 * the relaxation ignores the hierarchy (|cl(S)| >= |S|), which lives in the branching.  slm_solve_l0_local_group_nodes bounds ONE
 * BATCH of n_nodes <= 8192 nodes in one launch, one wavefront per node, with the arguments, outputs, stopping rule and return
 * values of slm_solve_l0_local_nodes; upper_out[i] = F(u) counts |cl(S(u))|; info[i].mode = 14.  A node's masks must be CLOSED:
 * an IN group brings every group it needs (transitively) IN, an OUT group takes every group that needs it OUT.  An intercept is
 * the caller's centring, as for the grouped local search's own rows.  Refusals, all before a device is touched, each with its
 * own message, in this order: everything slm_solve_l0_local_nodes refuses up to and including a non-finite start; groups that are
 * not contiguous and ascending (SLM_ERR_UNSUPPORTED); a need_ptr that does not start at 0 or falls; a need_idx outside the
 * groups; a mask bit beyond the groups; masks that are not closed (SLM_ERR_BAD_ARG); a row-sharded dataset (SLM_ERR_UNSUPPORTED).
 */
int slm_solve_l0_local_group_nodes(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas /* [n_cells] each */,
                                   double big_M, int32_t n_nodes, const int32_t* cell /* n_nodes */,
                                   const uint64_t* in_mask /* n_nodes * 16, by group */, const uint64_t* out_mask /* n_nodes * 16 */,
                                   const double* parent_lower /* n_nodes, or NULL */, const double* starts /* n_nodes * p, or NULL */,
                                   const int32_t* need_ptr /* n_groups + 1, or NULL */, const int32_t* need_idx,
                                   int32_t max_sweeps /* <=0: default */, double gap_tol /* <0: BAD_ARG */, double* lower_out /* n_nodes */,
                                   double* primal_out /* n_nodes, or NULL */, double* upper_out /* n_nodes, or NULL */,
                                   double* u_out /* n_nodes * p, or NULL */, int32_t* stat_out /* n_nodes * 2, or NULL */,
                                   slm_point_info* info /* n_nodes or NULL */);

/*
 * (ABI 24, see above.)  slm_solve_l0_local_group_prove grows THE WHOLE TREE over group nodes for every cell of a grid, with the
 * arguments, outputs, rounds, pruning rule and return values of slm_solve_l0_local_prove.  A node is split on the FREE group whose
 * optimal z_g is closest to 1/2 among those strictly between 0 and 1 (ties: the lowest index; where every z_g is 0 or 1, the
 * largest ||u_g||_inf, then the largest sum of h(t_j)); the IN child sets g and everything need*(g) reaches IN, the OUT child g
 * and every group that transitively needs g OUT (cycles are legal).  An incumbent's value counts |cl(S)|; a child whose F(u) is
 * below the incumbent replaces it, polished on ALL columns of cl(S(u)) inside the box where that is lower still.
 * group_support_out[e] (n_groups ints, or NULL): cl(S) of cell e's incumbent.  The leaves' masks are GROUP masks; info[e].mode =
 * 15.  WHERE THE TREE CLOSES: with a ridge or a box that binds; at eta = 0 under a loose box, and with deep hierarchies whose
 * free groups are cheap, it does not, and the proven gap reached is returned.  Refusals, all before a device is touched, in this
 * order: everything slm_solve_l0_local_prove refuses up to and including an incumbent outside the box; then the groups, need_ptr,
 * need_idx and the row-sharded dataset as above.
 */
int slm_solve_l0_local_group_prove(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas /* [n_cells] each */,
                                   double big_M, const double* incumbents /* n_cells * p, or NULL */,
                                   const int32_t* need_ptr /* n_groups + 1, or NULL */, const int32_t* need_idx, double rel_gap,
                                   int32_t max_nodes, int32_t width, int32_t max_sweeps /* <=0: default */,
                                   int64_t leaf_capacity /* 0: no certificate */, double* beta_out /* n_cells * p */,
                                   double* objective_out /* n_cells */, double* lower_out /* n_cells */, int32_t* nodes_out,
                                   int32_t* rounds_out, int32_t* status_out /* n_cells each, or NULL */,
                                   int32_t* group_support_out /* n_cells * n_groups, or NULL */, int32_t* leaf_cell /* leaf_capacity */,
                                   uint64_t* leaf_in, uint64_t* leaf_out /* leaf_capacity * 16 each */, double* leaf_u /* leaf_capacity * p */,
                                   double* leaf_lower /* leaf_capacity */, int64_t* leaf_count /* or NULL */,
                                   slm_point_info* info /* n_cells or NULL */);

/*
 * (added under ABI 24: two new symbols beside slm_solve_l0 and slm_solve_l0_wide, no existing entry, structure or constant
 * changes, so the version stays 24 -- a caller that needs them looks the symbols up.)  The exact l0 search with the
 * EXCLUSION BOUND (csrc/l0_kernels.hpp, template parameter XB): the arguments, outputs, argument errors and contract of
 * slm_solve_l0 and slm_solve_l0_wide, and on any problem with a unique optimum that both searches finish the same
 * coefficients, support and objective bit for bit (the winner is recomputed on the host by the same function).  What differs
 * is the subtree bound: q_all + alpha (|S| + 1) becomes q(all \ E) + alpha (|S| + 1), E the columns of the groups the path has
 * excluded, from P = H^-1 and P c by a second register Cholesky (of P on E) that grows with every exclude; the increment is
 * lowered by the relative margin delta = 256 kappa_1 2^-53, kappa_1 = ||H||_1 ||P||_1 (csrc/l0_host.hpp, l0_excl_bound).  The
 * search visits fewer nodes and each costs more; nothing else changes -- *lower_bound_out on a spent budget stays
 * min(objective, q_all).  FALLBACK, not refusal: when H is not positive definite on all columns under the pivot rule (n < p
 * with eta = 0, duplicated columns), or delta >= 1/2, the call runs the kernel and bound of slm_solve_l0 / slm_solve_l0_wide.
 * info->mode says which ran: 5 the exclusion bound, 6 q_all because H is not positive definite, 7 q_all because delta >= 1/2;
 * info->beta_norm holds delta (0 under mode 6) instead of ||beta||_2; the other fields as for the plain entries.
 */
int slm_solve_l0_xb(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T /* p*p or NULL */, double big_M,
                    const uint64_t* need /* n_groups masks or NULL */, int64_t max_nodes /* <=0: default */, double* beta_out,
                    uint64_t* support_out, double* lower_bound_out, int64_t* nodes_out, slm_point_info* info);
int slm_solve_l0_xb_wide(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T /* p*p or NULL */,
                         double big_M, const uint64_t* need /* 2 words per group, low word first, or NULL */,
                         int64_t max_nodes /* <=0: default */, double* beta_out, uint64_t* support_out /* [2] */,
                         double* lower_bound_out, int64_t* nodes_out, slm_point_info* info);

/*
 * (added under ABI 24: a new symbol beside slm_solve_l0, no existing entry, structure or constant changes, so the version
 * stays 24 -- a caller that needs it looks the symbol up.)  The exact l0 search under LINEAR CONSTRAINTS on the coefficients
 * (csrc/l0_kernels.hpp, template parameter CON; the reference's add_constraints on its mixed-integer estimators,
 * examples/plot_chull.py:157-183): slm_solve_l0's problem and arguments with, in addition,
 *       lo <= A beta <= hi   (A: m x p row-major, m <= 64; an infinite lo_i or hi_i leaves that side open)   and
 *       box_lo_j <= beta_j <= box_hi_j   (each NULL: -big_M / +big_M; intersected with +-big_M; box_lo_j <= 0 <= box_hi_j).
 * A column whose interval excludes 0 is forced active -- that is a row e_j of A, not a box.  A support's value f(S) is a
 * quadratic programme (+inf where no beta on S is feasible); f(S) >= q(S) keeps the register Cholesky as an exact lower-bound
 * filter, and a node that passes it is valued on chip by a splitting (augmented Lagrangian of the rows, clipped coordinate
 * sweeps) that ends every sweep with a dual value D <= f(S), lowered by a rounding margin.  A candidate is VALUED (rows within
 * 1e-9 of their scale, value within 1e-9 of D: L0_CON_TOL), REJECTED (D above what it has to beat; infeasible supports end so)
 * or UNSETTLED (max_qp_sweeps sweeps ran out, <= 0: 20000; D + alpha |S| is then a lower bound on that one support).
 * G + 2 eta T must be positive definite on all columns (with constraints a dependent column can lower the value):
 * SLM_ERR_UNSUPPORTED otherwise, with a message that names the cure (eta > 0, or a design of full column rank) -- as for
 * m > 64, more than 64 columns or groups, and row-sharded datasets.  SLM_ERR_BAD_ARG before anything is launched: m < 0, a NaN
 * or an infinity in A, a NaN bound, lo_i > hi_i, box_lo_j > 0 or box_hi_j < 0, and slm_solve_l0's own.
 * beta_out, support_out, nodes_out as for slm_solve_l0; the winner's coefficients come from the same splitting on the host
 * followed by an exact solve on the face it identifies (active rows and clipped coordinates fixed), kept when feasibility and
 * the multipliers' signs hold.  lambda_out [m] (may be NULL): the rows' multipliers, 0 = H beta - c + A^T lambda + mu on the
 * support, > 0 only where hi binds, < 0 only where lo binds (mu: the box's).  *lower_bound_out = min(objective, the lowest
 * bound of an unsettled candidate), and the bound on all columns as well when the node budget ran out.  SLM_OK iff the search
 * finished and the objective is <= every unsettled bound; otherwise SLM_ERR_NOT_CONVERGED with valid outputs.  When the search
 * finished, nothing is unsettled and no feasible admissible support exists: SLM_ERR_BAD_ARG ("no admissible support").
 * info as for slm_solve_l0 with info->L = F_lb, the proven lower bound on f(all columns) the subtree bound used;
 * info->rejects = candidates valued on chip; info->resid = candidates left unsettled; info->beta_norm = the lowest of their
 * bounds (+inf: none).
 */
int slm_solve_l0_constrained(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T /* p*p or NULL */,
                             double big_M, const uint64_t* need /* n_groups masks or NULL */, int64_t max_nodes /* <=0: default */,
                             const double* A /* m*p */, int32_t m, const double* lo /* m */, const double* hi /* m */,
                             const double* box_lo /* p or NULL */, const double* box_hi /* p or NULL */,
                             int32_t max_qp_sweeps /* <=0: default */, double* beta_out, uint64_t* support_out,
                             double* lower_bound_out, int64_t* nodes_out, double* lambda_out /* m or NULL */,
                             slm_point_info* info);

/*
 * The Gram of a row set, for covariance passes (SLM_FLAG_COVARIANCE): G = X^T W X / n_eff, c = X^T W y / n_eff and
 * y^T W y / n_eff, kept with the dataset (8 ld^2 bytes each) and found again by a fingerprint of the row weights and
 * n_eff -- what a lane of slm_solve_lanes brings as (row_weight, n_eff).  row_weight: length n on the host, NULL = the
 * dataset's own; n_eff <= 0 = the dataset's row count (the rule of slm_lane).  A 0/1 mask that leaves out at most half
 * of the rows costs the Gram of the rows left out (the Gram of all rows is built once per dataset and kept); other
 * weights cost a scaled copy of X and a full product.  The product is cov_syrk_kernel (fp64 matrix cores, the lower
 * triangle: 50 ms for all rows at 100 000 x 5 000, 11 ms for a fold's test rows).  Worth it when many solves share the row set: the ten
 * l1_ratio rows x fifty alphas of a CV fold, the rounds of an Adaptive* grid.  Replaces nothing in the
 * reference (cvxpy has no Gram form; scikit-learn's lasso_path(precompute=True) is the same idea on the host).
 * SLM_ERR_UNSUPPORTED on row-sharded datasets and rows beyond the split pass's 10 240 columns.  New targets
 * (slm_dataset_set_targets) and centring (slm_dataset_center) drop the Grams built so far.  At most sixteen Grams are
 * kept per dataset; the oldest goes first.
 */
int slm_dataset_covariance(slm_dataset* ds, const double* row_weight, int64_t n_eff);
/* The folds of a K-fold split at once: count (row_weight, n_eff) pairs.  When the masks' zeros are a partition of the rows
 * -- the test rows of K folds -- the Gram of all rows is the sum of the test rows' Grams and is never formed from X: K
 * products over n / K rows each.  Anything else is built mask by mask, as by slm_dataset_covariance. */
int slm_dataset_covariance_folds(slm_dataset* ds, const double* const* row_weights, const int64_t* n_effs, int32_t count);
/* The same in two steps.  _begin queues the products on the engine's stream and returns (*started_out = 0 and nothing queued
 * when the masks are no such partition: use slm_dataset_covariance then); _finish forms the Grams and files them.  Between the
 * two the caller may queue other work -- and a REPLICA (slm_dataset_set_replicated) on an engine with a communicator enters
 * its collective in _finish only: _begin builds the parts of this rank's n_ranks-th of the rows ([X_f^T X_f | X_f^T y_f |
 * y_f . y_f] of every fold's test rows among them: 1 / n_ranks of the products), _finish sums each part over the ranks (one
 * all-reduce of ld^2 + ld + 16 doubles per fold on a second stream, part f under way while part f + 1 is still being
 * multiplied) -- the grid mode's only collective (SURVEY 8e-1 has none; the reference dispatches whole fits,
 * src/sparselm/model_selection.py:273,304-323).  Every rank must call both with the same masks. */
int slm_dataset_covariance_folds_begin(slm_dataset* ds, const double* const* row_weights, const int64_t* n_effs, int32_t count,
                                       int32_t* started_out);
int slm_dataset_covariance_folds_finish(slm_dataset* ds);
int slm_dataset_covariance_count(slm_dataset* ds, int32_t* count_out);
/* Drops every Gram built so far (and a build under way): the memory goes back, later solves run over X. */
int slm_dataset_covariance_clear(slm_dataset* ds);
/* Diagnostic (tests): Gram `index` (oldest first) to the host -- G_out p x p (C-order), c_out length p (either may be NULL),
 * scalars_out = {y^T W y / n_eff, n_eff, the two fingerprint sums of the row weights}. */
int slm_dataset_covariance_download(slm_dataset* ds, int32_t index, double* G_out, double* c_out, double scalars_out[4]);

/*
 * Measurement: the rate at which THIS device streams the dataset's copy of X through plain 16-byte loads that are only
 * summed up (`reps` sweeps after one warm-up, HIP events) -- the read-only ceiling the passes over X are read against
 * (bench.py `roofline.read_stream_ceiling_gbs`; SURVEY Appendix D asks for it, the reference has no counterpart).
 */
int slm_dataset_read_ceiling(slm_dataset* ds, int32_t reps, double* gbs_out, double* ms_out);

/*
 * The model Gram (csrc/mg_kernels.hpp): G~ ~ X^T W X / n of the dataset's own rows and row weights from ONE product on the
 * fp16 matrix cores (columns scaled by powers of two, fp32 accumulation over chunks of rows, chunks summed in fp64):
 * relative error ~1e-4, built in a few milliseconds where the fp64 Gram of slm_dataset_covariance takes ten times as
 * long.  It only ever PROPOSES points: lanes of a working-set solve whose solutions outgrow the working set's 512 columns
 * take their next point from proximal-gradient steps on it (one read of its 8 p^2 bytes per step for sixteen lanes) and
 * every proposal is verified by a pass over X in fp64 under the unchanged acceptance test and stopping rule -- the
 * reference's solve has no density regime either (src/sparselm/model/_base.py:512-519).  Solves build it themselves when
 * they need it (slm_solve_stats.mg_*; SLM_FLAG_NO_MODEL_GRAM keeps them from it) and it stays with the dataset; this
 * entry point builds it now -- e.g. before the paths of a search -- and, for tests, hands it to the host: G_out ld x ld
 * (C-order, ld = p rounded up to a multiple of 16) or NULL.  SLM_ERR_UNSUPPORTED on row-sharded datasets and for
 * p > 16 384.
 */
int slm_dataset_model_gram(slm_dataset* ds, double* G_out);
/* On an engine with a communicator a dataset is a row block of one tall matrix (the row-sharded mode below) unless it is
 * marked as a replica: every rank then holds ALL rows, solves its own lanes without any per-pass collective (grid mode), and
 * the communicator only carries the folds' Grams (slm_dataset_covariance_folds). */
int slm_dataset_set_replicated(slm_dataset* ds, int32_t replicated);

/* ---- row-sharded mode (very tall X split by rows over ranks) ----------------------------------------
 * Every rank holds a block of rows and runs the whole state machine; per pass the ranks enter TWO all-reduces: the
 * lanes' gradients (ld + 16 doubles each), and a 16-double stop vector -- in working-set solves riding behind the
 * staged Gram parts in one buffer.  slm_dataset_center all-reduces the weighted sums and X^T w, so the global means are
 * subtracted.  HBM per rank: X plus, in working-set solves, its column-major copy (2 x 8 n p bytes). */
#define SLM_COMM_ID_BYTES 128
/* Rank 0 creates the id and distributes the 128 bytes to the other ranks out of band. */
int slm_comm_unique_id(uint8_t id_out[SLM_COMM_ID_BYTES]);
/* Collective over all ranks: afterwards slm_gradient / slm_solve_path on datasets of this engine
   sum X^T r (and the loss / n) over ranks with RCCL; n_global replaces n in the 1/n scaling. */
int slm_comm_init(slm_engine* eng, int32_t rank, int32_t n_ranks,
                  const uint8_t id[SLM_COMM_ID_BYTES]);
/* Rank and size of the engine's communicator as RCCL reports them (1 rank, rank 0 without one). */
int slm_comm_info(slm_engine* eng, int32_t* rank_out, int32_t* n_ranks_out);
/* All-reduces this engine has entered since its communicator was created: ranks of one job must agree
   on it at every quiescent point (the row-sharded state machine takes its stop decision from a word the
   ranks all-reduce after every pass, so that they do whatever their own states say). */
int slm_comm_collectives(slm_engine* eng, int64_t* count_out);
/* Measurement: microseconds per all-reduce of `count` doubles on the engine's communicator (`reps` of them on its stream,
 * after one warm-up, HIP events) -- the per-collective floor of a row-sharded pass (bench.py `rowshard.collective_us`).
 * Every rank of the communicator calls it with the same arguments. */
int slm_comm_all_reduce_probe(slm_engine* eng, int64_t count, int32_t reps, double* us_out);
/*
 * In-process communicator: the n_ranks engines (one process, ONE device, each driven by its own host
 * thread) become the ranks of a row-sharded job; the all-reduce is a rendezvous of their streams with the
 * staged buffers added in rank order.  For single-GPU boxes, where RCCL cannot form a group of several
 * ranks, and for the tests of the multi-rank state machine; a rank that fails to enter a collective within
 * timeout_s (<= 0: 30 s) fails it with SLM_ERR_COMM on the others instead of hanging them.
 */
int slm_comm_init_local(slm_engine** engines, int32_t n_ranks, double timeout_s);
/* n_global replaces n in the 1/n (gradient) and 1/(2n) (loss) scaling: the global row count of a
   row-sharded matrix, or the number of unmasked rows when row weights act as a CV-fold mask. */
int slm_dataset_set_global_rows(slm_dataset* ds, int64_t n_global);
int slm_comm_destroy(slm_engine* eng);

#ifdef __cplusplus
}
#endif
#endif /* SLM_ENGINE_H */
