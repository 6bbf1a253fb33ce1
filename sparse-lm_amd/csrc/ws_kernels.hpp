// Working-set refinement: Gram-assisted prediction of the next iterate between two passes over X.
//
// f(b) = 1/(2n) ||X b - y||^2_W is quadratic, so once the gradient g0 = grad f(z0) at ONE point is
// known (the fused pass just delivered it), the gradient at any b that differs from z0 only on a
// small column set W is exact without touching X again:
//
//     grad f(b)_W = g0_W + G_WW (b - z0)_W,        G_WW = X_W^T diag(w) X_W / n     (K x K, K <= 512)
//
// The kernels below (i) pick W on the device (every coefficient that is non-zero in any lane plus the
// features / groups whose gradient is within a factor theta of entering at the loosest penalty of
// the lane's range), (ii) gather the K columns into a compact n x K matrix, (iii) build G_WW with
// f64 MFMA (the one GEMM-shaped piece of this path: 2 n K^2 flop), and (iv) after every pass let one
// workgroup per lane minimise the penalised quadratic model over W (FISTA on K unknowns, the matrix
// stays in L2) and move the lane's next evaluation point there.  The next pass over X then VERIFIES
// that point with the true gradient under the unchanged stopping rule of fista_tail_kernel, so the
// meaning of `tol` and every reported solution are exactly those of the plain iteration; a point of
// a path costs one pass instead of three to seven.  Coordinates outside W are never touched: if a
// lane's iterate moves there (a feature outside W wants to enter) the refinement is skipped for
// that lane and W is rebuilt.
//
// Counterpart in the reference: none (cvxpy hands the whole problem to an interior-point solver,
// src/sparselm/model/_base.py:512-519); the idea is the covariance-update / working-set strategy
// of coordinate-descent Lasso solvers, restated for the proximal-gradient state machine.
#pragma once
#include <type_traits>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tail_kernels.hpp"
#include "newton_kernels.hpp"

namespace slm {

constexpr int WS_KCAP = 512;        // capacity of the working set (leading dimension of G and XW)
constexpr int WS_KLDS = 112;        // up to this many columns the Gram lives in LDS during the model solve
constexpr int WS_TILES = WS_KCAP / 16; // 16x16 tiles per side of the Gram
constexpr int WS_THREADS = 1024;
constexpr int WS_INNER_MAX = 400;   // inner iterations per refinement
constexpr int WS_BB_ITERS = 14;         // spectral steps the model solver opens with
constexpr double WS_BB_MAX_STEP = 20.0; // longest of them, in steps of 1/L
constexpr double WS_INNER_TOL = 0.05;  // inner stop: residual <= WS_INNER_TOL * tol * ||b||
constexpr int WS_MAX_REPEATS = 6;   // refinements of one path point before the lane iterates plainly
// Direct step of the model solver (newton_kernels.hpp): when the proximal-gradient iteration on the model has
// not converged after WS_NEWTON_AFTER iterations -- or the curvature it measures along its own moves says
// the face is ill-conditioned (Rayleigh quotient below WS_NEWTON_RQ of lambda_max) -- a projected Newton step
// on the free coordinates (Cholesky solve, ws_solve_kernels.hpp `ws_direct_step`) replaces further iterations; one prox-gradient
// step after it tests convergence, and the next direct step follows at once if that fails.
constexpr int WS_NEWTON_AFTER = 16;
// Direct steps per refinement.  Where the projected trial points do not lower the model (ill-conditioned faces: the projection
// destroys the cancellations the direction lives on) a step is the straight segment to the first sign change, i.e. ONE
// coordinate changes sides per step, and a start that is not yet on the minimiser's face needs about as many steps as the
// face has positions: 129 from a start with 80 of 120 coordinates non-zero to a minimiser with 30 (per-feature penalty,
// condition 1e8, direct mode from the first iteration; tests/test_model_solver_gpu.py::test_start_hard).  Until this was 256 it
// was 64: that solve ended unsettled, and so did the next five refinements of such a point -- the same steps in all, with a
// pass over X between every 64 of them.  WS_INNER_MAX bounds the steps of a refinement as before.
constexpr int WS_NEWTON_MAX = 256;
constexpr int WS_AFTER_DIRECT = 40;  // iterations left to a refinement whose direct steps are used up: on a face that
                                     // needed them more would not converge either -- the next pass re-expands the model
                                     // at the point reached and the refinement resumes from there
constexpr double WS_NEWTON_RQ = 0.05;
constexpr int WS_NEWTON_REFUSALS = 4; // refused direct steps after which a refinement stops trying
constexpr double WS_NEWTON_ENTER = 0.3;
constexpr int WS_NEWTON_RESOLVE = 5; // solves per direct step while the free set is being made consistent
static_assert(NT_MAXT * NT_B == WS_KCAP, "the direct solve covers a full working set");

struct WsCtl {
  int32_t request;    // (re)build W at the next opportunity
  int32_t building;   // select changed W in this pass: gather / gram / reduce must run
  int32_t valid;      // G matches idx
  int32_t K;          // columns in use, padded to a multiple of 16 (padding entries have idx = -1)
  int32_t Kreal;      // columns in use without the padding
  int32_t k_new;      // first position whose column / Gram rows this build has to produce (0 = all)
  int32_t builds;     // full selections built
  int32_t appends;    // builds that only appended columns to the existing W
  int32_t max_builds;
  int32_t disabled;   // the non-zero coefficients alone kept exceeding WS_KCAP
  int32_t misses;     // times a lane's plain step left W
  int32_t refined;    // refinements applied (all lanes)
  int32_t counter;    // last-workgroup detection of the reduce kernel
  int32_t stale;      // a lane left W and the build budget is spent: such lanes iterate plainly
  int32_t overflows;  // builds skipped because the non-zero coefficients alone exceed WS_KCAP
  int32_t sweep_new;  // ws_score_kernel -> ws_select_kernel: features of newcomers at theta ...
  int32_t sweep_miss; // ... and coordinates a plain step moved outside W (both reset by ws_select_kernel)
  int32_t staged;     // row-sharded mode: the local Gram parts sit in the staging matrix, waiting for the
                      // all-reduce and ws_publish_kernel
  int32_t inner_iters;  // model-solver iterations of all refinements (diagnostics: SLM_TRACE=2)
  int32_t hard;         // direct steps were needed earlier in this call: refinements start with them
  int32_t hard_next;    // ... as recorded during the current pass (ws_select_kernel publishes it between passes)
  int32_t newton_steps; // direct (Cholesky) steps taken by the model solver, all lanes
  int32_t newton_fails; // ... refused: face not positive definite, or the step did not lower the model
  int32_t newton_nopd;  // ... of which: Cholesky pivot below the floor
  int32_t newton_trial[4];  // accepted trial of a direct step: full step, 1/2, 1/4, up to the first sign change
  int32_t newton_ref[4];    // refused steps: no sign-consistent segment (t = 0), slope <= 0, curvature <= 0, no decrease
  int32_t newton_factors;   // Cholesky factorisations (a direct step re-solves when zero coordinates move the wrong way)
  int32_t newton_unknowns;  // sum of their sizes
  // device clock ticks (wall_clock64: 100 MHz) spent by each lane's workgroup in the parts of its direct steps
  // (SLM_TRACE=2 prints them): matvec + free set, assembly, factorisation, solve, trial points, mu
  unsigned long long nt_ticks[SLM_MAX_LANES][6];
  int32_t nt_factors[SLM_MAX_LANES];
  // ... and in the parts of lane 0's refinements: set-up, lambda_max of a new Gram, start value, the iteration,
  // acceptance + write-back (SLM_TRACE=2)
  unsigned long long solve_ticks[5];
  int32_t want_full[SLM_MAX_LANES];  // lanes the light model solver left to the one with direct steps (this pass)
  int32_t iters_hist[32];  // (SLM_TRACE=2) model solves by their number of iterations (last bin: 31 or more)
  unsigned long long lane_ticks[SLM_MAX_LANES];  // (SLM_TRACE=2) ws_solve_kernel, entry to exit, per lane
  int32_t last_point[SLM_MAX_LANES];  // path point of each lane's last refinement ...
  int32_t repeats[SLM_MAX_LANES];     // ... and how many times in a row it was that point WITH the same columns
  int32_t last_cols[SLM_MAX_LANES];   // columns W held at each lane's last refinement (growth resets the count)
  double Lw[SLM_MAX_LANES];  // lambda_max estimate per Gram (0 = not yet computed)
  int32_t carried;    // this solve took over the working set of the solve before it (ws_ctl_carry_kernel): its first
                      // selection may append as much as a fresh one would choose
  int32_t outgrown;   // selections that did not fit: appends that would pass WS_KCAP, non-zeros alone beyond it -- the solve's
                      // lanes are outgrowing the working set (solve_core turns the model-Gram rounds on, mg_kernels.hpp)
  int32_t served[SLM_MAX_LANES];  // lanes the model solver moved since the model-Gram rounds last looked (mg_begin_kernel,
                                  // mg_kernels.hpp: what the working set serves is not served twice)
  int32_t hard_lane[SLM_MAX_LANES];  // a refinement of THIS lane needed direct steps: its next ones start with them.  (Round 5:
                                     // per lane, not per call -- one refinement of 31 iterations among the 84 of a path sent
                                     // every later one of all eighteen lanes through two factorisations of 200 unknowns, 0.4 ms
                                     // each where eight iterations take 20 us: 26 ms for an 8-pass path, soak seed 29)
};

struct WsArgs {
  WsCtl* ws;
  int32_t* idx;    // [WS_KCAP] feature of working-set position k, or -1
  int32_t* pos;    // [ld] position of feature j in W, or -1
  int32_t* gs;     // [WS_KCAP] first position of k's group
  int32_t* gl;     // [WS_KCAP] members of k's group
  double* score;   // [ld] scratch: entry score per item
  double* XW;      // [n][WS_KCAP] gathered columns
  double* part;    // [n_sets][tile][nblk][16 x 16] partial Grams
  double* Gm;      // [n_sets][WS_KCAP * WS_KCAP]
  double* nt;      // [SLM_MAX_LANES][NT_SCRATCH] factor of each lane's direct solve (nullptr: no direct solves)
  double* Gx;      // row-sharded mode: [n_sets][WS_KCAP * WS_KCAP] staging, zeroed every pass, summed over
                   // ranks between ws_gram_reduce_kernel and ws_publish_kernel (nullptr otherwise)
  const double* X;
  const double* XT;   // column-major copy of X in tiles of 32 rows (tile_columns_kernel; built once per dataset)
  int64_t n, ld;
  const double* rw;   // row weights per set, or nullptr (all ones)
  int64_t rw_stride;
  double inv_n[SLM_MAX_LANES];        // per SET: 1 / n_eff
  int32_t set_of[SLM_MAX_LANES];      // Gram of lane l (lanes with the same row weights and scaling share one)
  int32_t set_lane[SLM_MAX_LANES];    // a lane of set s (whose row weights the Gram kernel reads)
  int32_t n_sets;     // distinct (row weights, 1/n scaling) among the lanes
  int32_t nblk;
  const int32_t* owner;  // [n_sets][nblk] whose partial Gram of a row block a set sums up (ws_block_owner_kernel), or nullptr: its own
  double theta;
  int32_t lookahead;   // path points ahead whose penalty decides what enters W now
  int32_t append_max;  // newcomers appended per pass (the likeliest first)
  int32_t k_init;      // a fresh selection is cut down to this size (or to its non-zeros)
  int32_t bb_steps;    // the model solver opens with spectral steps (SLM_WS_BB=0: accelerated steps throughout)
  int32_t one_solver;  // SLM_WS_ONE_SOLVER=1: every lane goes to the solver with direct steps (measurements)
  int32_t miss_factor; // an append after a miss may take up to this many times append_max (4) ...
  int32_t miss_div;    // ... one more append_max for every miss_div coordinates the plain steps moved outside W
  double fill;         // a selection cut down to a cap stops bisecting its threshold once it holds this share of the cap
  int32_t power_iters; // power steps for lambda_max of a new Gram (slm_host::kWsPowerIters)
  int32_t hard_call;   // SLM_HARD_CALLWIDE=1 (A/B runs): direct steps once needed start every later refinement of the CALL
  int32_t keep_full;   // a selection that does not fit leaves W as it is (`stale`: the lanes it no longer covers are served by
                       // the model-Gram rounds) instead of selecting, gathering and multiplying afresh pass after pass
};

// The first words of the control block (request ... hard_next) and the call's stop word in ONE round trip: the first
// WS_HEAD_WORDS + 1 threads fetch a word each into `hd`; the caller's barrier makes them visible.  (A kernel that reads
// five words behind five tests waits five times; worth 1.2 us of ws_score_kernel's 15.6, nothing measurable in
// ws_select_kernel, which keeps its plain reads.)
constexpr int WS_HEAD_WORDS = 24;
static_assert(offsetof(WsCtl, hard_next) / 4 < WS_HEAD_WORDS, "the words the pass kernels decide on");
#define WS_HEAD(hd, field) ((hd)[offsetof(WsCtl, field) / 4])
__device__ __forceinline__ void ws_head_load(const WsCtl* ws, const int* gdone, int32_t* hd) {
  const int tid = threadIdx.x;
  if (tid < WS_HEAD_WORDS) hd[tid] = reinterpret_cast<const int32_t*>(ws)[tid];
  else if (tid == WS_HEAD_WORDS) hd[tid] = gdone ? gdone[0] : 0;
}

// state of a fresh solve (the block is zeroed first): a build is requested, no lane has been refined yet
static __global__ void ws_ctl_init_kernel(WsCtl* ws, int max_builds) {
  if (threadIdx.x == 0) {
    ws->request = 1;
    ws->max_builds = max_builds;
  }
  if (threadIdx.x < SLM_MAX_LANES) ws->last_point[threadIdx.x] = -1;
}

// Everything a solve sets up on the device before its first pass, in ONE launch (round 6): the vectors (solve_setup_body), the
// path points and the lanes' control blocks -- fetched by the kernel from the page-locked staging the host has just filled, not
// by copy commands --, the head of the control block zeroed, the step-size seed written into the lanes' blocks
// (seed_step_kernel's work) and the working set's state started (ws_ctl_init_kernel's).  They were six commands of the stream,
// 4-6 us each, in front of every solve: a third of the 0.1 ms the device spent before the first pass of a headline path.
struct BeginArgs {
  const PathCtl* h_ctl;  // [n_lanes] page-locked, device-visible
  PathCtl* ctl;
  const slm_path_point* h_pts;  // [n_pts] page-locked, device-visible
  slm_path_point* pts;
  int64_t n_pts;
  int32_t* head;       // the control block's first words (GlobalCtl, MgCtl[, WsCtl]) ...
  int32_t head_words;  // ... this many of them are zeroed
  const double* lambda;  // step-size estimate on the device (nullptr: the host has written L into h_ctl)
  double margin;
  double factor[SLM_MAX_LANES];
  WsCtl* ws;           // nullptr: the working set's state is left alone (not used, taken over, or set up later)
  int32_t max_builds;
  int32_t n_lanes;
};
static __global__ __launch_bounds__(256) void solve_begin_kernel(SetupArgs s, BeginArgs b) {
  solve_setup_body(s);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  {  // path points: four doubles each
    static_assert(sizeof(slm_path_point) == 4 * sizeof(double), "points travel as doubles");
    const double* src = reinterpret_cast<const double*>(b.h_pts);
    double* dst = reinterpret_cast<double*>(b.pts);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < 4 * b.n_pts; e += stride) dst[e] = src[e];
  }
  if (blockIdx.x != 0) return;
  for (int e = threadIdx.x; e < b.head_words; e += 256) b.head[e] = 0;
  {
    static_assert(sizeof(PathCtl) % sizeof(int32_t) == 0, "control blocks travel as words");
    const int32_t* src = reinterpret_cast<const int32_t*>(b.h_ctl);
    int32_t* dst = reinterpret_cast<int32_t*>(b.ctl);
    const int words = b.n_lanes * (int)(sizeof(PathCtl) / sizeof(int32_t));
    for (int e = threadIdx.x; e < words; e += 256) dst[e] = src[e];
  }
  __syncthreads();
  if (b.lambda != nullptr && (int)threadIdx.x < b.n_lanes && threadIdx.x < SLM_MAX_LANES) {  // (seed_step_kernel)
    const int l = threadIdx.x;
    double L0 = b.lambda[0] * b.margin;
    if (L0 <= 0.0) L0 = 1.0;  // X == 0
    const double L = L0 * b.factor[l];
    b.ctl[l].L = L;
    b.ctl[l].ak = 1.25 * L;
    b.ctl[l].Lhat = 0.5 * L0;
  }
  if (b.ws != nullptr) {  // (ws_ctl_init_kernel; the block was zeroed above)
    if (threadIdx.x == 0) {
      b.ws->request = 1;
      b.ws->max_builds = b.max_builds;
    }
    if (threadIdx.x < SLM_MAX_LANES) b.ws->last_point[threadIdx.x] = -1;
  }
}

// state of a solve that starts where the dataset's last solve ended (solve_core: carried start, same lanes, same row
// sets): that solve's working set is still in place -- the columns' indices and positions, the gathered columns, the
// Grams, which depend on X and the rows alone -- and the penalty has changed, not the data.  The counters and per-solve
// records start afresh; W, its size and the Grams' lambda_max stay, and the first selection appends what the new
// penalty lets in instead of choosing, gathering and multiplying everything again (config 5's re-weighted solves: 0.8 ms
// of gather + Gram + reduce each).  One workgroup of 256.
static __global__ __launch_bounds__(256) void ws_ctl_carry_kernel(WsCtl* ws, int max_builds) {
  __shared__ int keep_i[2];
  __shared__ double keep_L[SLM_MAX_LANES];
  if (threadIdx.x == 0) {
    keep_i[0] = ws->K;
    keep_i[1] = ws->Kreal;
  }
  if (threadIdx.x < SLM_MAX_LANES) keep_L[threadIdx.x] = ws->Lw[threadIdx.x];
  __syncthreads();
  int32_t* words = reinterpret_cast<int32_t*>(ws);
  for (int e = threadIdx.x; e < (int)(sizeof(WsCtl) / sizeof(int32_t)); e += 256) words[e] = 0;
  __syncthreads();
  if (threadIdx.x == 0) {
    ws->K = keep_i[0];
    ws->Kreal = keep_i[1];
    ws->valid = 1;
    ws->carried = 1;
    ws->max_builds = max_builds;
  }
  if (threadIdx.x < SLM_MAX_LANES) {
    ws->Lw[threadIdx.x] = keep_L[threadIdx.x];
    ws->last_point[threadIdx.x] = -1;
  }
}

// exclusive prefix sum of one int per thread over the 1024-thread workgroup
__device__ __forceinline__ int block_excl_scan(int v, int* wave_tot /*[16]*/, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  __syncthreads();
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < TAIL_WAVES; ++w) {
    const int t = wave_tot[w];
    if (w < wave) base += t;
    tot += t;
  }
  *total = tot;
  return base + inc - v;
}

// ---------------------------------------------------------------------------------------------
// (i-a) one sweep over the items (features, or groups), one thread each: entry score (max over lanes;
// +inf marks items that are non-zero at a lane's expansion point), the feature count of newcomers at
// the default threshold, and whether the plain step of any lane moved a coordinate outside W
// (z = candidate / extrapolated point just produced by the tail kernel, zprev = the point it was
// produced from: they differ outside W exactly when a feature outside W wants to enter).
// Per-lane constants: is the lane walking a path, and the penalty scales w.lookahead points ahead of
// where it is (ranges may move between lanes in shared-path mode, so the look-ahead runs to the end of
// the path there).  Features that would enter by then are taken now; later ones are appended when
// their time comes.  (Inside the one-workgroup select kernel this sweep cost 45-60 us per pass.)
// ---------------------------------------------------------------------------------------------
// (the body, for the workgroup that scores items chunk * blockDim.x ...: ws_score_kernel runs it per blockIdx.x in workgroups
//  of 256 (features) or 64 (groups) threads)
__device__ __forceinline__ void ws_score_body(TailArgs a, WsArgs w, const int chunk) {
  WsCtl* ws = w.ws;
  const int tid = threadIdx.x;
  // The words this kernel decides on, fetched TOGETHER (ws_head_load) instead of one after the other behind the tests they
  // feed (`a || b` is two dependent round trips), and the lanes' point counts by a thread each instead of a loop per thread.
  __shared__ int32_t hd[WS_HEAD_WORDS + 1];
  __shared__ int lane_np[SLM_MAX_LANES];
  ws_head_load(ws, a.gdone, hd);
  if (tid < SLM_MAX_LANES) lane_np[tid] = tid < a.n_lanes ? a.ctl[tid].n_points : 0;  // (workgroups of 64 threads score groups)
  __syncthreads();
  if (hd[WS_HEAD_WORDS] != 0 || WS_HEAD(hd, disabled)) return;
  const bool had_w = WS_HEAD(hd, valid) != 0;
  if (!WS_HEAD(hd, request) && !had_w) return;
  if (WS_HEAD(hd, builds) >= WS_HEAD(hd, max_builds) || WS_HEAD(hd, appends) >= 8 * WS_HEAD(hd, max_builds)) return;
  const bool singleton = a.singleton != 0;
  const int nitems = singleton ? a.p : a.G;
  __shared__ int lane_live[SLM_MAX_LANES];
  __shared__ double lane_sa[SLM_MAX_LANES], lane_sb[SLM_MAX_LANES];
  __shared__ int cnt[2];
  if (tid < SLM_MAX_LANES) {
    int live = 0;
    double sa = 0.0, sb = 0.0;
    if (tid < a.n_lanes) {
      const PathCtl* c = a.ctl + tid;
      live = !(c->done || c->idle);
      int path_end = 0;
      for (int l = 0; l < SLM_MAX_LANES; ++l) path_end = max(path_end, lane_np[l]);
      const int end = a.steal ? path_end : c->pt_off + c->n_points;
      // (interleaved lanes jump `stride` points at a time: look at least as far as the next one)
      int look = min(c->pt_off + c->point + max(w.lookahead, c->stride), end - 1);
      if (c->tail_pt >= 0 && c->point + c->stride >= c->n_points) look = c->pt_off + c->tail_pt;  // (its next point)
      const slm_path_point pe = a.pts[look < 0 ? 0 : look];
      sa = pe.sa;
      sb = pe.sb;
    }
    lane_live[tid] = live;
    lane_sa[tid] = sa;
    lane_sb[tid] = sb;
  }
  if (tid == 0) cnt[0] = cnt[1] = 0;
  __syncthreads();

  const double inf = __builtin_huge_val();
  int n_new = 0, n_miss = 0;
  // features: one thread each.  Groups: SIXTEEN threads each, one per lane (a thread then walks the members
  // of its group for one lane: 10 x 4 scattered loads instead of 16 x 10 x 4; the lanes' scores meet in a
  // max over the 16 threads) -- 64-thread workgroups, four groups each.
  const int gt = chunk * (int)blockDim.x + tid;
  const int it = singleton ? gt : gt >> 4;
  if (singleton) {
    if (it < nitems) {
      double sc = 0.0;
      const int j = it;
      const bool in_w = had_w && w.pos[j] >= 0;
      // all loads of all lanes first (unconditional, clamped to a lane that exists), then the arithmetic: with
      // the tests between them every lane cost two dependent round trips, 32 in a row (21 us per pass)
      // (sixteen lanes at a time: a call of thirty-two is two such rounds -- all of them in registers at once would be 320)
      for (int l0 = 0; l0 < a.n_lanes; l0 += 16) {
        double zp[16], zz[16], aa[16], bb[16], gg[16];
#pragma unroll
        for (int l = 0; l < 16; ++l) {
          const int ll = l0 + l < a.n_lanes ? l0 + l : 0;
          const int64_t off = (int64_t)ll * a.ld;
          zp[l] = a.zprev[off + j];
          zz[l] = a.z[off + j];
          aa[l] = a.a0[off + j];
          bb[l] = a.b0[off + j];
          gg[l] = a.g[(int64_t)ll * (a.ld + 16) + j];
        }
#pragma unroll
        for (int l = 0; l < 16; ++l) {
          if (l0 + l >= a.n_lanes || !lane_live[l0 + l]) continue;
          if (!in_w && had_w && zz[l] != zp[l]) n_miss += 1;
          if (zp[l] != 0.0) {
            sc = inf;
          } else {
            const double thr = lane_sa[l0 + l] * aa[l] + lane_sb[l0 + l] * bb[l];
            sc = fmax(sc, thr > 0.0 ? fabs(gg[l]) / thr : inf);
          }
        }
      }
      if (sc >= w.theta && !in_w) n_new += 1;
      w.score[it] = sc;
    }
  } else {
    static_assert(SLM_MAX_LANES % 16 == 0, "16-thread teams: a thread per (group, lane of a half)");
    const int l16 = tid & 15;
    const bool have = it < nitems;  // (a team is all in or all out)
    double sc = 0.0;
    bool in_w = false;
    int k0 = 0, k1 = 0;
    if (have) {
      k0 = a.gstart[it];
      k1 = a.gstart[it + 1];
      in_w = had_w && w.pos[a.order[k0]] >= 0;
    }
    for (int l = l16; have && l < a.n_lanes; l += 16) {  // (a call of thirty-two lanes: two lanes per thread)
      if (lane_live[l]) {
        const int64_t off = (int64_t)l * a.ld;
        const double* g = a.g + (int64_t)l * (a.ld + 16);
        double num = 0.0, rmax = 0.0;
        bool act = false;
        for (int k = k0; k < k1; ++k) {
          const int j = a.order[k];
          const double zp = a.zprev[off + j], zj = a.z[off + j], aj = a.a0[off + j], gj = g[j];  // (one round of loads)
          if (!in_w && had_w && zj != zp) n_miss += 1;
          act = act || zp != 0.0;
          const double thr = lane_sa[l] * aj;
          const double m = fmax(fabs(gj) - thr, 0.0);
          num = __builtin_fma(m, m, num);
          rmax = fmax(rmax, thr > 0.0 ? fabs(gj) / thr : inf);
        }
        const double den = lane_sb[l] * a.b0[off + it];
        const double r = den > 0.0 ? sqrt(num) / den : rmax;
        sc = fmax(sc, act ? inf : r);
      }
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) sc = fmax(sc, __shfl_xor(sc, o, 64));
    if (have && l16 == 0) {
      if (sc >= w.theta && !in_w) n_new += k1 - k0;
      w.score[it] = sc;
    }
  }
  // integer counts: the order of the atomic additions does not matter
  if (n_new) atomicAdd(&cnt[0], n_new);
  if (n_miss) atomicAdd(&cnt[1], n_miss);
  __syncthreads();
  if (tid == 0) {
    if (cnt[0]) atomicAdd(&ws->sweep_new, cnt[0]);
    if (cnt[1]) atomicAdd(&ws->sweep_miss, cnt[1]);
  }
}

static __global__ __launch_bounds__(256) void ws_score_kernel(TailArgs a, WsArgs w) { ws_score_body(a, w, (int)blockIdx.x); }

// ---------------------------------------------------------------------------------------------
// (i-b) choose W.  One workgroup.  Runs after ws_score_kernel in every pass; returns at once unless a
// build was requested, a lane's plain step left the current W, or there are newcomers.  With a valid W the newcomers are
// APPENDED (their columns and Gram rows are all that has to be produced); a fresh selection is made
// at the start of a solve and when the appended set would exceed WS_KCAP.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void ws_select_body(TailArgs a, WsArgs w) {
  __shared__ double red[2][TAIL_WAVES];
  __shared__ int wave_tot[TAIL_WAVES];
  WsCtl* ws = w.ws;
  // `served` is this pass's: set again by the model solver (launched behind this kernel) for the lanes it moves.  Left
  // standing from pass to pass, the flags of the last pass the working set served everyone made the FIRST round on the
  // model Gram sit out -- a whole pass over X between the overflow and the first proposal.
  if (threadIdx.x < SLM_MAX_LANES) ws->served[threadIdx.x] = 0;
  if (a.gdone[0] != 0 || ws->disabled) return;
  const int tid = threadIdx.x;
  const int p = a.p, G = a.G;
  const bool singleton = a.singleton != 0;
  const int nitems = singleton ? p : G;
  const bool had_w = ws->valid != 0;

  if (tid == 0 && ws->hard_next) ws->hard = 1;
  const bool requested = ws->request != 0;
  if (!requested && !had_w) return;
  if (ws->builds >= ws->max_builds || ws->appends >= 8 * ws->max_builds) {
    // budget spent: keep the W we have; lanes whose plain step leaves it iterate plainly (ws_solve_kernel
    // checks that per lane once `stale` is set)
    if (tid == 0) {
      ws->request = 0;
      ws->stale = 1;
    }
    return;
  }

  // scores and the two counts come from ws_score_kernel (many workgroups, launched just before)
  double sweep[2] = {(double)ws->sweep_new, (double)ws->sweep_miss};
  const bool carried = ws->carried != 0;  // (first selection of a solve on its predecessor's W)
  __syncthreads();
  if (tid == 0) {
    ws->sweep_new = 0;
    ws->sweep_miss = 0;
    ws->carried = 0;
  }
  const double inf = __builtin_huge_val();
  const bool miss = had_w && sweep[1] != 0.0;
  if (miss && tid == 0) ws->misses += 1;
  if (had_w && !requested && sweep[0] == 0.0) {
    // no newcomer (the usual pass).  A lane that left W anyway cannot be helped: it iterates plainly.
    if (miss && tid == 0) ws->stale = 1;
    return;
  }

  // This thread's items (a contiguous run of `per`), read ONCE: score, feature count and whether the item sits in
  // W already.  Up to eight items per thread (p <= 8192) they live in registers -- the counting sweeps below (up to
  // fifteen of them when a threshold is fitted) and the position pass at the end then touch no memory; item by item
  // every sweep was a chain of dependent round trips (29 us for this kernel on the headline path).
  const int per = (nitems + WS_THREADS - 1) / WS_THREADS;
  const int i0 = tid * per, i1 = min(i0 + per, nitems);
  const bool cached = per <= 8;
  double c_sc[8];
  int c_sz[8];
  bool c_inw[8];
  if (cached) {
    int first[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int it = (i0 + u < i1) ? i0 + u : 0;
      c_sc[u] = (i0 + u < i1) ? w.score[it] : -1.0;  // (below every threshold: an item that is not there is never taken)
      first[u] = singleton ? it : a.gstart[it];
      c_sz[u] = singleton ? 1 : a.gstart[it + 1] - first[u];
    }
    if (!singleton) {
#pragma unroll
      for (int u = 0; u < 8; ++u) first[u] = a.order[first[u]];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) c_inw[u] = w.pos[first[u]] >= 0;
  }

  // feature count of the items with score >= thr (optionally only those not yet in W), and the
  // largest finite score
  auto count_at = [&](double thr, bool only_new, double* n_sel, double* smax) {
    double v[2] = {0.0, 0.0};
    if (cached) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (c_sc[u] >= thr && !(only_new && c_inw[u])) v[0] += (double)c_sz[u];
        if (c_sc[u] < inf) v[1] = fmax(v[1], c_sc[u]);
      }
    } else {
      for (int it = tid; it < nitems; it += WS_THREADS) {
        const double sc = w.score[it];
        const int first = singleton ? it : a.order[a.gstart[it]];
        const int size = singleton ? 1 : a.gstart[it + 1] - a.gstart[it];
        if (sc >= thr && !(only_new && w.pos[first] >= 0)) v[0] += (double)size;
        if (sc < inf) v[1] = fmax(v[1], sc);
      }
    }
    double s[1] = {v[0]};
    block_sum<1>(s, red);
    *n_sel = s[0];
    if (smax == nullptr) return;  // (only the first count of a fitted threshold asks for it: two barriers less for the others)
    double m = v[1];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    __syncthreads();
    if ((tid & 63) == 0) red[1][tid >> 6] = m;
    __syncthreads();
    double mm = 0.0;
#pragma unroll
    for (int k = 0; k < TAIL_WAVES; ++k) mm = fmax(mm, red[1][k]);
    *smax = mm;
  };

  // smallest threshold >= thr0 whose selection has at most `cap` features (scores >= it are kept)
  auto fit_threshold = [&](double thr0, bool only_new, double cap, double* n_out) -> double {
    double n_sel, smax;
    count_at(thr0, only_new, &n_sel, &smax);
    if (n_sel <= cap) {
      *n_out = n_sel;
      return thr0;
    }
    double lo = thr0, hi = fmax(smax, thr0) * (1.0 + 1e-12) + 1e-300;  // count(hi) = non-zeros only
    double n_hi = 0.0;
    for (int k = 0; k < 14; ++k) {
      const double mid = 0.5 * (lo + hi);
      count_at(mid, only_new, &n_sel, nullptr);
      if (n_sel > cap) {
        lo = mid;
      } else {
        hi = mid;
        n_hi = n_sel;
        if (n_sel >= w.fill * cap) break;  // close enough to the cap
      }
    }
    if (n_hi == 0.0) count_at(hi, only_new, &n_hi, nullptr);
    *n_out = n_hi;
    return hi;
  };

  double n_sel, smax, thr = w.theta;
  const int k_old = had_w ? ws->Kreal : 0;
  bool append = had_w;
  if (append) {
    // newcomers: at most w.append_max per pass, the likeliest first (a feature left out that enters
    // anyway shows up as a miss and is appended then)
    // (a lane is stuck: be generous; the first selection of a solve that took over its predecessor's W: as many as a
    //  fresh selection would take -- appended columns cost their own gather and Gram rows only)
    // (how generous, by how far the lanes left W: a path whose supports outgrow W in waves -- dozens of coordinates a pass --
    //  takes the full factor; ONE lane that met a feature or two at the deep end of a sparse path takes a single append_max:
    //  at four it pulled 150 candidates that never entered into every later Gram and model solve, 0.2-0.3 ms per path on
    //  three of nine draws of the headline's law, tools/ab_knobs_draws.py)
    const int miss_mult = miss ? min(w.miss_factor, 1 + (int)sweep[1] / max(w.miss_div, 1)) : 1;
    const double cap = (double)(carried ? max(w.k_init, 4 * w.append_max) : miss_mult * w.append_max);
    if (sweep[0] <= cap) {
      n_sel = sweep[0];
    } else {
      thr = fit_threshold(w.theta, true, cap, &n_sel);
    }
    if (n_sel == 0.0) {  // (requested with a valid W and nothing to add)
      if (tid == 0) ws->request = 0;
      return;
    }
    if ((double)k_old + n_sel > (double)WS_KCAP) {  // does not fit: select afresh
      if (tid == 0) ws->outgrown += 1;
      if (w.keep_full) {
        // the model-Gram rounds serve what W does not cover.  Where the non-zeros of the live lanes alone fill most of
        // the capacity -- a path whose solutions are outgrowing the set for good -- a fresh selection would be outgrown
        // again a pass later (gather + Gram of 500 columns, 2-3 ms a time): W stays as it is.  Where they do not -- W is
        // full of candidates that never entered, the way strongly correlated designs fill it -- the selection goes ahead
        // as it always did: those lanes are best served by W's own model solver and its direct steps.
        double nz_now;
        count_at(inf, false, &nz_now, nullptr);
        if (nz_now > 0.75 * (double)WS_KCAP) {
          if (tid == 0) {
            ws->request = 0;
            ws->stale = 1;
          }
          return;
        }
      }
      append = false;
      thr = w.theta;
    }
  }
  if (!append) {
    count_at(inf, false, &n_sel, nullptr);
    if (n_sel > (double)WS_KCAP) {
      // the non-zero coefficients of the expansion points alone do not fit (dense early iterates of
      // a cold start, a dense solution, or ONE lane whose plain steps went dense): with a W in place it
      // stays -- the lanes it still serves keep refining, the ones that left it iterate plainly (`stale`);
      // without one, try again after the next pass and give up after 50 tries
      if (tid == 0) {
        ws->overflows += 1;
        ws->outgrown += 1;
        if (had_w) {
          ws->request = 0;
          ws->stale = 1;
        } else {
          ws->request = 1;
          ws->valid = 0;
          if (ws->overflows >= 50) ws->disabled = 1;
        }
      }
      return;
    }
    const double nonzeros = n_sel;
    thr = fit_threshold(w.theta, false, fmax((double)w.k_init, nonzeros), &n_sel);
    for (int j = tid; j < p; j += WS_THREADS) w.pos[j] = -1;
  }
  for (int k = k_old * (append ? 1 : 0) + tid; k < WS_KCAP; k += WS_THREADS) {
    w.idx[k] = -1;
    w.gs[k] = k;
    w.gl[k] = 1;
  }
  __syncthreads();

  // ---- positions: items in index order, members of a group contiguous -----------------------------
  // which of this thread's items are taken (decided before pos[] is written below), and their feature count
  unsigned long long pick = 0ull;
  int mine = 0;
  if (cached) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (c_sc[u] >= thr && !(append && c_inw[u])) {
        pick |= 1ull << u;
        mine += c_sz[u];
      }
    }
  } else {
    for (int it = i0; it < i1 && it - i0 < 64; ++it) {
      if (!(w.score[it] >= thr)) continue;
      if (append && w.pos[singleton ? it : a.order[a.gstart[it]]] >= 0) continue;
      pick |= 1ull << (it - i0);
      mine += singleton ? 1 : a.gstart[it + 1] - a.gstart[it];
    }
  }
  int total = 0;
  int at = (append ? k_old : 0) + block_excl_scan(mine, wave_tot, &total);
  __syncthreads();
  for (int it = i0; it < i1 && it - i0 < 64; ++it) {
    if (!((pick >> (it - i0)) & 1ull)) continue;
    if (singleton) {
      w.idx[at] = it;
      w.pos[it] = at;
      at += 1;
    } else {
      const int k0 = a.gstart[it], len = a.gstart[it + 1] - k0;
      for (int m = 0; m < len; ++m) {
        const int j = a.order[k0 + m];
        w.idx[at + m] = j;
        w.pos[j] = at + m;
        w.gs[at + m] = at;
        w.gl[at + m] = len;
      }
      at += len;
    }
  }
  if (tid == 0) {
    const int Kreal = (append ? k_old : 0) + total;
    ws->Kreal = Kreal;
    ws->K = max(16, (Kreal + 15) & ~15);
    ws->k_new = append ? k_old : 0;
    ws->building = 1;
    ws->valid = 0;
    ws->stale = 0;
    ws->counter = 0;
    if (append) {
      ws->appends += 1;
    } else {
      ws->builds += 1;
      for (int l = 0; l < SLM_MAX_LANES; ++l) ws->Lw[l] = 0.0;
    }
  }
}

static __global__ __launch_bounds__(WS_THREADS) void ws_select_kernel(TailArgs a, WsArgs w) { ws_select_body(a, w); }

// ---------------------------------------------------------------------------------------------
// (ii) gather the new columns: XW[i][k] = X[i][idx[k]] for k >= k_new (0 for padding positions).
// Read from the column-major copy XT, where the 32 rows of a tile of a column are contiguous, through a 32 x 32 LDS
// tile, so reads and writes both move 256-byte segments.  (Gathering from the row-major X touches one 64-byte
// sector per element: 0.2 ms for 112 columns, 0.5 ms per 50-alpha path.)  grid (row tiles, 16 column
// tiles of 32 starting at k_new); tiles beyond K return at once.
//
// XTY (the build behind the pass on a row sample, (ii-b) below): the pass that moves a value also holds it in a register
// next to its row, so the linear term of the model comes out of it -- every thread sums x * y[i] for its four columns over
// the row tiles it walks, in the order of its grid-stride loop; the 32 row lanes of a column are folded by shuffles (xor
// 16, 8, 4, 2, 1: a fixed tree), and row lane 0 writes part[blockIdx.x][k], one partial per (row block, position).  The
// column tile blockIdx.y == 0 does the same for y[i]^2 into part[blockIdx.x][WS_KCAP].  No LDS beyond the tile, no
// atomics.  A pad position (idx < 0) and a row past n read nothing and add zeros.  The tiles start at position 0 whatever
// k_new is (the selection behind a sample pass is a fresh one; the diagnostic call may ask at an append, and then the old
// columns are written again with the values they hold), so every position below K has its partial in every row block.
// The plain gather (XTY = false, ws_gather_kernel) is the kernel as it was: the extra code is compiled out.
// ---------------------------------------------------------------------------------------------
template <bool XTY>
__device__ __forceinline__ void ws_gather_body(const WsArgs& w, const double* __restrict__ y, double* __restrict__ part) {
  if (!w.ws->building) return;
  const int K = w.ws->K;
  const int k0 = (XTY ? 0 : w.ws->k_new) + 32 * (int)blockIdx.y;
  if (k0 >= K) return;
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const int64_t row_tiles = (w.n + 31) / 32;
  // the four columns this thread reads in every row tile: looked up once (inside the loop every load of X waited
  // for the index load before it)
  int jcol[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int k = k0 + ty + 8 * u;
    jcol[u] = k < K ? w.idx[k] : -1;
  }
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  double yy = 0.0;
  const bool yy_tile = XTY && blockIdx.y == 0;
  for (int64_t rt = blockIdx.x; rt < row_tiles; rt += gridDim.x) {
    const int64_t i0 = rt * 32;
    const int64_t i = i0 + tx;
    double v[4];
    double yi = 0.0;
    if (XTY) yi = i < w.n ? y[i] : 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // read: lanes walk rows i (contiguous in XT)
      const int j = jcol[u];
      // (XT == nullptr: no memory for the column-major copy -- same tile, sector-granular reads from X)
      v[u] = (j >= 0 && i < w.n) ? (w.XT ? w.XT[((rt * w.ld + j) << 5) + tx] : w.X[i * w.ld + j]) : 0.0;
    }
    if (XTY) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = __builtin_fma(v[u], yi, acc[u]);
      if (yy_tile) yy = __builtin_fma(yi, yi, yy);
    }
    __syncthreads();  // the tile of the previous round has been written out
#pragma unroll
    for (int u = 0; u < 4; ++u) tile[ty + 8 * u][tx] = v[u];
    __syncthreads();
    for (int ii = ty; ii < 32; ii += 8) {  // write: lanes walk positions k (contiguous in XW)
      const int64_t i = i0 + ii;
      const int k = k0 + tx;
      if (i < w.n && k < K) w.XW[i * WS_KCAP + k] = tile[tx][ii];
    }
  }
  if (XTY) {
    // (a wavefront holds two values of ty, 32 row lanes each: the xor offsets below 32 stay inside a half)
#pragma unroll
    for (int off = 16; off >= 1; off >>= 1) {
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] += __shfl_xor(acc[u], off, 64);
      if (yy_tile) yy += __shfl_xor(yy, off, 64);  // (uniform for the workgroup)
    }
    double* out = part + (int64_t)blockIdx.x * (WS_KCAP + 1);
    if (tx == 0) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int k = k0 + ty + 8 * u;
        if (k < K) out[k] = acc[u];
      }
      if (yy_tile && ty == 0) out[WS_KCAP] = yy;
    }
  }
}
static __global__ __launch_bounds__(256) void ws_gather_kernel(WsArgs w) { ws_gather_body<false>(w, nullptr, nullptr); }
static __global__ __launch_bounds__(256) void ws_gather_xty_kernel(WsArgs w, const double* y, double* part) { ws_gather_body<true>(w, y, part); }

// ---------------------------------------------------------------------------------------------
// (ii-b) A path that opened on a row sample (solve_core, "sample start"): the gradient at zero the first call worked
// with is an estimate -- good enough to choose W, not to build the model on.  On W the exact one is c_k = -X_k^T y / n, and
// the loss at zero is y^T y / 2n.  The partial sums over row blocks are a by-product of the gather (ws_gather_xty_kernel);
// ws_xty_apply_kernel folds them and the sums go into g and gprev of every lane (all lanes stand at zero), the loss into
// g[ld], the first entry of the objective history and PathCtl::loss_base.  No row weights (the caller checks).
// A dataset without the column-major copy (XT == nullptr) keeps the launch of its own for the partial sums,
// ws_xty_partial_kernel, one more read of the gathered columns: its gather is bound by the sector-granular reads of X, ten
// times the time of the other, and is left as it is.  The partials of both have one layout, and the apply is the same.
// ---------------------------------------------------------------------------------------------
struct XtyArgs {
  const WsCtl* ws;
  const int32_t* idx;
  const double* XW;
  const double* y;
  double* part;     // [nblk][WS_KCAP + 1]: per block the sums of every position and, last, of y^2
  double* g;        // [lanes][ld + 16]
  double* gprev;    // [lanes][ld]
  double* z;        // [lanes][ld]: the model solves start from zero on W (the candidate of the first call is a step along the estimate)
  PathCtl* ctl;
  const int* done;
  int64_t n, ld;
  double inv_n;
  int n_lanes, nblk;
};
static __global__ __launch_bounds__(512) void ws_xty_partial_kernel(XtyArgs a) {
  if (*a.done) return;
  __shared__ double red[8][WS_KCAP];
  __shared__ double red_yy[8];
  const int K = a.ws->K;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t rows = (a.n + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * rows, i1 = i0 + rows < a.n ? i0 + rows : a.n;
  // a wavefront per row (rows i0 + wave, + 8, ...), a lane per position of each chunk of 64: the loads of a row are one
  // contiguous segment, and eight rows are in flight per workgroup
  double acc[WS_KCAP / 64];
#pragma unroll
  for (int c = 0; c < WS_KCAP / 64; ++c) acc[c] = 0.0;
  double yy = 0.0;
  // The number of 64-column chunks is settled ONCE, outside the row loop, and the loads of four rows are issued together (a
  // position past K reads position 0 of its chunk and counts with a factor of zero).  With the chunk test inside the loop the
  // compiler kept one row in flight: 82 us at 384 columns where this takes 48, 22 -> 15 at 96 (tools/probes/xty_probe.hip).
  auto rows4 = [&](auto NC) {
    constexpr int C = decltype(NC)::value;
    for (int64_t i = i0 + wave; i < i1; i += 32) {
      double xv[4][C], yv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool in = i + 8 * r < i1;
        const int64_t ii = in ? i + 8 * r : i;
        yv[r] = in ? a.y[ii] : 0.0;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const int k = lane + 64 * c;
          xv[r][c] = a.XW[ii * WS_KCAP + (k < K ? k : 64 * c)];
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        yy = __builtin_fma(yv[r], yv[r], yy);
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = __builtin_fma(lane + 64 * c < K ? xv[r][c] : 0.0, yv[r], acc[c]);
      }
    }
  };
  switch ((K + 63) >> 6) {
    case 1: rows4(std::integral_constant<int, 1>{}); break;
    case 2: rows4(std::integral_constant<int, 2>{}); break;
    case 3: rows4(std::integral_constant<int, 3>{}); break;
    case 4: rows4(std::integral_constant<int, 4>{}); break;
    case 5: rows4(std::integral_constant<int, 5>{}); break;
    case 6: rows4(std::integral_constant<int, 6>{}); break;
    case 7: rows4(std::integral_constant<int, 7>{}); break;
    default: rows4(std::integral_constant<int, 8>{}); break;
  }
  static_assert(WS_KCAP / 64 == 8, "eight chunks of 64 positions");
#pragma unroll
  for (int c = 0; c < WS_KCAP / 64; ++c) red[wave][lane + 64 * c] = acc[c];
  if (lane == 0) red_yy[wave] = yy;
  __syncthreads();
  double* out = a.part + (int64_t)blockIdx.x * (WS_KCAP + 1);
  const int k = threadIdx.x;
  if (k < K) {
    double sum = 0.0;
#pragma unroll
    for (int w = 0; w < 8; ++w) sum += red[w][k];
    out[k] = sum;
  }
  if (k == WS_KCAP - 1) {
    double sum = 0.0;
#pragma unroll
    for (int w = 0; w < 8; ++w) sum += red_yy[w];
    out[WS_KCAP] = sum;
  }
}
// grid: WS_KCAP / 16 workgroups of 512 threads -- 16 positions each (128 bytes of a row of partials), 32 threads per position
// that take every thirty-second row block, eight loads in flight each: at most 1 024 row blocks (slm_host::xty_part_rows) are
// four rounds of loads per thread.  (Four workgroups of 128 positions x 4 threads walked 512 blocks in sixteen rounds: 16 us.)
// The 32 slices of a position are added in order; so are the blocks' sums of y^2, by workgroup 0.
static __global__ __launch_bounds__(512) void ws_xty_apply_kernel(XtyArgs a) {
  if (*a.done || !a.ws->building) return;  // (no build under way: the gather has left no partial sums)
  __shared__ double red[32][17];
  __shared__ double ry[512];
  const int K = a.ws->K;
  const int kl = threadIdx.x & 15, q = threadIdx.x >> 4;
  const int k = (int)blockIdx.x * 16 + kl;
  if ((int)blockIdx.x * 16 >= K) return;  // (uniform for the workgroup)
  double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (k < K) {
    int b = q;
    for (; b + 224 < a.nblk; b += 256) {
#pragma unroll
      for (int u = 0; u < 8; ++u) s[u] += a.part[(int64_t)(b + 32 * u) * (WS_KCAP + 1) + k];
    }
    for (; b < a.nblk; b += 32) s[0] += a.part[(int64_t)b * (WS_KCAP + 1) + k];
  }
  red[q][kl] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  if (blockIdx.x == 0) {
    double t = 0.0;
    for (int b = threadIdx.x; b < a.nblk; b += 512) t += a.part[(int64_t)b * (WS_KCAP + 1) + WS_KCAP];
    ry[threadIdx.x] = t;
  }
  __syncthreads();
  if (q == 0 && k < K) {
    const int j = a.idx[k];
    if (j >= 0) {
      double t = 0.0;
#pragma unroll
      for (int w = 0; w < 32; ++w) t += red[w][kl];
      const double c = -t * a.inv_n;
      for (int l = 0; l < a.n_lanes; ++l) {
        a.g[(int64_t)l * (a.ld + 16) + j] = c;
        a.gprev[(int64_t)l * a.ld + j] = c;
        a.z[(int64_t)l * a.ld + j] = 0.0;
      }
    }
  }
  if (blockIdx.x == 0) {  // the loss at zero: the row blocks' sums of y^2, folded in a fixed order
    for (int off = 256; off >= 1; off >>= 1) {
      if ((int)threadIdx.x < off) ry[threadIdx.x] += ry[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x < (unsigned)a.n_lanes) {
      const int l = threadIdx.x;
      const double loss0 = 0.5 * ry[0] * a.inv_n;
      a.g[(int64_t)l * (a.ld + 16) + a.ld] = loss0;
      a.ctl[l].hist[0] = loss0;  // (the penalty at zero is zero)
      a.ctl[l].loss_base = loss0;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// (iii) partial Grams with v_mfma_f64_16x16x4_f64.  Grid (nblk, n_sets); 8 wavefronts per
// workgroup laid out 4 x 2, each owning a 4 x 4 block of 16x16 output tiles, so a workgroup covers
// 256 x 128 of the 512 x 512 capacity at a time and walks the slices that exist (2 row halves x 4 column
// quarters; see the loop over `slice`).  16 accumulator tiles = 128 registers per lane, which is why
// it is not one 1024-thread workgroup.  Only the tile
// rows that hold new positions (I >= k_new / 16) are computed; the reduce kernel mirrors them into
// the columns.  Operand maps (guide "Fragment layout"): lane l holds A[i = l & 15][k = l >> 4] and
// B[k = l >> 4][j = l & 15]; result register r of lane l is D[row (l >> 4) + 4 r][col l & 15].  Here
// k runs over 4 consecutive rows of XW, A[i][k] = w_k XW[row_k][16 I + i], B[k][j] = XW[row_k][16 J + j].
// ---------------------------------------------------------------------------------------------
// Row masks of a CV grid are ones except on their fold's test rows, and with contiguous folds (KFold as scikit-learn makes
// it) most row blocks of the Gram kernel see ALL ONES in most sets and ALL ZEROS in one: the partial Gram of such a block is
// the same matrix for every all-ones set (computed once, by the first of them) and nothing for an all-zeros set.
// owner[set][b]: the set whose partial the reduce kernel adds for (set, b) -- the set itself where its weights on the block
// are mixed (or it is the first all-ones set there), -1 where they are all zeros.  Two masks in a call: one read of the
// gathered columns instead of two (an eighth of config 4: 0.35 -> 0.15 ms per pass).  One workgroup per row block.
static __global__ __launch_bounds__(256) void ws_block_owner_kernel(const double* rw, int64_t rw_stride, WsArgs w, int32_t* owner) {
  __shared__ int cls[SLM_MAX_LANES];  // 0: all zeros, 1: all ones, 2: anything else
  __shared__ int red[2][4];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int64_t base = w.n / w.nblk, rem = w.n % w.nblk;
  const int64_t r0 = b * base + (b < rem ? b : rem);
  const int64_t nrows = base + (b < rem ? 1 : 0);
  for (int st = 0; st < w.n_sets; ++st) {
    const double* v = rw + (int64_t)w.set_lane[st] * rw_stride + r0;
    int zeros = 1, ones = 1;
    for (int64_t i = tid; i < nrows; i += 256) {
      const double x = v[i];
      zeros &= (x == 0.0);
      ones &= (x == 1.0);
    }
    zeros = __all(zeros);
    ones = __all(ones);
    if ((tid & 63) == 0) {
      red[0][tid >> 6] = zeros;
      red[1][tid >> 6] = ones;
    }
    __syncthreads();
    if (tid == 0) {
      const int z = red[0][0] & red[0][1] & red[0][2] & red[0][3], o = red[1][0] & red[1][1] & red[1][2] & red[1][3];
      cls[st] = z ? 0 : (o ? 1 : 2);
    }
    __syncthreads();
  }
  if (tid == 0) {
    int first_ones = -1;
    for (int st = 0; st < w.n_sets; ++st) {
      int o = st;
      if (cls[st] == 0) o = -1;
      else if (cls[st] == 1) {
        if (first_ones < 0) first_ones = st;
        o = first_ones;
      }
      owner[(int64_t)st * w.nblk + b] = o;
    }
  }
}

typedef double ws_d4 __attribute__((ext_vector_type(4)));
constexpr int WS_GRAM_THREADS = 512;
constexpr int WS_GRAM_ZCHUNKS = 4;  // slices of a row block: 4 column quarters x this many chunks of tile rows

// The products of one wavefront in one slice: rows [s_begin, s_end) of the block at row r0, NTI x NTJ output tiles from
// tile row `ibase` and tile column 4 wj.  HAS_RW and the tile counts are template parameters so that the loop body is
// ONE basic block -- loads, then MFMAs, no condition anywhere -- in which the compiler counts the loads exactly.
//
// Four register sets; the loads of three steps (twelve rows) stay in flight behind the MFMAs of a step.  A set is the
// NTI + NTJ operand loads the products need (eight for 4 x 4 tiles; the runtime tile pattern used to read eight whatever
// it needed, three of them from column blocks past K on a one-tile-row append), with the row weight as one more and LAST
// load where there are weights: the weight scales A, so the first MFMA of a step waits for its whole set at once.  Every
// wait in the compiled loop is exact: it leaves the three younger sets outstanding -- 3 (NTI + NTJ [+ 1]) loads, vmcnt(24)
// to vmcnt(31) for 4 x 4 tiles -- and none reaches into a younger set (profiles/gram_pipeline/isa_waits.txt).  A step
// beyond the wavefront's rows reads row 0 of the block with weight zero, so the prologue and the last iteration need no
// conditions either; the prologue sits under the same test as the do-while, in its preheader, so that it issues its sets in
// the order the back edge leaves them in (under a `for` its loads were sunk past the loop's entry test and reordered, and
// the loop head took the stricter count: vmcnt(11), (19)).  The sched_barriers keep the loads that open a step above its
// MFMAs and the select of a set's weight next to them: in one loop with the tile pattern as branches the compiler had
// moved the first step's MFMAs above the fourth set's loads and sunk the selects of all in-flight weights to the back
// edge, which drained the pipeline once per sixteen rows (vmcnt 3, 2, 10, 9).  The products are accumulated in row order
// whatever the depth.
template <bool HAS_RW, int NTI, int NTJ>
static __device__ __forceinline__ void ws_gram_rows(const double* __restrict__ XW, const double* __restrict__ rw, int64_t r0, int64_t s_begin,
                                                    int64_t s_end, int ibase, int wj, int kk, int c, ws_d4 (&acc)[4][4]) {
  auto load = [&](int64_t s, double(&av)[4], double(&bv)[4], double& wv) {
    const int64_t i = s + kk;
    const int64_t row = r0 + (i < s_end ? i : 0);
    const double* xr = XW + row * WS_KCAP + c;
#pragma unroll
    for (int t = 0; t < NTI; ++t) av[t] = xr[16 * (ibase + t)];
#pragma unroll
    for (int t = 0; t < NTJ; ++t) bv[t] = xr[16 * (4 * wj + t)];
    if constexpr (HAS_RW) wv = rw[row];
    __builtin_amdgcn_sched_barrier(0);
  };
  auto mma = [&](int64_t s, const double(&av)[4], const double(&bv)[4], double wv) {
    const bool ok = s + kk < s_end;
    const double wgt = ok ? (HAS_RW ? wv : 1.0) : 0.0;
#pragma unroll
    for (int ti = 0; ti < NTI; ++ti) {
      const double a = av[ti] * wgt;
#pragma unroll
      for (int tj = 0; tj < NTJ; ++tj) acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv[tj], acc[ti][tj], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  double a0[4], b0[4], a1[4], b1[4], a2[4], b2[4], a3[4], b3[4], w0 = 1.0, w1 = 1.0, w2 = 1.0, w3 = 1.0;
  if (s_begin >= s_end) return;  // (a row part without rows)
  load(s_begin, a0, b0, w0);
  load(s_begin + 4, a1, b1, w1);
  load(s_begin + 8, a2, b2, w2);
  int64_t s = s_begin;
  do {
    load(s + 12, a3, b3, w3);
    mma(s, a0, b0, w0);
    load(s + 16, a0, b0, w0);
    mma(s + 4, a1, b1, w1);
    load(s + 20, a1, b1, w1);
    mma(s + 8, a2, b2, w2);
    load(s + 24, a2, b2, w2);
    mma(s + 12, a3, b3, w3);
    s += 16;
  } while (s < s_end);
}

template <bool HAS_RW>
static __global__ __launch_bounds__(WS_GRAM_THREADS) void ws_gram_kernel(WsArgs w) {
  if (!w.ws->building) return;
  __shared__ ws_d4 comb[2][16][64];  // 64 KiB: row-split appends fold their four parts through here
  const int K = w.ws->K;
  const int tile_lo = w.ws->k_new >> 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles = K >> 4;
  // An append touches at most four tile rows.  With the usual mapping only the wavefronts whose tile
  // rows those are would work (2 of 8, 98 dependent steps each: 0.13 ms of latency); instead the four
  // wavefront pairs split the ROWS of the block between them, all on the new tile rows, and fold
  // their accumulators through LDS in a fixed order.
  // Larger appends (a miss quadruples the cap) are cut into chunks of four tile rows, one per value of
  // slice >> 2 below, each handled the same way (up to 16 new tile rows = 256 columns; the generic
  // mapping left most wavefronts idle on them: 0.44 ms for 170 new columns).
  // (a small fresh selection -- the first 112 columns of a path: 7 x 7 tiles -- keeps half of the wavefronts of ONE
  //  workgroup per row block busy under the usual mapping, each walking all rows of the block: 90 us; split by rows
  //  like an append it is eight wavefronts of two workgroups on a quarter of the rows each)
  const bool row_split = (tile_lo > 0 || tiles <= 8) && tiles - tile_lo <= 4 * WS_GRAM_ZCHUNKS;
  const int set = blockIdx.y;
  const int64_t b = blockIdx.x;
  if (w.owner != nullptr && w.owner[(int64_t)set * w.nblk + b] != set) return;  // (all zeros here, or another set's partial serves)
  const int64_t base = w.n / w.nblk, rem = w.n % w.nblk;
  const int64_t r0 = b * base + (b < rem ? b : rem);
  const int64_t nrows = base + (b < rem ? 1 : 0);
  const double* rw = HAS_RW ? w.rw + (int64_t)w.set_lane[set] * w.rw_stride : nullptr;
  // rows of this wavefront: everything, or the part-th quarter (in steps of four rows)
  const int part = row_split ? (wave >> 1) : 0;
  const int64_t steps = (nrows + 3) >> 2;
  const int64_t s_begin = row_split ? 4 * (steps * part / 4) : 0;
  const int64_t s_end = row_split ? min(nrows, 4 * (steps * (part + 1) / 4)) : nrows;

  // The (column quarter, chunk of tile rows) slices of this row block, one after the other in ONE workgroup.  As
  // grid.z they were sixteen workgroups per row block of which an append on the headline path needs two: the other
  // fourteen still had to be started, each holding the CU's registers and 64 KB of its LDS until it had read the
  // control block and left -- half of the kernel's 67 us.
  for (int slice = 0; slice < 4 * WS_GRAM_ZCHUNKS; ++slice) {
  const int zhi = slice >> 2;
  if (8 * (slice & 3) >= tiles) continue;  // (no column of this quarter exists)
  if (row_split ? (tile_lo + 4 * zhi >= tiles) : (zhi >= 2)) continue;
  const int wj = 2 * (slice & 3) + (wave & 1);
  const int ntj = min(4, max(0, tiles - 4 * wj));
  const int irow = row_split ? tile_lo + 4 * zhi : 4 * (4 * zhi + (wave >> 1));  // the four tile rows of this wavefront
  const int ibase = max(tile_lo, irow);  // (the first of them to do: tile_lo where the plain mapping straddles it on an append)
  const int nti = max(0, min(tiles, irow + 4) - ibase);
  const bool active = nti > 0 && ntj > 0;
  if (!row_split && !active) continue;  // (per wavefront: this mode has no barrier)
  ws_d4 acc[4][4];
#pragma unroll
  for (int ti = 0; ti < 4; ++ti)
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) acc[ti][tj] = ws_d4{0.0, 0.0, 0.0, 0.0};

  const int kk = lane >> 4, c = lane & 15;
  if (active) {
#define WS_GRAM_ROWS(I, J) \
  case 4 * (I - 1) + (J - 1): ws_gram_rows<HAS_RW, I, J>(w.XW, rw, r0, s_begin, s_end, ibase, wj, kk, c, acc); break;
    switch (4 * (nti - 1) + (ntj - 1)) {  // (uniform for the wavefront)
      WS_GRAM_ROWS(1, 1) WS_GRAM_ROWS(1, 2) WS_GRAM_ROWS(1, 3) WS_GRAM_ROWS(1, 4)
      WS_GRAM_ROWS(2, 1) WS_GRAM_ROWS(2, 2) WS_GRAM_ROWS(2, 3) WS_GRAM_ROWS(2, 4)
      WS_GRAM_ROWS(3, 1) WS_GRAM_ROWS(3, 2) WS_GRAM_ROWS(3, 3) WS_GRAM_ROWS(3, 4)
      WS_GRAM_ROWS(4, 1) WS_GRAM_ROWS(4, 2) WS_GRAM_ROWS(4, 3) WS_GRAM_ROWS(4, 4)
    }
#undef WS_GRAM_ROWS
  }
  if (row_split) {  // parts 0..3 in order: store, add + store, add + store, add (and write below)
    for (int round = 0; round < 4; ++round) {
      if (part == round && active) {
#pragma unroll
        for (int ti = 0; ti < 4; ++ti)
#pragma unroll
          for (int tj = 0; tj < 4; ++tj) {
            if (ti < nti && tj < ntj) {
              if (round > 0) acc[ti][tj] += comb[wave & 1][ti * 4 + tj][lane];
              if (round < 3) comb[wave & 1][ti * 4 + tj][lane] = acc[ti][tj];
            }
          }
      }
      __syncthreads();
    }
  }
  if (!row_split || (part == 3 && active)) {
  // partials are stored tile by tile, the row blocks of one tile next to each other:
  // part[set][tile (I, J)][b][16 x 16] -- the reduce kernel then walks 2 KiB strides, not 2 MiB ones
#pragma unroll
  for (int ti = 0; ti < 4; ++ti) {
    if (ti >= nti) continue;
#pragma unroll
    for (int tj = 0; tj < 4; ++tj) {
      if (tj >= ntj) continue;
      const int64_t tile = (int64_t)(ibase + ti) * WS_TILES + (4 * wj + tj);
      double* out = w.part + (((int64_t)set * (WS_TILES * WS_TILES) + tile) * w.nblk + b) * 256;
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(kk + 4 * r) * 16 + c] = acc[ti][tj][r];
    }
  }
  }
  if (row_split) __syncthreads();  // (the fold buffer is used again by the next slice)
  }
}

// fixed-order sum of the partial Grams, scaled by 1/n_set: the new tile rows and, mirrored, the
// matching columns of the old part.  One workgroup per 16x16 tile (grid (WS_TILES^2, n_sets)); the
// last workgroup publishes the Gram.
static __global__ __launch_bounds__(256) void ws_gram_reduce_kernel(WsArgs w) {
  WsCtl* ws = w.ws;
  if (!ws->building) return;
  const int K = ws->K;
  const int row_lo = (ws->k_new >> 4) << 4;
  const int set = blockIdx.y;
  const int tile = blockIdx.x, I = tile / WS_TILES, J = tile % WS_TILES;
  const int tiles = K >> 4, I_lo = row_lo >> 4;
  if (I < I_lo || I >= tiles || J >= tiles) return;  // (only the working tiles take part in the count below)
  const int i = 16 * I + (threadIdx.x >> 4), j = 16 * J + (threadIdx.x & 15);
  {
    const double* src = w.part + (((int64_t)set * (WS_TILES * WS_TILES) + tile) * w.nblk) * 256 + threadIdx.x;
    // four interleaved chains, 32 loads in flight per thread (the loop is latency-bound); the order
    // of additions is fixed, so the result is reproducible
    double s4[4] = {0.0, 0.0, 0.0, 0.0};
    int b = 0;
    if (w.owner != nullptr) {
      // row blocks whose partial another set computed (ws_block_owner_kernel), or nobody (all rows weigh zero): the same
      // sum in the same order, every term from where it lies.  Offsets of the blocks' partials relative to this set's.
      __shared__ int64_t off_s[512];
      static_assert(sizeof(off_s) >= 8 * 512, "nblk <= 512");
      for (int bb = threadIdx.x; bb < w.nblk; bb += 256) {
        const int o = w.owner[(int64_t)set * w.nblk + bb];
        off_s[bb] = o < 0 ? -1 : (int64_t)(o - set) * (WS_TILES * WS_TILES) * w.nblk * 256;
      }
      __syncthreads();
      for (; b + 32 <= w.nblk; b += 32) {
        double v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) {
          const int64_t o = off_s[b + u];
          v[u] = o == -1 ? 0.0 : src[(int64_t)(b + u) * 256 + o];
        }
#pragma unroll
        for (int u = 0; u < 32; ++u) s4[u & 3] += v[u];
      }
      for (; b < w.nblk; ++b) {
        const int64_t o = off_s[b];
        s4[b & 3] += o == -1 ? 0.0 : src[(int64_t)b * 256 + o];
      }
    }
    for (; b + 32 <= w.nblk; b += 32) {
      double v[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) v[u] = src[(int64_t)(b + u) * 256];
#pragma unroll
      for (int u = 0; u < 32; ++u) s4[u & 3] += v[u];
    }
    for (; b < w.nblk; ++b) s4[b & 3] += src[(int64_t)b * 256];
    double s = ((s4[0] + s4[1]) + (s4[2] + s4[3])) * w.inv_n[set];
    double* Gs = (w.Gx ? w.Gx : w.Gm) + (int64_t)set * (WS_KCAP * WS_KCAP);
    Gs[i * WS_KCAP + j] = s;
    if (j < row_lo) Gs[j * WS_KCAP + i] = s;
  }
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = (tiles - I_lo) * tiles * (int)gridDim.y;
    if (atomicAdd(&ws->counter, 1) + 1 == total) {
      ws->counter = 0;
      if (w.Gx) {
        ws->staged = 1;  // this rank's rows only: all-reduce, then ws_publish_kernel
      } else {
        ws->request = 0;
        ws->valid = 1;
        __threadfence();
        ws->building = 0;
      }
    }
  }
}

// Row-sharded mode: after the all-reduce of the staging matrix, move the new rows / columns into the
// Gram and publish it.  grid (WS_PUBLISH_BLOCKS, n_sets): a workgroup walks its share of the K x K corner (as 1 024
// workgroups over the whole 512 x 512 matrix, each with its turn at the one counter, the kernel took 62 us).
constexpr int WS_PUBLISH_BLOCKS = 64;
static __global__ __launch_bounds__(256) void ws_publish_kernel(WsArgs w) {
  WsCtl* ws = w.ws;
  if (!ws->building || !ws->staged) return;
  const int K = ws->K;
  const int row_lo = (ws->k_new >> 4) << 4;
  const int set = blockIdx.y;
  // rows of the corner, WS_KCAP doubles apart; a wavefront moves 64 consecutive columns of one row
  for (int i = blockIdx.x; i < K; i += gridDim.x)
    for (int j = threadIdx.x; j < K; j += 256)
      if (i >= row_lo || j >= row_lo) {
        const int64_t at = (int64_t)set * (WS_KCAP * WS_KCAP) + (int64_t)i * WS_KCAP + j;
        w.Gm[at] = w.Gx[at];
      }
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    const int total = gridDim.x * gridDim.y;
    if (atomicAdd(&ws->counter, 1) + 1 == total) {
      ws->counter = 0;
      ws->staged = 0;
      ws->request = 0;
      ws->valid = 1;
      __threadfence();
      ws->building = 0;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Hold-out scoring of sparse coefficient vectors (grid searches): gather the union of their supports
// once (<= WS_KCAP columns, same tiled gather as above, explicit arguments), then one thread per row
// computes up to SSE_M residuals from K contiguous doubles.  A dense evaluation costs a pass over X
// per four vectors; this costs n x K doubles per sixteen.
// ---------------------------------------------------------------------------------------------
constexpr int SSE_M = 16;

struct GatherArgs {
  const double* X;
  const double* XT;  // nullptr: read the row-major X
  int64_t n, ld;
  const int32_t* idx;  // [K] columns (all >= 0)
  int K;               // multiple of 16 is not required
  double* XW;          // [n][WS_KCAP]
};

static __global__ __launch_bounds__(256) void gather_cols_kernel(GatherArgs w) {
  const int k0 = 32 * (int)blockIdx.y;
  if (k0 >= w.K) return;
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t row_tiles = (w.n + 31) / 32;
  for (int64_t rt = blockIdx.x; rt < row_tiles; rt += gridDim.x) {
    const int64_t i0 = rt * 32;
    __syncthreads();
    for (int kk = ty; kk < 32; kk += 8) {
      const int k = k0 + kk;
      const int j = k < w.K ? w.idx[k] : -1;
      const int64_t i = i0 + tx;
      tile[kk][tx] = (j >= 0 && i < w.n) ? (w.XT ? w.XT[((rt * w.ld + j) << 5) + tx] : w.X[i * w.ld + j]) : 0.0;
    }
    __syncthreads();
    for (int ii = ty; ii < 32; ii += 8) {
      const int64_t i = i0 + ii;
      const int k = k0 + tx;
      if (i < w.n && k < w.K) w.XW[i * WS_KCAP + k] = tile[tx][ii];
    }
  }
}

struct SseArgs {
  const double* XW;  // [n][WS_KCAP]
  const double* y;
  const double* rw;  // nullptr: ones
  const double* Zs;  // [m][K] coefficients on the gathered columns
  double* partial;   // [gridDim.x][SSE_M]
  int64_t n;
  int K, m;          // m <= SSE_M vectors in this launch
};

static __global__ __launch_bounds__(256) void sse_sparse_kernel(SseArgs a) {
  extern __shared__ double zs[];  // [K][SSE_M]
  __shared__ double wsum[4][SSE_M];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < a.K * SSE_M; e += 256) {
    const int k = e / SSE_M, v = e - k * SSE_M;
    zs[e] = v < a.m ? a.Zs[(int64_t)v * a.K + k] : 0.0;
  }
  __syncthreads();
  double sse[SSE_M];
#pragma unroll
  for (int v = 0; v < SSE_M; ++v) sse[v] = 0.0;
  for (int64_t row = (int64_t)blockIdx.x * 256 + tid; row < a.n; row += (int64_t)gridDim.x * 256) {
    const double w = a.rw ? a.rw[row] : 1.0;
    if (w == 0.0) continue;  // (a fold mask: four fifths of the rows)
    const double* xr = a.XW + row * WS_KCAP;
    double dot[SSE_M];
#pragma unroll
    for (int v = 0; v < SSE_M; ++v) dot[v] = 0.0;
    for (int k = 0; k < a.K; ++k) {
      const double x = xr[k];
#pragma unroll
      for (int v = 0; v < SSE_M; ++v) dot[v] = __builtin_fma(x, zs[k * SSE_M + v], dot[v]);
    }
    const double yi = a.y[row];
#pragma unroll
    for (int v = 0; v < SSE_M; ++v) {
      const double e = dot[v] - yi;
      sse[v] = __builtin_fma(w * e, e, sse[v]);
    }
  }
#pragma unroll
  for (int v = 0; v < SSE_M; ++v) {
    double t = sse[v];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) t += __shfl_xor(t, off, 64);
    if (lane == 0) wsum[wave][v] = t;
  }
  __syncthreads();
  if (tid < SSE_M) a.partial[(int64_t)blockIdx.x * SSE_M + tid] = wsum[0][tid] + wsum[1][tid] + wsum[2][tid] + wsum[3][tid];
}

}  // namespace slm
