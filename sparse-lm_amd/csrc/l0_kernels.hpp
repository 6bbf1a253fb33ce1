// Exact l0 estimators (the reference's mixed-integer family: BestSubsetSelection, RidgedBestSubsetSelection, RegularizedL0,
// L2L0 -- src/sparselm/model/_miqp/_best_subset.py, _regularized_l0.py) by a depth-first search over supports on chip.
//
//     minimise over supports S (sets of groups) and beta, supp beta in cols(S), |beta_j| <= big_M:
//         1/2 beta^T H beta - c^T beta + alpha |S|        H = G + 2 eta T,  G = X^T X / n,  c = X^T y / n
//     subject to |S| <= K and i in S => need[i] in S
//
// The host hands over H, c and the groups in SEARCH ORDER (a group's columns contiguous, groups by descending
// ||c_g||^2 / tr G_gg).  One wavefront owns one subtree at a time: the subtrees are the 2^d include / exclude prefixes of
// the first d = min(groups, 16) groups, handed out by a ticket counter.  Inside a wave lane r holds row r of the Cholesky
// factor L of H on the included columns (in registers: every index into the row is a compile-time constant, the loops over
// its entries are unrolled and guarded by the wave-uniform column count) and entry r of w = L^-1 c.  Including a group
// appends its columns by a column-oriented forward substitution -- one cross-lane broadcast per step; excluding one costs
// nothing; backtracking is lowering the column count.  The quadratic value of a support is -1/2 ||w||^2, so a node is
// evaluated without a back-substitution.
//
// Pruning, all exact: cardinality; hierarchy (an included group needs an excluded one); and the bound
// q_all + alpha (|S| + 1) >= incumbent for everything below a node, q_all the unconstrained value on all columns -- the
// quadratic part is monotone in the support, so no descendant (which includes at least one more group) can be below it.
// A column whose pivot is <= 1e-12 of its diagonal depends on the included ones and cannot lower the value: it is skipped
// (its coefficient is 0) and the rest of its group goes on -- what makes n < p, duplicated columns and centred one-hot groups
// safe.  A group that brings NO column leaves the value where it was and costs a slot (and alpha): its include branch is
// dropped unless some other group needs it -- every support with it is matched by the same support without it.
//
// The incumbent is shared through a 64-bit atomic min on an order-preserving integer image of the double; every wave also
// keeps its own best (value, support), and the host picks the winner from those in a fixed order, so the result does not
// depend on which wave met it first.  Only a candidate that would beat the incumbent is back-substituted; if it leaves the
// box its value comes from cyclic coordinate descent with clipping on its own block of H, stopped at a relative change of
// L0_CD_TOL per sweep -- the host values its seed by the same descent, so boxed supports are compared like with like.  A global node counter is
// bumped in batches; past max_nodes every wave drains and exits.  Every loop is bounded.
//
// l1 mode (template parameter L1, slm_solve_l0_l1: the reference's L1L0): eta_l1 ||beta||_1 joins the objective, so a support's
// value f(S) is a lasso inside the box.  f is monotone in the support and f(S) >= q(S) = -1/2 ||w||^2, so the register
// Cholesky stays as an exact lower-bound FILTER: only a node whose q(S) + alpha |S| is <= the incumbent and better than the
// wave's own best runs the descent -- the cyclic one of the boxed case with a soft-threshold in the update -- and its value
// is what the descent reaches.  The descent runs over ALL columns of the support, the ones the pivot rule skipped
// included: with an l1 term a column equal to a + b replaces two coefficients by one, so a dependent column CAN lower the
// value, and the cut of a group that brought no independent column is off.  The subtree bound takes a proven lower bound
// on f(all columns) from the host in q_all (the lasso dual value at a feasible point, or q_all itself).
//
// profile mode (template parameter PROFILE, slm_solve_l0_profile; with L1: see "l1 profile" below): ONE search returns, for every
// size k = 1 .. K, the best admissible support of exactly k groups -- the table Q_k that answers best subset for every bound
// K' <= K (min_{k <= K'} Q_k) and RegularizedL0 / L2L0 for every alpha (min_k Q_k + alpha k).  Lane k - 1 of a wave keeps the
// wave's best (value, support) of size k and the shared incumbent of that size, read from an array of 64 keys behind the
// control words (one coalesced load per refresh, one atomic min per improvement).  A node of cnt groups is a candidate for
// entry cnt alone, valued without an alpha term; the tie rule is the one above, per size.  a.alpha holds alpha_min, and the
// subtree bound becomes  q_all + alpha_min (cnt + 1) >= E(cnt),  E(c) = min(0, min_{1 <= k <= c} Qinc_k + alpha_min k)
// (l0_profile_term / l0_profile_join of l0_host.hpp, a prefix-min over the lanes at every refresh): every support S' below
// the node has k' >= cnt + 1 groups and q(S') >= q_all, so for the minimising k* <= cnt and any alpha >= alpha_min
//     Qinc_k* + alpha k* <= q_all + alpha_min (cnt + 1) + (alpha - alpha_min) k* <= q(S') + alpha k'
// -- S' is never strictly better than a support already held.  With alpha_min = 0 the cut fires only where a held support
// has reached q_all, and the table is the full one.
//
// wide mode (template parameter WIDE, slm_solve_l0_wide / slm_solve_l0_profile_wide; with L1 only as the l1 profile below): up to
// L0_WIDE_PMAX = 128 columns and groups.  The factor is indexed by inclusion position, not by column, so it keeps its 64 rows
// and a support draws its at most 64 INDEPENDENT columns from any of the 128.  What differs, all under if constexpr (WIDE) or
// behind the mask type: H sits in LDS as a packed lower triangle (row i at i (i + 1) / 2: 66 048 B at 128 columns, so two
// workgroups still share a CU); every mask is two 64-bit words (L0Mask128 of l0_host.hpp, ordered as a 128-bit integer); lane
// g & 63 holds the state before group g was decided in slot g >> 6, the slot picked by a wave-uniform branch.  Capacity: an
// independent column that arrives when the factor holds 64 rows REFUSES its group's include -- the state is restored as for
// any refused include and the exclude branch is taken.  The wave keeps the smallest cnt at which it refused one and lowers
// the control word L0_CAPACITY with cnt + 1 on exit: every support below such a refusal has at least cnt + 1 groups and
// q >= q_all, so nothing unsearched is below q_all + alpha (c_min + 1) -- the host proves optimality against that.
//
// l1 profile (template parameters L1 and PROFILE together, slm_solve_l0_l1_profile; with WIDE slm_solve_l0_l1_profile_wide): for one
// fixed eta_l1 the value f(S) of a support depends on neither alpha nor the size, so the table F_k = min_{|S| = k} f(S) answers L1L0 at
// EVERY alpha (min_k F_k + alpha k).  The two modes compose as they stand.  A node of cnt groups is a candidate for row cnt alone: the
// filter compares q(S) = -1/2 ||w||^2 <= f(S) with that size's incumbent and the wave's best of that size, the descent's value goes
// into the table without an alpha term, and the subtree cut is the profile's with bound_all, the host's proven lower bound on
// f(all columns), in q_all:  bound_all + alpha_min (cnt + 1) >= E(cnt).  The argument of profile mode carries over word for word
// with f for q: f is monotone in the support, so every S' below the node has f(S') >= f(all) >= bound_all and k' >= cnt + 1 groups.
// The lasso zeroes coefficients by itself, so the table saturates: from the size that holds every column the lasso on all
// columns uses, larger sizes tie in value and the tie rule (the smaller mask) picks their supports.  WIDE: the descent reads H
// through Hat (the packed triangle), st_na gets its second slot beside st_m1 / st_ss1, and lane r still stands for the r-th
// column of the support -- the host refuses a call whose max_groups largest groups hold more than 64 columns, so a support's
// column list (dependent columns included) fits the lanes; an include that would take it past 64 is refused all the same and
// lowers L0_CAPACITY, which the host reports as an internal error.  There is no plain wide l1 search: it would need a dynamic
// capacity rule on the column list.  230 (narrow) / 250 (wide) VGPRs, no AGPRs, no scratch, 34 056 / 69 640 B of LDS, 2 waves/SIMD;
// measured in profiles/l1l0_profile.txt.
//
// constrained mode (template parameter CON, slm_solve_l0_constrained; alone): rows lo <= A beta <= hi and a per-column box
// blo_j <= beta_j <= bhi_j join the problem, so f(S) is a quadratic programme, +inf on an infeasible support.  f is monotone in
// the support and f(S) >= q(S), so the register Cholesky stays an exact lower-bound FILTER as in l1 mode, and a node that
// passes it is valued by the splitting of l0_host.hpp (l0_con_solve is this code on the host): lane r < m keeps beta_r and
// (H beta - c)_r, lane i < rows keeps (A beta)_i, s_i and u_i; a sweep is the clipped coordinate descent with the row term
// rho A_k^T (A beta - s + u) from one wave sum per coordinate, then s <- clip(A beta + u), u <- A beta + u - s.  Every sweep ends
// with the dual value D_S(rho u, mu) <= f(S) -- one forward substitution with the factor the wave holds -- lowered by its
// rounding margin: the candidate is VALUED when its rows hold and its value meets D to L0_CON_TOL, REJECTED when D is above
// what it has to beat (the incumbent, or the wave's best under the tie rule; an infeasible support's D grows past every
// feasible value), and UNSETTLED when the sweep cap runs out -- D + alpha |S| then goes into the control word L0_UNSETTLED by
// one atomic min, a lower bound on that one support, and the search below goes on.  H is positive definite on all columns
// (the host refuses the call otherwise), so no column is skipped and the cut of a group that brought none is off; q_all is
// the host's proven lower bound on f(all columns).  A lives in LDS beside H, column by column with a padded stride.
//
// exclusion bound (template parameter XB, slm_solve_l0_xb / slm_solve_l0_xb_wide; with WIDE or alone): the subtree bound becomes
// q(all \ E) + alpha (|S| + 1) >= incumbent, E the columns of the groups the path has excluded -- every support below the node
// avoids them and q is monotone.  With P = H^-1 and bhat = P c from the host (l0_excl_plan of l0_host.hpp),
//     q(all \ E) = q_all + 1/2 ||w'||^2,   w' = L'^-1 bhat_E,   L' L'^T = P_EE,
// and E grows in the order of the decisions, so L' grows by the SAME append as L (L0_APPEND below), on P and bhat in LDS in
// H's layout: lane r keeps row r of L' in a second register row of L0_XCAP entries with 1 / L'[r][r] and w'_r, the wave keeps
// the column count mx and ssx = ||w'||^2, lane g (wide: slot g >> 6) saves both from before group g was decided beside st_m and
// st_ss, and every exclude -- back from an include, a forced 0 bit of the ticket, a refused include, a group that brought no
// column -- restores them and appends the group's columns.  A column whose pivot is <= L0_PIVOT P_jj is left out, and so is every
// column once mx == L0_XCAP: a sub-collection of E gives a valid, weaker bound.  Includes do not touch L'.  What is compared
// is l0_excl_bound (l0_host.hpp): the increment lowered by the margin delta the host derived from the conditioning of H.
// LDS: 67 336 B narrow, 136 712 B wide (one workgroup per CU); 256 VGPRs + 80 / 103 AGPRs at L0_XCAP = 64, no scratch, 1 wave/SIMD.
// Measured in profiles/l0_bound.txt, L0_XCAP = 32 beside it (256 + 19 / 41 registers, also 1 wave/SIMD: the same time on the 25-row
// problems, more nodes and more time on the reference's 290 x 66 data).  Not measured: the time one wavefront walks alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "l0_host.hpp"  // L0_PMAX, L0_CD_SWEEPS, L0_CD_TOL, L0_PIVOT: shared with the host side

namespace slm {

constexpr int L0_WAVES = 4;        // wavefronts per workgroup (they share H in LDS and nothing else)
constexpr int L0_PREFIX = 16;      // groups decided by the ticket
constexpr int L0_BATCH = 256;      // nodes between two bumps of the global counter
// control words (unsigned 64-bit each), zeroed / seeded by the host before the launch
constexpr int L0_TICKET = 0, L0_INCUMBENT = 1, L0_NODES = 2, L0_STOP = 3, L0_ABORTED = 4, L0_DESCENTS = 5, L0_CAPACITY = 6, L0_UNSETTLED = 7,
              L0_UNSETTLED_COUNT = 8, L0_BATCH_QALL = 9, L0_BATCH_ETA = 10, L0_CTL_WORDS = 11;
// (L0_BATCH_QALL, batched profile only: the bits of the problem's own q_all, written by the host and only read on the device)
// (L0_BATCH_ETA, batched l1 profile only: the bits of the problem's own l1 weight, written by the host and only read on the device)
// (L0_CAPACITY, wide mode only: seeded with all ones, lowered to c_min + 1 by a wave that refused an include for capacity)
// (L0_UNSETTLED, constrained mode only: seeded with all ones, lowered to the key of D + alpha |S| by a wave whose candidate ran
//  out of sweeps; L0_UNSETTLED_COUNT counts them.  L0_DESCENTS counts the candidates valued in l1 and constrained mode.)
constexpr int L0_CON_LD = L0_CON_MMAX + 1;  // the stride of a column of A in LDS (odd: lanes that read different columns spread over the banks)
// profile mode: the incumbents of the sizes 1 .. 64 (keys, seeded by the host) follow the control words
constexpr int L0_PROFILE_INC = L0_CTL_WORDS, L0_PROFILE_WORDS = L0_CTL_WORDS + L0_PMAX;

struct L0Args {
  const double* H;                  // [p][p] G + 2 eta T, search order
  const double* c;                  // [p]
  const long long* gstart;          // [ng + 1] first column of each group
  const unsigned long long* need;   // [ng] groups (search order) each group depends on; wide mode: [ng][2], low word first
  unsigned long long* ctl;          // [L0_CTL_WORDS]; profile mode: [L0_PROFILE_WORDS]
  double* best_val;                 // [waves of the grid]; profile mode: [waves][64], entry k - 1 for size k
  unsigned long long* best_mask;    // [waves of the grid]; profile mode: [waves][64]; wide mode: two words each, low word first
  int p, ng, d, K;
  double alpha, big_M, q_all;       // (q_all: the proven lower bound on the value of ALL columns the subtree bound uses;
                                    //  profile mode: alpha is alpha_min)
  long long max_nodes;
  double eta_l1;                    // l1 mode only: the weight of ||beta||_1
  // constrained mode only
  const double* A;                  // [p][rows] column by column: A[j * rows + i], rows of unit norm, search order
  const double* lo;                 // [rows]
  const double* hi;                 // [rows]
  const double* blo;                // [p] the box, blo_j <= 0 <= bhi_j
  const double* bhi;                // [p]
  int rows, con_sweeps;
  double rho;
  // exclusion bound only
  const double* P;                  // [p][p] H^-1, search order
  const double* bhat;               // [p] P c
  double xb_delta;                  // the relative margin of the increment (l0_excl_bound)
  // batched profile only: the pointers above are problem 0's, problem b's lie b * batch_stride words further on
  long long batch_stride;           // 8-byte words from one problem's copy of the block to the next
  int batch_blocks;                 // workgroups per problem: problem b owns the workgroups b * batch_blocks .. (b + 1) * batch_blocks - 1
};

// order-preserving image of a double in an unsigned 64-bit integer (and back)
static __host__ __device__ inline unsigned long long l0_key(double v) {
  unsigned long long b;
  __builtin_memcpy(&b, &v, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
static __host__ __device__ inline double l0_unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v;
  __builtin_memcpy(&v, &b, 8);
  return v;
}

static __device__ __forceinline__ double l0_bcast(double v, int k) {  // lane k's value (k wave-uniform)
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), k);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), k);
  return __hiloint2double(hi, lo);
}
static __device__ __forceinline__ double l0_wave_sum(double v) {  // the same bits in every lane
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
static __device__ __forceinline__ unsigned long long l0_bcast(unsigned long long v, int k) {
  return ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(v >> 32), k) << 32) | (unsigned)__builtin_amdgcn_readlane((int)v, k);
}
static __device__ __forceinline__ L0Mask128 l0_bcast(L0Mask128 v, int k) { return L0Mask128{l0_bcast(v.lo, k), l0_bcast(v.hi, k)}; }
static __device__ __forceinline__ double l0_wave_max(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}

// The append both factors run: x = L^-1 b by columns (b: lane r holds the new column's entry against the column lane r stands
// for), x_k broadcast from lane k at step k and written into lane m's row; s2 = ||x||^2 and sw = x^T w come back.  Every index
// into the register row is a compile-time constant; the steps are guarded by the wave-uniform column count m.  (A macro, not
// a function: a register row handed to a function by reference left the six older instantiations with other register
// counts; expanded in place they keep theirs.)
#define L0_APPEND(CAP, row, invd, w, m, b, s2, sw)    \
  _Pragma("unroll") for (int k = 0; k < (CAP); ++k) { \
    if (k < (m)) {                                    \
      const double xk = l0_bcast((b) * (invd), k);    \
      s2 = fma(xk, xk, s2);                           \
      sw = fma(xk, l0_bcast(w, k), sw);               \
      b = fma(-row[k], xk, b);                        \
      if (lane == (m)) row[k] = xk;                   \
    }                                                 \
  }

// H[i][j] as the l1 descent reads it: the narrow instantiations keep the expression they had (and with it their code), the wide
// one goes through Hat's packed triangle.  (WIDE is a template parameter: the branch not taken is not compiled into the kernel.)
#define L0_HL1(i, j) (WIDE ? Hat((i), (j)) : Hs[(i) * p + (j)])

// L1 = false: the search above.  L1 = true: eta_l1 ||beta||_1 joins the objective (see the head of the file).
// PROFILE = true: the best support of every size (see the head of the file); everything it adds sits under if constexpr.
// WIDE = true: up to 128 columns and groups (see the head of the file); what it adds sits under if constexpr or behind Mask.
// CON = true: linear constraints and a per-column box (see the head of the file); everything it adds sits under if constexpr.
// XB = true: the exclusion bound (see the head of the file); everything it adds sits under if constexpr.
// BATCH = true (slm_solve_l0_profile_batch, slm_solve_l0_profile_grid; narrow profile only, with or without L1): up to 16 problems
// (the grid entry: up to L0_GRID_MAX = 128, one per (row set, eta)) of one shape in one launch.  The block is
// `count` copies of the single-problem profile layout at a constant stride (l0_batch_layout of l0_host.hpp); a workgroup
// belongs to problem blockIdx.x / batch_blocks, moves every base pointer to that copy and numbers its waves within the
// problem.  Ticket counter, node counter, stop and aborted words, the 64 incumbents and q_all (L0_BATCH_QALL) are the copy's
// own, so a problem that runs out of its budget stops its own workgroups alone, and waves of different problems share no
// word: no new barrier, no new loop.  A workgroup whose problem has no ticket left exits (it is not moved to another
// problem: that would re-stage H behind a barrier).  With L1 the l1 weight is the copy's own too (L0_BATCH_ETA, read once per
// workgroup; a.eta_l1 stays what the other instantiations read), as L0_DESCENTS already is; q_all then holds the problem's l1
// bound.  Nothing waits on another workgroup, so a grid of more workgroups than the device holds at once runs in waves.
// Everything it adds sits under if constexpr.  L1 + PROFILE + BATCH: 231 VGPRs, no AGPRs, no scratch, 34 056 B of LDS, 2 waves/SIMD.
template <bool L1, bool PROFILE = false, bool WIDE = false, bool CON = false, bool XB = false, bool BATCH = false>
static __global__ __launch_bounds__(64 * L0_WAVES) void l0_search_kernel(L0Args a) {
  static_assert(!(L1 && WIDE) || PROFILE, "a wide l1 search exists only as a profile (a plain one needs a dynamic capacity rule on the support's column list)");
  static_assert(!(CON && (L1 || PROFILE || WIDE)), "the constrained mode stands alone");
  static_assert(!(XB && (L1 || PROFILE || CON)), "the exclusion bound serves the plain search, narrow and wide");
  static_assert(!(BATCH && (!PROFILE || WIDE || CON || XB)), "a batch holds narrow profile searches, with or without an l1 term, and nothing else");
  if constexpr (BATCH) {  // the workgroup's problem (wave-uniform): every base pointer moves to that problem's copy of the block
    const size_t at = (size_t)(blockIdx.x / (unsigned)a.batch_blocks) * (size_t)a.batch_stride;
    a.ctl += at;
    a.best_val += at;
    a.best_mask += at;
    a.H += at;
    a.c += at;
    a.need += at;
    a.gstart += at;
  }
  using Mask = std::conditional_t<WIDE, L0Mask128, unsigned long long>;
  constexpr int PM = WIDE ? L0_WIDE_PMAX : L0_PMAX;
  __shared__ double Hs[WIDE ? PM * (PM + 1) / 2 : PM * PM];  // (wide: the lower triangle, row i at i (i + 1) / 2)
  __shared__ double cs[PM];
  [[maybe_unused]] __shared__ double Ps[XB ? (WIDE ? PM * (PM + 1) / 2 : PM * PM) : 1];  // exclusion bound: P in H's layout, and bhat
  [[maybe_unused]] __shared__ double bhs[XB ? PM : 1];
  __shared__ Mask needs[PM];
  __shared__ int gs[PM + 1];
  // constrained mode: A by columns (column j at j * L0_CON_LD), the rows' bounds, the box, the curvature H_jj + rho ||A_j||^2
  [[maybe_unused]] __shared__ double As[CON ? L0_PMAX * L0_CON_LD : 1];
  [[maybe_unused]] __shared__ double los[CON ? L0_CON_MMAX : 1], his[CON ? L0_CON_MMAX : 1];
  [[maybe_unused]] __shared__ double blos[CON ? L0_PMAX : 1], bhis[CON ? L0_PMAX : 1], curvs[CON ? L0_PMAX : 1];
  const int tid = threadIdx.x, lane = tid & 63;
  const int p = a.p, ng = a.ng, d = a.d, K = a.K;
  [[maybe_unused]] const int rows = CON ? a.rows : 0;
  if constexpr (CON) {
    for (int e = tid; e < p * rows; e += 64 * L0_WAVES) {
      const int j = e / rows, i = e - j * rows;
      As[j * L0_CON_LD + i] = a.A[e];
    }
    for (int e = tid; e < rows; e += 64 * L0_WAVES) {
      los[e] = a.lo[e];
      his[e] = a.hi[e];
    }
    for (int e = tid; e < p; e += 64 * L0_WAVES) {
      double a2 = 0.0;
      for (int i = 0; i < rows; ++i) a2 = fma(a.A[e * rows + i], a.A[e * rows + i], a2);
      blos[e] = a.blo[e];
      bhis[e] = a.bhi[e];
      curvs[e] = a.H[e * p + e] + a.rho * a2;
    }
  }
  if constexpr (WIDE) {
    for (int e = tid; e < p * p; e += 64 * L0_WAVES) {
      const int i = e / p, j = e - i * p;
      if (j <= i) Hs[i * (i + 1) / 2 + j] = a.H[e];
    }
  } else {
    for (int e = tid; e < p * p; e += 64 * L0_WAVES) Hs[e] = a.H[e];
  }
  for (int e = tid; e < p; e += 64 * L0_WAVES) cs[e] = a.c[e];
  if constexpr (XB) {
    if constexpr (WIDE) {
      for (int e = tid; e < p * p; e += 64 * L0_WAVES) {
        const int i = e / p, j = e - i * p;
        if (j <= i) Ps[i * (i + 1) / 2 + j] = a.P[e];
      }
    } else {
      for (int e = tid; e < p * p; e += 64 * L0_WAVES) Ps[e] = a.P[e];
    }
    for (int e = tid; e < p; e += 64 * L0_WAVES) bhs[e] = a.bhat[e];
  }
  if constexpr (WIDE) {
    for (int e = tid; e < ng; e += 64 * L0_WAVES) needs[e] = L0Mask128{a.need[2 * e], a.need[2 * e + 1]};
  } else {
    for (int e = tid; e < ng; e += 64 * L0_WAVES) needs[e] = a.need[e];
  }
  for (int e = tid; e <= ng; e += 64 * L0_WAVES) gs[e] = (int)a.gstart[e];
  __syncthreads();  // (the only barrier: from here on the waves run on their own and leave when they are done)
  // H[i][j] (symmetric) from LDS
  auto Hat = [&](int i, int j) -> double {
    if constexpr (WIDE) {
      const int hi = i > j ? i : j, lo = i > j ? j : i;
      return Hs[hi * (hi + 1) / 2 + lo];
    } else {
      return Hs[i * p + j];
    }
  };

  [[maybe_unused]] auto Pat = [&](int i, int j) -> double {  // P[i][j] (symmetric) from LDS
    if constexpr (WIDE) {
      const int hi = i > j ? i : j, lo = i > j ? j : i;
      return Ps[hi * (hi + 1) / 2 + lo];
    } else {
      return Ps[i * p + j];
    }
  };

  const long long n_tickets = 1ll << d;
  const double alpha = a.alpha, big_M = a.big_M;
  double q_all = a.q_all;
  if constexpr (BATCH) q_all = __longlong_as_double((long long)a.ctl[L0_BATCH_QALL]);  // (the folds' c differ: so does the bound)
  [[maybe_unused]] double eta_own = 0.0;  // batched l1 profile: the problem's own l1 weight
  if constexpr (BATCH && L1) eta_own = __longlong_as_double((long long)a.ctl[L0_BATCH_ETA]);
  // lane r: row r of L (entries below the diagonal), 1 / L[r][r], w[r], the column it stands for
  double Lrow[L0_PMAX];
#pragma unroll
  for (int k = 0; k < L0_PMAX; ++k) Lrow[k] = 0.0;
  double invd = 0.0, w = 0.0;
  int mycol = 0;
  // exclusion bound: lane r holds row r of L' (P on the excluded columns), 1 / L'[r][r], w'[r] and the column it stands for;
  // mx columns, ssx = ||w'||^2 (wave-uniform), and what they were before group g was decided (lane g; wide: slot g >> 6)
  [[maybe_unused]] double Xrow[XB ? L0_XCAP : 1];
  [[maybe_unused]] double xinvd = 0.0, xw = 0.0, ssx = 0.0, st_ssx = 0.0, st_ssx1 = 0.0;
  [[maybe_unused]] int xcol = 0, mx = 0, st_mx = 0, st_mx1 = 0;
  [[maybe_unused]] const double xb_delta = XB ? a.xb_delta : 0.0;
  if constexpr (XB) {
#pragma unroll
    for (int k = 0; k < L0_XCAP; ++k) Xrow[k] = 0.0;
  }
  // l1 mode: lane r also stands for the r-th column of the SUPPORT (dependent ones included), na of them
  int acol = 0, na = 0, st_na = 0;
  [[maybe_unused]] int st_na1 = 0;  // (the second slot: wide only)
  long long descents_local = 0;
  [[maybe_unused]] long long unsettled_local = 0;
  // the state before group g was decided, held by lane g (wide: by lane g & 63, in slot g >> 6)
  int st_m = 0;
  double st_ss = 0.0;
  Mask st_need = l0m_none<Mask>();
  [[maybe_unused]] int st_m1 = 0;  // (the second slot: wide only)
  [[maybe_unused]] double st_ss1 = 0.0;
  [[maybe_unused]] Mask st_need1 = l0m_none<Mask>();
  [[maybe_unused]] int cap_min = 0x7fffffff;  // wide: the smallest cnt at which an include was refused because the factor was full
  auto saved_m = [&](int g) -> int {
    if constexpr (WIDE)
      if (g >= 64) return __builtin_amdgcn_readlane(st_m1, g - 64);
    return __builtin_amdgcn_readlane(st_m, g);
  };

  // (profile mode: these two and inc are per lane -- lane k - 1 holds size k -- and env is E(k) of the head of the file)
  double best_v = __builtin_inf();
  Mask best_mask = l0m_ones<Mask>();
  auto read_incumbent = [&]() {
    if constexpr (PROFILE)
      return l0_unkey(__hip_atomic_load(&a.ctl[L0_PROFILE_INC + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    else
      return l0_unkey(__hip_atomic_load(&a.ctl[L0_INCUMBENT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  };
  double inc = read_incumbent();
  double env = 0.0;
  auto envelope = [&]() {  // an inclusive prefix-min of Qinc_k + alpha_min k over the lanes, capped by 0 (the empty support)
    double v = l0_profile_term(inc, lane + 1, alpha);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const double t = __shfl_up(v, off);
      if (lane >= off) v = l0_profile_join(v, t);
    }
    env = l0_profile_join(0.0, v);
  };
  long long nodes_local = 0;
  int since_refresh = 0;
  Mask needed = l0m_none<Mask>();  // groups some other group depends on
  for (int g = 0; g < ng; ++g) l0m_or(needed, needs[g]);
  bool quit = false;

  for (long long round = 0; round <= n_tickets && !quit; ++round) {
    long long t = 0;
    unsigned long long stop = 0;
    if (lane == 0) {
      t = (long long)atomicAdd(&a.ctl[L0_TICKET], 1ull);
      stop = __hip_atomic_load(&a.ctl[L0_STOP], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    t = ((long long)__builtin_amdgcn_readfirstlane((int)(t >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)t);
    stop = (unsigned)__builtin_amdgcn_readfirstlane((int)stop);
    if (t >= n_tickets) break;
    if (stop) {  // (a ticket taken and not searched: the search is incomplete)
      if (lane == 0) atomicOr(&a.ctl[L0_ABORTED], 1ull);
      break;
    }
    inc = read_incumbent();
    if constexpr (PROFILE) envelope();
    int m = 0, cnt = 0, depth = 0;
    na = 0;
    double ss = 0.0;
    if constexpr (XB) {
      mx = 0;
      ssx = 0.0;
    }
    Mask incl = l0m_none<Mask>(), needm = l0m_none<Mask>();
    bool down = true;
    // every pass of this loop either descends one level, or climbs one, or turns an include into an exclude: at most
    // three passes per edge of a finite tree; the node budget ends it earlier
    for (;;) {
      int g;
      bool try_exclude = false;
      if (down) {
        bool stop_here;
        if constexpr (PROFILE)  // the subtree bound against E(cnt)
          stop_here = depth >= ng || cnt >= K || l0_profile_cut(q_all, alpha, cnt, cnt == 0 ? 0.0 : l0_bcast(env, cnt - 1));
        else if constexpr (XB)  // the subtree bound on everything not yet excluded
          stop_here = depth >= ng || cnt >= K || !(l0_excl_bound(q_all, ssx, xb_delta) + alpha * (double)(cnt + 1) < inc);
        else
          stop_here = depth >= ng || cnt >= K || !(q_all + alpha * (double)(cnt + 1) < inc);
        if (stop_here) {
          down = false;
          continue;
        }
        g = depth;
        const bool forced = g < d;
        const bool want = forced ? ((t >> g) & 1) != 0 : true;
        if constexpr (WIDE) {
          if (g < 64) {
            if (lane == g) {
              st_m = m;
              st_ss = ss;
              st_need = needm;
              if constexpr (L1) st_na = na;
              if constexpr (XB) {
                st_mx = mx;
                st_ssx = ssx;
              }
            }
          } else if (lane == g - 64) {
            st_m1 = m;
            st_ss1 = ss;
            st_need1 = needm;
            if constexpr (L1) st_na1 = na;
            if constexpr (XB) {
              st_mx1 = mx;
              st_ssx1 = ssx;
            }
          }
        } else if (lane == g) {
          st_m = m;
          st_ss = ss;
          st_need = needm;
          if constexpr (L1) st_na = na;
          if constexpr (XB) {
            st_mx = mx;
            st_ssx = ssx;
          }
        }
        bool ok = want;
        if (ok) ok = !l0m_any_outside(l0m_and(needs[g], l0m_below<Mask>(g)), incl);  // hierarchy: it needs a group that was excluded
        if (ok) {
          if (++nodes_local >= L0_BATCH) {  // the node budget
            unsigned long long flag = 0;
            if (lane == 0) {
              const unsigned long long total = atomicAdd(&a.ctl[L0_NODES], (unsigned long long)nodes_local) + (unsigned long long)nodes_local;
              if ((long long)total > a.max_nodes) atomicOr(&a.ctl[L0_STOP], 1ull);
              flag = __hip_atomic_load(&a.ctl[L0_STOP], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) | ((long long)total > a.max_nodes ? 1ull : 0ull);
            }
            nodes_local = 0;
            if (__builtin_amdgcn_readfirstlane((int)flag)) {
              if (lane == 0) atomicOr(&a.ctl[L0_ABORTED], 1ull);
              quit = true;
              break;
            }
          }
          const int c0 = __builtin_amdgcn_readfirstlane(gs[g]), c1 = __builtin_amdgcn_readfirstlane(gs[g + 1]);
          if constexpr (L1 && WIDE) {
            // lane r stands for the support's r-th column: a group that would take the list past 64 is refused like an include
            // the factor has no row for (the host refuses such a call before the launch: this only guards the lanes)
            if (na + (c1 - c0) > L0_PMAX) {
              ok = false;
              cap_min = cnt < cap_min ? cnt : cap_min;
            }
          }
          if constexpr (L1) {  // the support's own column list grows by the whole group
            if (lane >= na && lane < na + (c1 - c0)) acol = c0 + (lane - na);
            na += c1 - c0;
          }
          for (int j = c0; j < c1; ++j) {
            if constexpr (L1 && WIDE)
              if (!ok) break;
            // append column j: x = L^-1 H[cols, j] by columns, x_k broadcast from lane k at step k
            const double hjj = Hat(j, j);
            double b = lane < m ? Hat(j, mycol) : 0.0;  // (H is symmetric: the lanes read one row)
            double s2 = 0.0, sw = 0.0;
            L0_APPEND(L0_PMAX, Lrow, invd, w, m, b, s2, sw)
            const double piv = hjj - s2;
            if (piv > L0_PIVOT * hjj) {  // (otherwise the column depends on the included ones: it is skipped, its beta is 0)
              if constexpr (WIDE)
                if (m == L0_PMAX) {  // capacity: the factor is full, the include is refused (the exclude branch restores the state)
                  ok = false;
                  cap_min = cnt < cap_min ? cnt : cap_min;
                  break;
                }
              const double lmm = sqrt(piv), wm = (cs[j] - sw) / lmm;
              if (lane == m) {
                invd = 1.0 / lmm;
                w = wm;
                mycol = j;
              }
              ss = fma(wm, wm, ss);
              ++m;
            }
          }
          // a group that brought no column leaves the value where it was and costs a slot (and alpha): unless another
          // group needs it, every support with it is matched by the same support without it
          // (not with an l1 term: a column equal to a + b replaces two coefficients by one, and the value falls)
          // (nor with constraints: a dependent column moves A beta -- and H is positive definite there, none is skipped)
          if constexpr (!L1 && !CON)
            if (m == saved_m(g) && !l0m_test(needed, g)) ok = false;
        }
        if (ok) {
          l0m_set(incl, g);
          ++cnt;
          l0m_or(needm, needs[g]);
          depth = g + 1;
          // every node is a candidate; inside the prefix the ticket whose remaining bits are zero evaluates it
          const bool mine = depth >= d || (t >> depth) == 0;
          double val = -0.5 * ss + alpha * (double)cnt;
          // what the candidate has to beat: the incumbent and the wave's best -- in profile mode those of its size
          double inc_k = inc, best_k = best_v;
          Mask mask_k = best_mask;
          if constexpr (PROFILE) {
            val = -0.5 * ss;
            inc_k = l0_bcast(inc, cnt - 1);
            best_k = l0_bcast(best_v, cnt - 1);
            mask_k = l0_bcast(best_mask, cnt - 1);
          }
          if (mine && !l0m_any_outside(needm, incl) && val <= inc_k && (val < best_k || (val == best_k && l0m_less(incl, mask_k)))) {
            // back-substitution beta = L^-T w, row by row from the last: lane r contributes L[r][k] beta_r to entry k
            double beta = 0.0;
            [[maybe_unused]] bool settled = true;  // (constrained mode: the candidate was valued)
#pragma unroll
            for (int k = L0_PMAX - 1; k >= 0; --k) {
              if (k < m) {
                const double part = l0_wave_sum((lane > k && lane < m) ? Lrow[k] * beta : 0.0);
                if (lane == k) beta = (w - part) * invd;
              }
            }
            if constexpr (L1) {
              // the node's value is a lasso inside the box on ALL columns of the support: the same cyclic descent with a
              // soft-threshold, from the back-substituted beta (clipped; zero on the columns the pivot rule skipped).
              // Lane r keeps beta_r and the gradient entry (H beta - c)_r of the support's r-th column.
              ++descents_local;
              double eta1 = a.eta_l1;
              if constexpr (BATCH) eta1 = eta_own;
              double b1 = 0.0;
              for (int k = 0; k < m; ++k) {
                const int ck = __builtin_amdgcn_readlane(mycol, k);
                const double bk = l0_bcast(beta, k);
                if (lane < na && acol == ck) b1 = fmin(fmax(bk, -big_M), big_M);
              }
              double gr = lane < na ? -cs[acol] : 0.0;
              for (int k = 0; k < na; ++k) {
                const int ck = __builtin_amdgcn_readlane(acol, k);
                gr = fma(lane < na ? L0_HL1(ck, acol) : 0.0, l0_bcast(b1, k), gr);
              }
              for (int sweep = 0; sweep < L0_CD_SWEEPS; ++sweep) {
                double maxd = 0.0, maxb = 0.0;
                for (int k = 0; k < na; ++k) {
                  const int ck = __builtin_amdgcn_readlane(acol, k);
                  const double bk = l0_bcast(b1, k), gk = l0_bcast(gr, k);
                  const double nb = l0_l1_step(bk, gk, L0_HL1(ck, ck), eta1, big_M);
                  const double dk = nb - bk;
                  if (dk != 0.0) {
                    gr = fma(lane < na ? L0_HL1(ck, acol) : 0.0, dk, gr);
                    if (lane == k) b1 = nb;
                  }
                  maxd = fmax(maxd, fabs(dk));
                  maxb = fmax(maxb, fabs(nb));
                }
                if (maxd <= L0_CD_TOL * maxb || maxd == 0.0) break;
              }
              if constexpr (PROFILE)  // (the table holds f(S) itself: no alpha term)
                val = 0.5 * l0_wave_sum(lane < na ? b1 * (gr - cs[acol]) : 0.0) + eta1 * l0_wave_sum(lane < na ? fabs(b1) : 0.0);
              else
                val = 0.5 * l0_wave_sum(lane < na ? b1 * (gr - cs[acol]) : 0.0) + eta1 * l0_wave_sum(lane < na ? fabs(b1) : 0.0) +
                      alpha * (double)cnt;
            } else if constexpr (CON) {
              // the node's value is a quadratic programme: the splitting of l0_host.hpp (l0_con_solve, step for step) from the
              // back-substituted beta, clipped.  Lane r < m: beta_r and (H beta - c)_r; lane i < rows: (A beta)_i, s_i, u_i.
              ++descents_local;
              settled = false;
              const double rho = a.rho, half_ss = 0.5 * ss;
              const double bref = l0_wave_max(lane < m ? fabs(beta) : 0.0);
              const double blo = lane < m ? blos[mycol] : 0.0, bhi = lane < m ? bhis[mycol] : 0.0;
              const double rlo = lane < rows ? los[lane] : 0.0, rhi = lane < rows ? his[lane] : 0.0;
              beta = l0_con_clip(beta, blo, bhi);
              double gr = lane < m ? -cs[mycol] : 0.0, tt = 0.0, amax = 0.0;
              for (int k = 0; k < m; ++k) {
                const int ck = __builtin_amdgcn_readlane(mycol, k);
                const double bk = l0_bcast(beta, k), ak = lane < rows ? As[ck * L0_CON_LD + lane] : 0.0;
                gr = fma(lane < m ? Hat(ck, mycol) : 0.0, bk, gr);
                tt = fma(ak, bk, tt);
                amax = fmax(amax, fabs(ak));
              }
              val = __builtin_inf();
              // a row that is zero on the support and excludes 0: infeasible without a solve
              if (l0_wave_max(lane < rows && amax == 0.0 && (rlo > 0.0 || rhi < 0.0) ? 1.0 : 0.0) == 0.0) {
                double sv = l0_con_clip(tt, rlo, rhi), u = 0.0, bound = -__builtin_inf();
                bool rejected = false;
                for (int sweep = 0; sweep < a.con_sweeps; ++sweep) {
                  double maxb = bref;
                  for (int k = 0; k < m; ++k) {
                    const int ck = __builtin_amdgcn_readlane(mycol, k);
                    const double ak = lane < rows ? As[ck * L0_CON_LD + lane] : 0.0;
                    const double pen = l0_wave_sum(ak * (tt - sv + u));
                    const double bk = l0_bcast(beta, k), gk = l0_bcast(gr, k);
                    const double nb = l0_con_step(bk, gk + rho * pen, curvs[ck], blos[ck], bhis[ck]);
                    const double dk = nb - bk;
                    if (dk != 0.0) {
                      gr = fma(lane < m ? Hat(ck, mycol) : 0.0, dk, gr);
                      tt = fma(ak, dk, tt);
                      if (lane == k) beta = nb;
                    }
                    maxb = fmax(maxb, fabs(nb));
                  }
                  // the multiplier step, y = rho u; then D_S(y, mu): A^T y and mu per column, one forward substitution
                  const double v = tt + u;
                  sv = l0_con_clip(v, rlo, rhi);
                  u = v - sv;
                  const double y = lane < rows ? rho * u : 0.0;
                  double aty = 0.0;
                  for (int i = 0; i < rows; ++i) aty = fma(lane < m ? As[mycol * L0_CON_LD + i] : 0.0, l0_bcast(y, i), aty);
                  const double mu = lane < m ? l0_con_box_mu(beta, gr + aty, blo, bhi) : 0.0;
                  double b = lane < m ? cs[mycol] - aty - mu : 0.0, zz = 0.0;
#pragma unroll
                  for (int k = 0; k < L0_PMAX; ++k) {
                    if (k < m) {
                      const double zk = l0_bcast(b * invd, k);
                      zz = fma(zk, zk, zz);
                      b = fma(-Lrow[k], zk, b);
                    }
                  }
                  const double st = (lane < rows ? l0_con_sigma(y, rlo, rhi) : 0.0) + (lane < m ? l0_con_sigma(mu, blo, bhi) : 0.0);
                  const double sa = (lane < rows ? fabs(l0_con_sigma(y, rlo, rhi)) : 0.0) + (lane < m ? fabs(l0_con_sigma(mu, blo, bhi)) : 0.0);
                  const L0ConDual dual = l0_con_dual(zz, l0_wave_sum(st), l0_wave_sum(sa));
                  const double primal = 0.5 * l0_wave_sum(lane < m ? beta * (gr - cs[mycol]) : 0.0);
                  const double viol = l0_wave_max(lane < rows ? l0_con_violation(tt, rlo, rhi, maxb) : 0.0);
                  bound = dual.bound + alpha * (double)cnt;
                  // rejected: it cannot beat the incumbent, or the wave's best under the tie rule
                  if (bound > inc_k || bound > best_k || (bound == best_k && !l0m_less(incl, mask_k))) {
                    rejected = true;
                    break;
                  }
                  if (l0_con_valued(primal, dual, viol, half_ss)) {
                    settled = true;
                    val = primal + alpha * (double)cnt;
                    break;
                  }
                }
                if (!settled && !rejected) {  // the sweep cap ran out: a lower bound on this one support
                  ++unsettled_local;
                  if (lane == 0) atomicMin(&a.ctl[L0_UNSETTLED], l0_key(bound));
                }
              }
            } else if (l0_wave_max(lane < m ? fabs(beta) : 0.0) > big_M) {
              // the box binds: cyclic coordinate descent with clipping on the support's block of H; lane r keeps
              // beta_r and the gradient entry (H beta - c)_r
              beta = fmin(fmax(beta, -big_M), big_M);
              double gr = lane < m ? -cs[mycol] : 0.0;
              for (int k = 0; k < m; ++k) {
                const int ck = __builtin_amdgcn_readlane(mycol, k);
                gr = fma(lane < m ? Hat(ck, mycol) : 0.0, l0_bcast(beta, k), gr);
              }
              for (int sweep = 0; sweep < L0_CD_SWEEPS; ++sweep) {
                double maxd = 0.0, maxb = 0.0;
                for (int k = 0; k < m; ++k) {
                  const int ck = __builtin_amdgcn_readlane(mycol, k);
                  const double bk = l0_bcast(beta, k), gk = l0_bcast(gr, k);
                  const double nb = fmin(fmax(bk - gk / Hat(ck, ck), -big_M), big_M);
                  const double dk = nb - bk;
                  if (dk != 0.0) {
                    gr = fma(lane < m ? Hat(ck, mycol) : 0.0, dk, gr);
                    if (lane == k) beta = nb;
                  }
                  maxd = fmax(maxd, fabs(dk));
                  maxb = fmax(maxb, fabs(nb));
                }
                if (maxd <= L0_CD_TOL * maxb || maxd == 0.0) break;
              }
              if constexpr (PROFILE)
                val = 0.5 * l0_wave_sum(lane < m ? beta * (gr - cs[mycol]) : 0.0);
              else
                val = 0.5 * l0_wave_sum(lane < m ? beta * (gr - cs[mycol]) : 0.0) + alpha * (double)cnt;
            }
            if (settled && val <= inc_k && (val < best_k || (val == best_k && l0m_less(incl, mask_k)))) {
              unsigned long long old = 0;
              if (lane == 0) old = atomicMin(PROFILE ? &a.ctl[L0_PROFILE_INC + cnt - 1] : &a.ctl[L0_INCUMBENT], l0_key(val));
              const double seen = l0_unkey(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(old >> 32)) << 32) |
                                           (unsigned)__builtin_amdgcn_readfirstlane((int)old));
              if constexpr (PROFILE) {
                const double now = fmin(seen, val);
                if (lane == cnt - 1) {
                  inc = now;
                  if (val <= now) {
                    best_v = val;
                    best_mask = incl;
                  }
                }
              } else {
                inc = fmin(seen, val);
                if (val <= inc) {
                  best_v = val;
                  best_mask = incl;
                }
              }
            }
          }
          // a fresh look at the incumbent now and then
          if (++since_refresh >= 32) {
            since_refresh = 0;
            inc = fmin(inc, read_incumbent());
            if constexpr (PROFILE) envelope();
          }
          continue;  // (down, one level deeper)
        }
        if (forced && want) break;  // the ticket's own include is impossible: its subtree is empty
        try_exclude = true;
      } else {
        g = depth - 1;
        if (g < d) break;  // back at the prefix: the ticket is done
        if (l0m_test(incl, g)) {  // back from the include branch: undo it, take the exclude branch
          l0m_clear(incl, g);
          --cnt;
          try_exclude = true;
        } else {
          depth = g;  // back from the exclude branch: climb on
          continue;
        }
      }
      if (try_exclude) {
        m = saved_m(g);
        if constexpr (WIDE) {
          if (g < 64) {
            ss = l0_bcast(st_ss, g);
            needm = l0_bcast(st_need, g);
            if constexpr (L1) na = __builtin_amdgcn_readlane(st_na, g);
          } else {
            ss = l0_bcast(st_ss1, g - 64);
            needm = l0_bcast(st_need1, g - 64);
            if constexpr (L1) na = __builtin_amdgcn_readlane(st_na1, g - 64);
          }
        } else {
          ss = l0_bcast(st_ss, g);
          if constexpr (L1) na = __builtin_amdgcn_readlane(st_na, g);
          needm = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(st_need >> 32), g) << 32) |
                  (unsigned)__builtin_amdgcn_readlane((int)st_need, g);
        }
        if (l0m_test(needm, g)) {  // an included group needs this one
          if (g < d) break;
          depth = g;
          down = false;
        } else {
          if constexpr (XB) {
            // the group joins E: the exclusion factor as it was before the group was decided, then its columns appended
            // (a dependent column and every column beyond L0_XCAP rows are left out: a sub-collection of E bounds too)
            if constexpr (WIDE) {
              if (g < 64) {
                mx = __builtin_amdgcn_readlane(st_mx, g);
                ssx = l0_bcast(st_ssx, g);
              } else {
                mx = __builtin_amdgcn_readlane(st_mx1, g - 64);
                ssx = l0_bcast(st_ssx1, g - 64);
              }
            } else {
              mx = __builtin_amdgcn_readlane(st_mx, g);
              ssx = l0_bcast(st_ssx, g);
            }
            const int x0 = __builtin_amdgcn_readfirstlane(gs[g]), x1 = __builtin_amdgcn_readfirstlane(gs[g + 1]);
            for (int j = x0; j < x1 && mx < L0_XCAP; ++j) {
              const double pjj = Pat(j, j);
              double b = lane < mx ? Pat(j, xcol) : 0.0;
              double s2 = 0.0, sw = 0.0;
              L0_APPEND(L0_XCAP, Xrow, xinvd, xw, mx, b, s2, sw)
              const double piv = pjj - s2;
              if (piv > L0_PIVOT * pjj) {
                const double lmm = sqrt(piv), wm = (bhs[j] - sw) / lmm;
                if (lane == mx) {
                  xinvd = 1.0 / lmm;
                  xw = wm;
                  xcol = j;
                }
                ssx = fma(wm, wm, ssx);
                ++mx;
              }
            }
          }
          depth = g + 1;
          down = true;
        }
      }
    }
  }
  if constexpr (PROFILE) {  // every lane its size: 64 values and 64 supports per wave
    int wv = blockIdx.x * L0_WAVES + (tid >> 6);
    if constexpr (BATCH) wv = (int)(blockIdx.x % (unsigned)a.batch_blocks) * L0_WAVES + (tid >> 6);  // (its number within the problem)
    a.best_val[(size_t)wv * 64 + lane] = best_v;
    if constexpr (WIDE) {
      a.best_mask[((size_t)wv * 64 + lane) * 2] = best_mask.lo;
      a.best_mask[((size_t)wv * 64 + lane) * 2 + 1] = best_mask.hi;
    } else {
      a.best_mask[(size_t)wv * 64 + lane] = best_mask;
    }
  }
  if (lane == 0) {
    if (nodes_local > 0) atomicAdd(&a.ctl[L0_NODES], (unsigned long long)nodes_local);
    if constexpr (L1 || CON)
      if (descents_local > 0) atomicAdd(&a.ctl[L0_DESCENTS], (unsigned long long)descents_local);
    if constexpr (CON)
      if (unsettled_local > 0) atomicAdd(&a.ctl[L0_UNSETTLED_COUNT], (unsigned long long)unsettled_local);
    if constexpr (!PROFILE) {
      const int wv = blockIdx.x * L0_WAVES + (tid >> 6);
      a.best_val[wv] = best_v;
      if constexpr (WIDE) {
        a.best_mask[(size_t)wv * 2] = best_mask.lo;
        a.best_mask[(size_t)wv * 2 + 1] = best_mask.hi;
      } else {
        a.best_mask[wv] = best_mask;
      }
    }
    if constexpr (WIDE)
      if (cap_min != 0x7fffffff) atomicMin(&a.ctl[L0_CAPACITY], (unsigned long long)cap_min + 1ull);
  }
}

#undef L0_APPEND
#undef L0_HL1

}  // namespace slm
