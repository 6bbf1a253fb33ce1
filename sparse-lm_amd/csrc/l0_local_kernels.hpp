// The l0 LOCAL SEARCH on chip (slm_solve_l0_local, engine_l0.hip; the rule and its host twin l0_ls_solve: l0_host.hpp, "local
// search"; DESIGN 4d "Local search").  Where the exact search (l0_kernels.hpp) stops at 128 columns, this kernel takes
// L0_LS_PMAX = 1024 and proves nothing: cyclic coordinate descent with hard thresholding on
//     F(beta) = 1/2 beta^T H beta - c^T beta + alpha ||beta||_0,   H = G + 2 eta I,   |beta_j| <= big_M,
// then one-for-one swaps until none helps.
//
// One WAVEFRONT per (cell, start) problem; the L0_WAVES wavefronts of a workgroup share nothing, there is no LDS and no barrier,
// and a grid-stride loop over the problems lets a launch hold more problems than the grid has waves.  Coordinate j lives in
// lane j & 63, slot j >> 6: beta, r = c - H beta and d = diag H take 16 doubles each per lane.  Every loop over the slots is
// unrolled and every index into them a compile-time constant; the one entry a step updates is selected by comparing the lane
// (and, for a swap's incoming column, the slot) -- nothing is indexed at run time, so nothing goes to scratch.
//
// The sequential rule does not cost p steps per sweep.  Until a coordinate changes, r is unchanged, so all lanes evaluate their
// coordinates at once; because j = 64 slot + lane, the first j >= the cursor whose value would change is in the first slot with
// a changing lane, and there it is the lowest such lane: one ballot per slot, no arg-min.  That change is applied -- ONE read of
// row j of G (symmetric: column j), 64 consecutive doubles per slot, all slots' loads in flight together -- and the cursor moves
// to j + 1.  This is exactly the sequence of changes of the sequential rule.  The swap scan does the same per i of the support:
// one read of row i, every lane's best gain over its outside columns, a wave arg-max with the lowest index on ties.
//
// G and c are read IN PLACE from the dataset's Gram store with its leading dimension; 2 eta goes on the diagonal here.  Each
// problem owns row q of every output, so nothing is shared and there is no atomic.  Every applied change is one dependent read
// of 8 p bytes (from L2 / Infinity Cache: the Gram is at most 8 MB), so a problem is latency-bound and the chip fills only
// through the number of problems.
//
// ROW SETS (slm_solve_l0_local_folds: the training rows of a cross-validation's folds, then all rows).  Problem
// q = (r * n_cells + e) * n_starts + s is row set r, cell e, start s: it reads G_r, c_r and yy_r (which feeds tol); alphas and
// etas stay per cell and are shared by the row sets.  Up to L0_LS_ROW_SETS = 16 pointers and scalars ride in the kernel
// argument; r is made a scalar (readfirstlane: a wave is one problem), so the choice is three scalar loads per problem and
// nothing per lane.  With one row set r = 0 and e = q / n_starts: the parent's problem, change by change.
//
// THE CARDINALITY RULE (l0_local_kernel<true>; slm_solve_l0_local_subsets; the host twin l0_lc_solve, l0_host.hpp "local
// subsets").  Cell e is (sizes[e], etas[e]):  minimise Q = 1/2 beta^T H beta - c^T beta over the box with ||beta||_0 <= k.  The same
// wave, state, Gram reads and outputs; three moves more, each a scan of the registers with no row read of its own: SHRINK (a
// start larger than k loses its column of the smallest one-coordinate gain, an arg-min over the support, until k are left),
// the descent restricted to beta != 0 with no threshold (a coordinate whose b is exactly 0 leaves), and GROW (below k, the
// arg-max of the gains over the columns outside enters when it would move by more than the descent's stopping tolerance; the
// descent runs again).  The swap scan follows once nothing grows, with alpha = 0.  stat_out gets two words more per problem:
// grows and drops.  The penalised instantiation l0_local_kernel<false> is the code it was.
//
// THE L1 RULE (l0_local_l1_kernel; slm_solve_l0_local_l1; the host twin l0_local_solve<false, true>, l0_host.hpp "local search
// with an l1 term").  Cell e is (alphas[e], l1s[e], etas[e]) and F gains lam ||beta||_1.  The penalised rule, word for word, with
// the coordinate l0_ls_coord_l1 (a soft threshold before the clip, lam |b| off the gain) in the descent and in both gains of the
// swap scan: lam is one scalar per problem, read next to alpha.  The three kernels are ONE body, l0_local_body.inc; what a rule
// does not use is compiled out (if constexpr), so the two older kernels are the code they were.
//
// l0_eliminate_kernel is the intercept of those row sets: the dataset is [X | 1] with the ones column last, and for each row
// set the Schur complement of that column,  G' = G - g1 g1^T / G11  (g1 = G[:, last], G11 = G[last][last]), is written into a
// workspace of the call with the dataset's leading dimension -- exactly weighted centring of X by the row set's own means --
// and the search reads G' as it reads a filed Gram.  The filed Grams are not modified.  (The vectors c', xmean and the
// scalars yy', ymean are the host's: l0_eliminate_vectors, l0_host.hpp.)  Cancellation, as for l0_eliminate_last: G_ij holds
// mean_i mean_j + cov_ij and the subtraction removes the first term, so the centred entry keeps a relative error of about
// 2^-53 (1 + mean_i mean_j / cov_ij): a column whose |mean| is 1e4 times its spread loses eight to nine of sixteen digits.
// Data far from the origin should be shifted by the caller.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "l0_host.hpp"     // L0_LS_*, l0_ls_coord, l0_ls_coord_l1, l0_ls_threshold, l0_ls_swap_better: shared with the host twin
#include "l0_kernels.hpp"  // L0_WAVES, l0_bcast, l0_wave_max, l0_wave_sum

namespace slm {

struct L0LsArgs {
  const double* G[L0_LS_ROW_SETS];  // [p][ld] per row set: a filed Gram in place, or the call's eliminated copy
  const double* c[L0_LS_ROW_SETS];  // [p] per row set
  double yy[L0_LS_ROW_SETS];        // per row set
  const double* alphas;  // [n_cells]
  const double* etas;    // [n_cells]
  const double* starts;  // [n_problems][p] inside the box, or NULL: zero
  double* beta_out;      // [n_problems][p]
  double* F_out;         // [n_problems]
  int* stat_out;         // [n_problems][stat_stride]: sweeps, swaps, status word (L0_LS_SWEEPS_OUT | L0_LS_SWAPS_OUT), non-zeros;
                         // the cardinality rule: then grows, drops
  const int* sizes;      // [n_cells]: the cardinality rule's k per cell (l0_local_kernel<true>; alphas is not read there)
  long long ld;
  int p, n_problems, n_starts, swaps;  // swaps == 0: the descent alone
  int n_cells;                         // problem q = (r * n_cells + e) * n_starts + s: row set r, cell e, start s
  int stat_stride;                     // 4, the cardinality rule 6
  double big_M;
};

struct L0ElimArgs {
  const double* G[L0_LS_ROW_SETS];  // [ps + 1][ld] per row set: the filed Gram of [X | 1]
  double* out;                      // row set r: [ps][ld] at out + r * stride
  long long ld, stride;
  int ps;
};

// G'[i][j] = G[i][j] - g1[i] g1[j] / G11 for i, j < ps (the padding j >= ps of a row: 0).  Grid (column blocks, ps rows, row
// sets); g1 is read from the LAST ROW (the store holds both triangles, mirrored from one value), so every read is coalesced.
// (a - (b c) / d: the division stands between the product and the difference, so nothing contracts and the host twin
// l0_eliminate_last_ld gives the same bits.)
static __global__ __launch_bounds__(256) void l0_eliminate_kernel(L0ElimArgs a) {
  const int i = (int)blockIdx.y, ps = a.ps;
  const long long ld = a.ld;
  const double* __restrict__ G = a.G[blockIdx.z];
  const double* __restrict__ last = G + (long long)ps * ld;
  const double g11 = last[ps], gi = last[i];
  const double* __restrict__ row = G + (long long)i * ld;
  double* __restrict__ out = a.out + (long long)blockIdx.z * a.stride + (long long)i * ld;
  for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < ld; j += (long long)gridDim.x * 256)
    out[j] = j < ps ? row[j] - gi * last[j] / g11 : 0.0;
}

static __device__ __forceinline__ int l0_ls_wave_min(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}

// r += w H[:, j] (row j of G, 2 eta on the diagonal): one coalesced read, the slots' loads independent of each other
static __device__ __forceinline__ void l0_ls_axpy(double (&r)[L0_LS_SLOTS], const double* __restrict__ G, long long ld, int p, int ns, int lane,
                                                  double eta2, int j, double w) {
  const double* row = G + (long long)j * ld;
#pragma unroll
  for (int t = 0; t < L0_LS_SLOTS; ++t)
    if (t < ns) {
      const int k = t * 64 + lane;
      if (k < p) {
        double h = row[k];
        if (k == j) h += eta2;
        r[t] += w * h;
      }
    }
}

// The l1 rule's argument: the penalised rule's, and the cells' l1 weights.  (Its own struct, so that the two older kernels keep
// their argument and their code.)
struct L0LsL1Args : L0LsArgs {
  const double* l1s;  // [n_cells]
};

// the coordinate of the penalised path: with an l1 term l0_ls_coord_l1, else l0_ls_coord (lam is not read)
template <bool L1>
static __device__ __forceinline__ L0LsCoord l0_ls_coord_of(double u, double d, double big_M, double lam) {
  if constexpr (L1)
    return l0_ls_coord_l1(u, d, big_M, lam);
  else
    return l0_ls_coord(u, d, big_M);
}

// The family's kernels: one body (l0_local_body.inc), three kernels.  CARD: the cardinality rule; else the penalised rule of the
// unit's head.
template <bool CARD>
static __global__ __launch_bounds__(64 * L0_WAVES) void l0_local_kernel(L0LsArgs a) {
  constexpr bool L1 = false;
  const double* const l1s = nullptr;
#include "l0_local_body.inc"
}

// The penalised rule with an l1 term (slm_solve_l0_local_l1; the host twin l0_local_solve<false, true>).
static __global__ __launch_bounds__(64 * L0_WAVES) void l0_local_l1_kernel(L0LsL1Args a) {
  constexpr bool CARD = false, L1 = true;
  const double* const l1s = a.l1s;
#include "l0_local_body.inc"
}

}  // namespace slm
