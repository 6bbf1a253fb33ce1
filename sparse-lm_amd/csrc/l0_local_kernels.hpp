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

#include "l0_host.hpp"     // L0_LS_*, l0_ls_coord, l0_ls_threshold, l0_ls_swap_better: shared with the host twin
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

// CARD: the cardinality rule (below, at the loop); else the penalised rule of the unit's head.
template <bool CARD>
static __global__ __launch_bounds__(64 * L0_WAVES) void l0_local_kernel(L0LsArgs a) {
  const int lane = threadIdx.x & 63;
  const int p = a.p, ns = (p + 63) >> 6;
  const long long ld = a.ld;
  const double big_M = a.big_M;
  const int stride = (int)gridDim.x * L0_WAVES;
  for (int q = (int)blockIdx.x * L0_WAVES + (int)(threadIdx.x >> 6); q < a.n_problems; q += stride) {
    const int rc = q / a.n_starts;                                  // r * n_cells + e
    const int rs = __builtin_amdgcn_readfirstlane(rc / a.n_cells);  // the row set: one per wave, so a scalar
    const int cell = rc - rs * a.n_cells;
    const double* __restrict__ G = a.G[rs];
    const double* __restrict__ cv = a.c[rs];
    const double tol = L0_CD_TOL * sqrt(a.yy[rs]);
    const double alpha = CARD ? 0.0 : a.alphas[cell], eta2 = 2.0 * a.etas[cell];
    double beta[L0_LS_SLOTS], r[L0_LS_SLOTS], d[L0_LS_SLOTS];
    double dmax = 0.0;
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s) {
      const int j = s * 64 + lane;
      beta[s] = 0.0;
      r[s] = 0.0;
      d[s] = 0.0;
      if (s < ns && j < p) {
        d[s] = G[(long long)j * ld + j] + eta2;
        r[s] = cv[j];
        if (a.starts) beta[s] = a.starts[(long long)q * p + j];
      }
      dmax = fmax(dmax, d[s]);
    }
    dmax = l0_wave_max(dmax);
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s)
      if (!(d[s] > L0_PIVOT * dmax)) {  // d = 0 marks a column that stays out (and the lanes beyond p)
        d[s] = 0.0;
        beta[s] = 0.0;
      }
    // r = c - H beta of the start, column by column in ascending order
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s)
      if (s < ns) {
        unsigned long long act = __ballot(beta[s] != 0.0);
        while (act) {
          const int k = __builtin_ctzll(act);
          act &= act - 1;
          l0_ls_axpy(r, G, ld, p, ns, lane, eta2, s * 64 + k, -l0_bcast(beta[s], k));
        }
      }

    int sweeps = 0, swaps = 0, status = 0;
    int kmax = 0, nact = 0, grows = 0, drops = 0;  // (the cardinality rule's: the cell's size, the support's, the two counts)
    if constexpr (CARD) {
      kmax = a.sizes[cell];
#pragma unroll
      for (int s = 0; s < L0_LS_SLOTS; ++s)
        if (s < ns) nact += __popcll(__ballot(beta[s] != 0.0));
      // ---- shrink: while the support is larger than k its weakest column leaves (only a start can be: nothing below adds beyond k)
      while (nact > kmax) {
        double gb = HUGE_VAL;
        int ib = 0x7fffffff;
#pragma unroll
        for (int t = 0; t < L0_LS_SLOTS; ++t)
          if (t < ns) {
            const double g = l0_ls_coord(r[t] + d[t] * beta[t], d[t], big_M).gain;
            if (beta[t] != 0.0 && g < gb) {  // (ascending slots: the lane keeps its lowest i on ties)
              gb = g;
              ib = t * 64 + lane;
            }
          }
        const double gmin = -l0_wave_max(-gb);
        const int imin = l0_ls_wave_min(gb == gmin ? ib : 0x7fffffff);
        if (imin == 0x7fffffff) break;
        double mine = 0.0;
#pragma unroll
        for (int t = 0; t < L0_LS_SLOTS; ++t)
          if (t == (imin >> 6)) {
            mine = beta[t];
            if (lane == (imin & 63)) beta[t] = 0.0;
          }
        l0_ls_axpy(r, G, ld, p, ns, lane, eta2, imin, l0_bcast(mine, imin & 63));
        --nact;
        ++drops;
      }
    }
    for (;;) {
      // ---- 1. the descent to its fixed point (the cardinality rule: on the support alone, no threshold, b == 0 leaves) ---------
      for (int sw = 0;; ++sw) {
        if (sw == L0_CD_SWEEPS) {
          status |= L0_LS_SWEEPS_OUT;
          break;
        }
        bool moved = false;
        double maxd = 0.0;
        int cursor = 0;
        for (;;) {  // the next change at or after the cursor
          const int s0 = cursor >> 6;
          bool found = false;
          int jf = 0;
          double delta = 0.0;
#pragma unroll
          for (int s = 0; s < L0_LS_SLOTS; ++s)
            if (!found && s >= s0 && s < ns) {
              const L0LsCoord cd = l0_ls_coord(r[s] + d[s] * beta[s], d[s], big_M);
              const double nb = CARD ? cd.b : l0_ls_threshold(cd, alpha);
              const unsigned long long bal = __ballot((CARD ? beta[s] != 0.0 : d[s] > 0.0) && s * 64 + lane >= cursor && nb != beta[s]);
              if (bal) {
                const int k = __builtin_ctzll(bal);
                const double nbk = l0_bcast(nb, k), old = l0_bcast(beta[s], k), dk = l0_bcast(d[s], k);
                if (lane == k) beta[s] = nbk;
                found = true;
                jf = s * 64 + k;
                delta = nbk - old;
                moved = moved || ((nbk != 0.0) != (old != 0.0));
                if constexpr (CARD)
                  if (nbk == 0.0) {
                    --nact;
                    ++drops;
                  }
                maxd = fmax(maxd, fabs(delta) * sqrt(dk));
              }
            }
          if (!found) break;
          l0_ls_axpy(r, G, ld, p, ns, lane, eta2, jf, -delta);
          cursor = jf + 1;
        }
        ++sweeps;
        if (!moved && maxd <= tol) break;
      }
      if constexpr (CARD) {
        // ---- grow: below k, the outside column with the largest gain enters -- if it would move by more than the descent's own
        // stopping tolerance -- and the descent runs again.  The swap scan's arg-max without a removed column and without a row read.
        if (status) break;
        if (nact < kmax) {
          double gb = -1.0, bb = 0.0;
          int jb = 0x7fffffff;
#pragma unroll
          for (int t = 0; t < L0_LS_SLOTS; ++t)
            if (t < ns) {
              const L0LsCoord co = l0_ls_coord(r[t], d[t], big_M);
              if (d[t] > 0.0 && beta[t] == 0.0 && co.gain > gb) {  // (ascending slots: the lane keeps its lowest j on ties)
                gb = co.gain;
                bb = fabs(co.b) * sqrt(d[t]) > tol ? co.b : 0.0;  // (0: it would not move)
                jb = t * 64 + lane;
              }
            }
          const double gmax = l0_wave_max(gb);
          const int jmin = l0_ls_wave_min(gb == gmax ? jb : 0x7fffffff);
          const double bj = jmin != 0x7fffffff ? l0_bcast(bb, jmin & 63) : 0.0;  // (that lane's best IS jmin)
          if (bj != 0.0) {
#pragma unroll
            for (int t = 0; t < L0_LS_SLOTS; ++t)
              if (t == (jmin >> 6) && lane == (jmin & 63)) beta[t] = bj;
            l0_ls_axpy(r, G, ld, p, ns, lane, eta2, jmin, -bj);
            ++nact;
            ++grows;
            continue;
          }
        }
      }
      if (!a.swaps || status) break;
      // ---- 2. the swap scan: the first i of the support that a column outside replaces with a gain ----------------------------
      bool swapped = false;
#pragma unroll
      for (int si = 0; si < L0_LS_SLOTS; ++si)
        if (!swapped && si < ns) {
          unsigned long long act = __ballot(beta[si] != 0.0);
          while (act && !swapped) {
            const int k = __builtin_ctzll(act);
            act &= act - 1;
            const int i = si * 64 + k;
            const double bi = l0_bcast(beta[si], k), di = l0_bcast(d[si], k), ri = l0_bcast(r[si], k);
            const double gi = l0_ls_coord(ri + di * bi, di, big_M).gain;
            const double* row = G + (long long)i * ld;
            double gb = -1.0, bb = 0.0;
            int jb = 0x7fffffff;
#pragma unroll
            for (int t = 0; t < L0_LS_SLOTS; ++t)
              if (t < ns) {
                const int j = t * 64 + lane;
                const double h = j < p ? row[j] : 0.0;
                const L0LsCoord co = l0_ls_coord(r[t] + h * bi, d[t], big_M);
                if (d[t] > 0.0 && beta[t] == 0.0 && co.gain > gb) {  // (ascending slots: the lane keeps its lowest j on ties)
                  gb = co.gain;
                  bb = co.b;
                  jb = j;
                }
              }
            const double gmax = l0_wave_max(gb);
            const int jmin = l0_ls_wave_min(gb == gmax ? jb : 0x7fffffff);
            if (jmin != 0x7fffffff && l0_ls_swap_better(gmax, gi, alpha)) {
              const double bj = l0_bcast(bb, jmin & 63);  // (that lane's best IS jmin)
              if (lane == k) beta[si] = 0.0;
              l0_ls_axpy(r, G, ld, p, ns, lane, eta2, i, bi);
#pragma unroll
              for (int t = 0; t < L0_LS_SLOTS; ++t)
                if (t == (jmin >> 6) && lane == (jmin & 63)) beta[t] = bj;
              l0_ls_axpy(r, G, ld, p, ns, lane, eta2, jmin, -bj);
              ++swaps;
              swapped = true;
            }
          }
        }
      if (!swapped) break;
      if (swaps == L0_LS_SWAPS) {
        status |= L0_LS_SWAPS_OUT;
        break;
      }
    }

    // F = 1/2 beta^T H beta - c^T beta + alpha nnz with H beta = c - r; the problem's own row of every output
    double acc = 0.0;
    int nnz = 0;
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s)
      if (s < ns) {
        const int j = s * 64 + lane;
        if (j < p) {
          acc += beta[s] * (cv[j] + r[s]);
          nnz += beta[s] != 0.0;
          a.beta_out[(long long)q * p + j] = beta[s];
        }
      }
    acc = l0_wave_sum(acc);
    nnz = (int)l0_wave_sum((double)nnz);
    if (lane == 0) {
      a.F_out[q] = -0.5 * acc + alpha * (double)nnz;
      int* stat = a.stat_out + (long long)q * a.stat_stride;
      stat[0] = sweeps;
      stat[1] = swaps;
      stat[2] = status;
      stat[3] = nnz;
      if constexpr (CARD) {
        stat[4] = grows;
        stat[5] = drops;
      }
    }
  }
}

}  // namespace slm
