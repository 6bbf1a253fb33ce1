// The NODE RELAXATION on chip (slm_solve_l0_local_nodes and, round after round, slm_solve_l0_local_prove, engine_l0.hip; the
// mathematics, the shared arithmetic, the host twin l0_node_solve and the tree l0_prove_tree: l0_host.hpp, "local proof";
// DESIGN 4d "Local proof").  The local bound (l0_local_bound_kernels.hpp) bounds the root of a cell.  A branch-and-bound tree
// fixes some columns IN (they pay alpha whether their coefficient is zero or not) and some OUT (beta_j = 0), and the bound's
// relaxation on such a node is the same separable convex problem with three kinds of coordinate: for EVERY vector u, with
// t = c - G u,
//     L_node(u) = -1/2 u^T G u - sum over FREE of max(0, h(t_j) - alpha) - sum over IN of (h(t_j) - alpha)   <=   min F on the node.
// This kernel is l0_local_bound_kernel with that third of a difference -- the older kernel stays as it is -- and with what a
// tree needs beside the bound: every node names its CELL (an index into the alphas, etas, lams and taus of the call, so that
// the trees of every cell of a grid advance in one launch), brings its parent's bound (lower = max(L_node(u), L_node(0),
// parent_lower): the child's feasible set lies inside the parent's) and its parent's u as its start, and gets back
// F(u) = 1/2 u^T (G + 2 eta I) u - c^T u + alpha nnz(u), an upper bound of the cell because u lies in the box.
//
// One WAVEFRONT per NODE, a grid-stride loop over the nodes, the bound kernel's layout: coordinate j lives in lane j & 63, slot
// j >> 6; u, t and G_jj take 16 doubles each per lane, every loop over the slots is unrolled and every index a compile-time
// constant; no LDS, no barrier, no atomic.  A node's masks are 16 + 16 words of 64 bits, bit `lane` of word `slot`; a lane
// packs the two bits of its 16 slots into ONE 32-bit register at the start of its node.  An OUT column is handled like one
// that fails the pivot test: its G_jj is set to zero, which keeps u_j = 0.  Where a tree's round holds hundreds of nodes, this
// latency-bound kernel fills the chip from a handful of cells.
//
// Kernel and twin give the same bits, by the bound kernel's discipline: contraction off wherever the compiler would decide it,
// the sums in one fixed order (per lane over its slots, then the butterfly), lam and tauc from the host, and the one contracted
// step, t += w G[:, j] in l0_ls_axpy, std::fma in the twin.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "l0_host.hpp"           // L0_LS_*, L0_ND_*, l0_node_coord, l0_node_phi, l0_node_conj, l0_node_combine, l0_lb_changed, l0_lb_closed
#include "l0_kernels.hpp"        // L0_WAVES, l0_bcast, l0_wave_max, l0_wave_sum
#include "l0_local_kernels.hpp"  // l0_ls_axpy

namespace slm {

struct L0NdArgs {
  const double* G;       // [p][ld]: the filed Gram, in place
  const double* c;       // [p]
  const double* alphas;  // [n_cells]
  const double* etas;    // [n_cells]
  const double* lams;    // [n_cells]: l0_lb_cell's lam
  const double* taus;    // [n_cells]: l0_lb_cell's tauc
  const int* cell;       // [n_nodes]: the node's cell
  const unsigned long long* in_mask;   // [n_nodes][16]
  const unsigned long long* out_mask;  // [n_nodes][16]
  const double* parent_lower;          // [n_nodes], or NULL: none
  const double* starts;  // [n_nodes][p], or NULL: zero
  double* lower_out;     // [n_nodes]: max(L_node(u), L_node(0), parent_lower)
  double* primal_out;    // [n_nodes]: P_node(u)
  double* upper_out;     // [n_nodes]: F(u)
  double* u_out;         // [n_nodes][p]
  int* stat_out;         // [n_nodes][2]: sweeps, status word
  long long ld;
  int p, n_nodes, max_sweeps;
  double big_M, gap_tol;
};

// P_node(u), L_node(u) and F(u) from the registers (the host's l0_node_values, in its order); st: the lane's packed states
static __device__ __forceinline__ L0NodeValues l0_nd_wave_values(const double (&u)[L0_LS_SLOTS], const double (&t)[L0_LS_SLOTS],
                                                                 const double* __restrict__ cv, int p, int ns, int lane, unsigned st,
                                                                 double alpha, double eta, double lam, double tauc, double big_M) {
#pragma clang fp contract(off)
  double qp = 0.0, ql = 0.0, sp = 0.0, sc = 0.0, s2 = 0.0, nz = 0.0;
#pragma unroll
  for (int s = 0; s < L0_LS_SLOTS; ++s)
    if (s < ns) {
      const int j = s * 64 + lane;
      if (j < p) {
        const int state = (int)((st >> (2 * s)) & 3u);
        const double cj = cv[j];
        qp += u[s] * (cj + t[s]);
        ql += u[s] * (cj - t[s]);
        sp += l0_node_phi(u[s], alpha, eta, lam, tauc, state);
        sc += l0_node_conj(t[s], alpha, eta, big_M, state);
        s2 += u[s] * u[s];
        nz += u[s] != 0.0 ? 1.0 : 0.0;
      }
    }
  qp = l0_wave_sum(qp);
  ql = l0_wave_sum(ql);
  sp = l0_wave_sum(sp);
  sc = l0_wave_sum(sc);
  s2 = l0_wave_sum(s2);
  nz = l0_wave_sum(nz);
  return l0_node_combine(qp, ql, sp, sc, s2, nz, alpha, eta);
}

// t = c - G u, column by column in ascending order
static __device__ __forceinline__ void l0_nd_build(double (&t)[L0_LS_SLOTS], const double (&u)[L0_LS_SLOTS], const double* __restrict__ G,
                                                   const double* __restrict__ cv, long long ld, int p, int ns, int lane) {
#pragma unroll
  for (int s = 0; s < L0_LS_SLOTS; ++s) {
    const int j = s * 64 + lane;
    t[s] = s < ns && j < p ? cv[j] : 0.0;
  }
#pragma unroll
  for (int s = 0; s < L0_LS_SLOTS; ++s)
    if (s < ns) {
      unsigned long long act = __ballot(u[s] != 0.0);
      while (act) {
        const int k = __builtin_ctzll(act);
        act &= act - 1;
        l0_ls_axpy(t, G, ld, p, ns, lane, 0.0, s * 64 + k, -l0_bcast(u[s], k));
      }
    }
}

static __global__ __launch_bounds__(64 * L0_WAVES) void l0_local_node_kernel(L0NdArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int p = a.p, ns = (p + 63) >> 6;
  const long long ld = a.ld;
  const double big_M = a.big_M;
  const double* __restrict__ G = a.G;
  const double* __restrict__ cv = a.c;
  const int stride = (int)gridDim.x * L0_WAVES;
  for (int e0 = (int)blockIdx.x * L0_WAVES + (int)(threadIdx.x >> 6); e0 < a.n_nodes; e0 += stride) {
    const int e = __builtin_amdgcn_readfirstlane(e0);  // the node: one per wave, so a scalar
    const int ce = a.cell[e];
    const double alpha = a.alphas[ce], eta = a.etas[ce], lam = a.lams[ce], tauc = a.taus[ce];
    unsigned st = 0;  // the lane's 16 states, two bits a slot: bit 2 s the IN bit, bit 2 s + 1 the OUT bit
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s)
      if (s < ns) {
        const unsigned long long wi = a.in_mask[(long long)e * L0_ND_WORDS + s], wo = a.out_mask[(long long)e * L0_ND_WORDS + s];
        st |= ((unsigned)((wi >> lane) & 1ull) | ((unsigned)((wo >> lane) & 1ull) << 1)) << (2 * s);
      }
    double u[L0_LS_SLOTS], t[L0_LS_SLOTS], d[L0_LS_SLOTS];
    double dmax = 0.0;
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s) {
      const int j = s * 64 + lane;
      u[s] = 0.0;
      t[s] = 0.0;
      d[s] = 0.0;
      if (s < ns && j < p) {
        d[s] = G[(long long)j * ld + j];
        t[s] = cv[j];
      }
      dmax = fmax(dmax, d[s]);
    }
    dmax = l0_wave_max(dmax);
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s)  // d = 0 marks a column that keeps u_j = 0: a failed pivot, an OUT column, a lane beyond p
      if (!(d[s] > L0_PIVOT * dmax) || ((st >> (2 * s)) & 3u) == (unsigned)L0_ND_OUT) d[s] = 0.0;
    const double L0 = l0_nd_wave_values(u, t, cv, p, ns, lane, st, alpha, eta, lam, tauc, big_M).L;  // L_node(0): u = 0, t = c
    if (a.starts) {
#pragma unroll
      for (int s = 0; s < L0_LS_SLOTS; ++s) {
        const int j = s * 64 + lane;
        if (s < ns && j < p && d[s] > 0.0) {
          const double v = a.starts[(long long)e * p + j];
          u[s] = v < -big_M ? -big_M : (v > big_M ? big_M : v);  // clipped into the box
        }
      }
      l0_nd_build(t, u, G, cv, ld, p, ns, lane);
    }

    int sweeps = 0, status = 0;
    for (int sw = 0;; ++sw) {
      if (sw == a.max_sweeps) {
        status |= L0_LS_SWEEPS_OUT;
        break;
      }
      int cursor = 0;
      for (;;) {  // the next change at or after the cursor
        const int s0 = cursor >> 6;
        bool found = false;
        int jf = 0;
        double delta = 0.0;
#pragma unroll
        for (int s = 0; s < L0_LS_SLOTS; ++s)
          if (!found && s >= s0 && s < ns) {
            const double nb = l0_node_coord(t[s] + d[s] * u[s], d[s], eta, lam, tauc, big_M, (int)((st >> (2 * s)) & 3u));
            const unsigned long long bal = __ballot(d[s] > 0.0 && s * 64 + lane >= cursor && l0_lb_changed(nb, u[s]));
            if (bal) {
              const int k = __builtin_ctzll(bal);
              const double nbk = l0_bcast(nb, k), old = l0_bcast(u[s], k);
              if (lane == k) u[s] = nbk;
              found = true;
              jf = s * 64 + k;
              delta = nbk - old;
            }
          }
        if (!found) break;
        l0_ls_axpy(t, G, ld, p, ns, lane, 0.0, jf, -delta);
        cursor = jf + 1;
      }
      ++sweeps;
      const L0NodeValues v = l0_nd_wave_values(u, t, cv, p, ns, lane, st, alpha, eta, lam, tauc, big_M);
      if (l0_lb_closed(v.P, v.L, alpha, a.gap_tol)) break;
    }

    // the certificate: t rebuilt from u alone, L, P and F on it; the node's own row of every output
    l0_nd_build(t, u, G, cv, ld, p, ns, lane);
    const L0NodeValues v = l0_nd_wave_values(u, t, cv, p, ns, lane, st, alpha, eta, lam, tauc, big_M);
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s)
      if (s < ns) {
        const int j = s * 64 + lane;
        if (j < p) a.u_out[(long long)e * p + j] = u[s];
      }
    if (lane == 0) {
      double low = v.L > L0 ? v.L : L0;
      if (a.parent_lower) {
        const double pl = a.parent_lower[e];
        low = low > pl ? low : pl;
      }
      a.lower_out[e] = low;
      a.primal_out[e] = v.P;
      a.upper_out[e] = v.F;
      a.stat_out[2 * e] = sweeps;
      a.stat_out[2 * e + 1] = status;
    }
  }
}

}  // namespace slm
