// The LOCAL BOUND on chip (slm_solve_l0_local_bound, engine_l0.hip; the mathematics, the shared arithmetic and the host twin
// l0_bound_solve: l0_host.hpp, "local bound"; DESIGN 4d "Local bound").  The local search (l0_local_kernels.hpp) returns a support
// and proves nothing; this kernel returns, for every cell (alpha, eta) of a grid, a number that is PROVEN to lie at or below
//     min over |beta_j| <= big_M of   F(beta) = 1/2 beta^T (G + 2 eta I) beta - c^T beta + alpha ||beta||_0:
// for every vector u, with t = c - G u,   L(u) = -1/2 u^T G u - sum_j max(0, h(t_j) - alpha)  <=  min F   (h: l0_lb_conj).
// The kernel looks for the u that makes the bound tight -- the minimiser of the convex relaxation P(b) = 1/2 b^T G b - c^T b +
// sum phi(b_j) -- by cyclic coordinate descent (l0_lb_coord, the exact coordinate minimiser), and whatever u it ends at, the
// number it writes is a bound: the certificate is evaluated on t REBUILT from u alone, and L(0) stands in where that is better.
//
// One WAVEFRONT per cell, the layout of the local search: coordinate j lives in lane j & 63, slot j >> 6; u, t and G_jj take 16
// doubles each per lane, every loop over the slots is unrolled and every index a compile-time constant, so nothing goes to
// scratch; there is no LDS, no barrier and no atomic, and a grid-stride loop takes the cells beyond the grid.  A sweep costs
// one row read per coordinate that CHANGES: until one changes, t is unchanged, so all lanes evaluate their coordinates at once
// and the first changing j at or after the cursor is found by one ballot per slot -- exactly the sequential rule's sequence.
// The Gram is read in place through l0_ls_axpy with the ridge argument 0 (the ridge lives in phi).  After every sweep P and L
// come from the running t by four wave sums; the sweeps end when P - L <= gap_tol max(|P|, alpha) or at max_sweeps (status
// word bit L0_LS_SWEEPS_OUT).  A cell whose every active coordinate moves costs p dependent row reads a sweep: like the local
// search it is latency-bound and fills the chip only through the number of cells.
//
// Kernel and twin give the same bits: every expression whose contraction the compiler would decide is compiled with
// contraction off (L0_LB_STRICT in the shared functions, the pragma below), the sums run in one fixed order (per lane over its
// slots, then the butterfly: l0_lb_wave_sum is its restatement), lam and tauc come from the host, and the one contracted step,
// t += w G[:, j] in l0_ls_axpy, is std::fma in the twin.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "l0_host.hpp"           // L0_LS_*, l0_lb_coord, l0_lb_phi, l0_lb_conj, l0_lb_changed, l0_lb_closed: shared with the host twin
#include "l0_kernels.hpp"        // L0_WAVES, l0_bcast, l0_wave_max, l0_wave_sum
#include "l0_local_kernels.hpp"  // l0_ls_axpy

namespace slm {

struct L0LbArgs {
  const double* G;       // [p][ld]: the filed Gram, in place
  const double* c;       // [p]
  const double* alphas;  // [n_cells]
  const double* etas;    // [n_cells]
  const double* lams;    // [n_cells]: l0_lb_cell's lam
  const double* taus;    // [n_cells]: l0_lb_cell's tauc
  const double* starts;  // [n_cells][p], or NULL: zero
  double* lower_out;     // [n_cells]: max(L(u), L(0))
  double* primal_out;    // [n_cells]: P(u)
  double* u_out;         // [n_cells][p]
  int* stat_out;         // [n_cells][2]: sweeps, status word
  long long ld;
  int p, n_cells, max_sweeps;
  double big_M, gap_tol;
};

// P(u) and L(u) from the registers (the host's l0_lb_values, in its order)
static __device__ __forceinline__ L0LbValues l0_lb_wave_values(const double (&u)[L0_LS_SLOTS], const double (&t)[L0_LS_SLOTS],
                                                               const double* __restrict__ cv, int p, int ns, int lane, double alpha,
                                                               double eta, double lam, double tauc, double big_M) {
#pragma clang fp contract(off)
  double qp = 0.0, ql = 0.0, sp = 0.0, sc = 0.0;
#pragma unroll
  for (int s = 0; s < L0_LS_SLOTS; ++s)
    if (s < ns) {
      const int j = s * 64 + lane;
      if (j < p) {
        const double cj = cv[j];
        qp += u[s] * (cj + t[s]);
        ql += u[s] * (cj - t[s]);
        sp += l0_lb_phi(u[s], alpha, eta, lam, tauc);
        sc += l0_lb_conj(t[s], alpha, eta, big_M);
      }
    }
  qp = l0_wave_sum(qp);
  ql = l0_wave_sum(ql);
  sp = l0_wave_sum(sp);
  sc = l0_wave_sum(sc);
  return L0LbValues{-0.5 * qp + sp, -0.5 * ql - sc};
}

// t = c - G u, column by column in ascending order
static __device__ __forceinline__ void l0_lb_build(double (&t)[L0_LS_SLOTS], const double (&u)[L0_LS_SLOTS], const double* __restrict__ G,
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

static __global__ __launch_bounds__(64 * L0_WAVES) void l0_local_bound_kernel(L0LbArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int p = a.p, ns = (p + 63) >> 6;
  const long long ld = a.ld;
  const double big_M = a.big_M;
  const double* __restrict__ G = a.G;
  const double* __restrict__ cv = a.c;
  const int stride = (int)gridDim.x * L0_WAVES;
  for (int e0 = (int)blockIdx.x * L0_WAVES + (int)(threadIdx.x >> 6); e0 < a.n_cells; e0 += stride) {
    const int e = __builtin_amdgcn_readfirstlane(e0);  // the cell: one per wave, so a scalar
    const double alpha = a.alphas[e], eta = a.etas[e], lam = a.lams[e], tauc = a.taus[e];
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
    for (int s = 0; s < L0_LS_SLOTS; ++s)
      if (!(d[s] > L0_PIVOT * dmax)) d[s] = 0.0;  // d = 0 marks a column that keeps u_j = 0 (and the lanes beyond p)
    const double L0 = l0_lb_wave_values(u, t, cv, p, ns, lane, alpha, eta, lam, tauc, big_M).L;  // L(0): u = 0, t = c
    if (a.starts) {
#pragma unroll
      for (int s = 0; s < L0_LS_SLOTS; ++s) {
        const int j = s * 64 + lane;
        if (s < ns && j < p && d[s] > 0.0) {
          const double v = a.starts[(long long)e * p + j];
          u[s] = v < -big_M ? -big_M : (v > big_M ? big_M : v);  // clipped into the box
        }
      }
      l0_lb_build(t, u, G, cv, ld, p, ns, lane);
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
            const double nb = l0_lb_coord(t[s] + d[s] * u[s], d[s], eta, lam, tauc, big_M);
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
      const L0LbValues v = l0_lb_wave_values(u, t, cv, p, ns, lane, alpha, eta, lam, tauc, big_M);
      if (l0_lb_closed(v.P, v.L, alpha, a.gap_tol)) break;
    }

    // the certificate: t rebuilt from u alone, L and P on it; the cell's own row of every output
    l0_lb_build(t, u, G, cv, ld, p, ns, lane);
    const L0LbValues v = l0_lb_wave_values(u, t, cv, p, ns, lane, alpha, eta, lam, tauc, big_M);
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s)
      if (s < ns) {
        const int j = s * 64 + lane;
        if (j < p) a.u_out[(long long)e * p + j] = u[s];
      }
    if (lane == 0) {
      a.lower_out[e] = v.L > L0 ? v.L : L0;
      a.primal_out[e] = v.P;
      a.stat_out[2 * e] = sweeps;
      a.stat_out[2 * e + 1] = status;
    }
  }
}

}  // namespace slm
