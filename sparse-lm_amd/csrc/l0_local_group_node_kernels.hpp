// The GROUP NODE RELAXATION on chip (slm_solve_l0_local_group_nodes and, round after round, slm_solve_l0_local_group_prove,
// engine_l0.hip; the mathematics, the shared arithmetic, the host twin l0_group_node_solve and the tree: l0_host.hpp, "local
// proof with groups"; DESIGN 4d "Local proof with groups").  The node kernel (l0_local_node_kernels.hpp) bounds a node whose
// COLUMNS are FREE, IN or OUT; here the GROUPS of the grouped local search are, and for EVERY vector u, with t = c - G u,
//     L_node(u) = -1/2 u^T G u - sum over FREE g of max(0, sum_{j in g} h(t_j) - alpha) - sum over IN g of (sum_{j in g} h(t_j) - alpha)
// is at or below the minimum over the node of F = 1/2 beta^T (G + 2 eta I) beta - c^T beta + alpha |cl(S(beta))|.  The older
// kernel stays as it is; this one is its body with the group penalty phi_g in the place of phi.
//
// One WAVEFRONT per NODE, a grid-stride loop over the nodes, coordinate j in lane j & 63, slot j >> 6; u, t and G_jj take 16
// doubles each per lane and every index into them is a compile-time constant; the Gram is read in place through l0_ls_axpy.  A
// node's masks are 16 + 16 words of 64 bits, bit g for GROUP g; a lane packs the two bits of its 16 columns' groups into one
// register at the start of its node, and its columns' group ranges (first column | end << 16) into 16 more at the start of the
// kernel.  What is indexed at run time lives in LDS, PER WAVE: us[j] = u_j and hs[j] = h(t_j), 16 KB a wave, 64 KB a
// workgroup; the waves share nothing and meet at no barrier (l0_lg_sync keeps a wave's own traffic in order).  A lane gets
// R = sum of the other squares of its group, m = their largest modulus and S = sum of h by walking its group's range in
// ascending order: the order of the twin, no floating-point atomic.  At the end of a node the hs table is reused for the marks
// of cl(S(u)), which F(u) counts.
//
// The descent is the twin's, change for change (l0_host.hpp): the next change at or after the cursor is found by ballot; a
// zero group of several columns that passes sum h > alpha moves AS ONE (every lane of the group takes eps b*(t_j), then the
// columns are applied to t in ascending order) and the cursor jumps behind it.  Kernel and twin give the same bits: contraction
// off, the sums in one fixed order, the one contracted step in l0_ls_axpy (std::fma in the twin), the square root of phi_g's
// middle regime correctly rounded on both sides.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "l0_host.hpp"                  // L0_GN_*, l0_gn_*, l0_node_*, l0_lb_*: shared with the host twin
#include "l0_kernels.hpp"               // L0_WAVES, l0_bcast, l0_wave_max, l0_wave_sum
#include "l0_local_kernels.hpp"         // l0_ls_axpy
#include "l0_local_group_kernels.hpp"   // l0_lg_sync, l0_lg_wave_isum
#include "l0_local_node_kernels.hpp"    // L0NdArgs

namespace slm {

struct L0GnArgs {
  L0NdArgs nd;        // the node kernel's arguments; in_mask and out_mask by GROUP
  const int* gof;     // [p]: the column's group
  const int* gstart;  // [ng + 1]
  const int* cptr;    // [ng + 1]: the closed need lists, CSR (all zero without a hierarchy)
  const int* cidx;    // [cptr[ng]]
  int ng;
};

struct L0GnCell {
  double alpha, eta, lam, tauc, big_M, amax;
};

// hs[j] = h(t_j) for the lane's columns
static __device__ __forceinline__ void l0_gn_refresh(const double (&t)[L0_LS_SLOTS], double* hs, int p, int ns, int lane, double eta, double big_M) {
#pragma unroll
  for (int s = 0; s < L0_LS_SLOTS; ++s)
    if (s < ns) {
      const int j = s * 64 + lane;
      if (j < p) hs[j] = l0_node_h(t[s], eta, big_M);
    }
  l0_lg_sync();
}

// P_node(u), L_node(u) and F(u) (the host's l0_gn_values, in its order); st: the lane's packed states, gr: its packed ranges
static __device__ __forceinline__ L0NodeValues l0_gn_wave_values(const double (&u)[L0_LS_SLOTS], const double (&t)[L0_LS_SLOTS],
                                                                 const unsigned (&gr)[L0_LS_SLOTS], const double* __restrict__ cv,
                                                                 const double* us, const double* hs, int p, int ns, int lane, unsigned st,
                                                                 const L0GnCell& ce, double ncl) {
#pragma clang fp contract(off)
  double qp = 0.0, ql = 0.0, sp = 0.0, sc = 0.0, s2 = 0.0;
#pragma unroll
  for (int s = 0; s < L0_LS_SLOTS; ++s)
    if (s < ns) {
      const int j = s * 64 + lane;
      if (j < p) {
        const int state = (int)((st >> (2 * s)) & 3u);
        const double cj = cv[j];
        qp += u[s] * (cj + t[s]);
        ql += u[s] * (cj - t[s]);
        s2 += u[s] * u[s];
        const int lo = (int)(gr[s] & 0xffffu), hi = (int)(gr[s] >> 16);
        if (j == lo) {  // the group's terms, in the lane of its first column
          if (hi - lo == 1) {
            sp += l0_node_phi(u[s], ce.alpha, ce.eta, ce.lam, ce.tauc, state);
            sc += l0_node_conj(t[s], ce.alpha, ce.eta, ce.big_M, state);
          } else {
            double N2 = 0.0, inf = 0.0, S = 0.0;
            for (int k = lo; k < hi; ++k) {
              const double x = us[k], ax = x < 0.0 ? -x : x;
              N2 += x * x;
              inf = ax > inf ? ax : inf;
              S += hs[k];
            }
            sp += l0_gn_group_phi(N2, inf, ce.alpha, ce.eta, ce.big_M, state);
            sc += l0_gn_group_conj(S, ce.alpha, state);
          }
        }
      }
    }
  qp = l0_wave_sum(qp);
  ql = l0_wave_sum(ql);
  sp = l0_wave_sum(sp);
  sc = l0_wave_sum(sc);
  s2 = l0_wave_sum(s2);
  return l0_node_combine(qp, ql, sp, sc, s2, ncl, ce.alpha, ce.eta);
}

// a live column's step at the current state (the twin's, statement by statement); jump: the column's group is zero and moves as
// one, by eps
static __device__ __forceinline__ double l0_gn_step(double uj, double tj, double dj, unsigned grj, int j, int state, const double* us,
                                                    const double* hs, const L0GnCell& ce, bool& jump, double& eps) {
#pragma clang fp contract(off)
  jump = false;
  eps = 0.0;
  const double s = tj + dj * uj;
  const int lo = (int)(grj & 0xffffu), hi = (int)(grj >> 16);
  if (state != L0_ND_FREE || hi - lo == 1) return l0_node_coord(s, dj, ce.eta, ce.lam, ce.tauc, ce.big_M, state);
  double R = 0.0, m = 0.0, S = 0.0;
  for (int k = lo; k < hi; ++k) {
    S += hs[k];
    if (k == j) continue;
    const double x = us[k], ax = x < 0.0 ? -x : x;
    R += x * x;
    m = ax > m ? ax : m;
  }
  if (!(R > 0.0) && uj == 0.0) {
    eps = l0_gn_jump(S, ce.alpha, ce.eta, ce.big_M, ce.amax, hi - lo);
    jump = true;
    return eps * l0_gn_bstar(tj, ce.eta, ce.big_M);
  }
  return !(R > 0.0) ? l0_lb_coord(s, dj, ce.eta, ce.lam, ce.tauc, ce.big_M) : l0_gn_coord(s, dj, R, m, ce.alpha, ce.eta, ce.big_M);
}

static __global__ __launch_bounds__(64 * L0_WAVES) void l0_local_group_node_kernel(L0GnArgs ga) {
#pragma clang fp contract(off)
  __shared__ double us_s[L0_WAVES][L0_LS_PMAX], hs_s[L0_WAVES][L0_LS_PMAX];
  const L0NdArgs& a = ga.nd;
  const int wave = (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  double* us = us_s[wave];
  double* hs = hs_s[wave];
  int* own = reinterpret_cast<int*>(hs);  // (the end of a node: [ng] the groups that hold a non-zero, then [ng] cl(S))
  int* closed = own + L0_LS_PMAX;
  const int p = a.p, ns = (p + 63) >> 6, ng = ga.ng;
  const long long ld = a.ld;
  const double* __restrict__ G = a.G;
  const double* __restrict__ cv = a.c;
  unsigned gr[L0_LS_SLOTS];
#pragma unroll
  for (int s = 0; s < L0_LS_SLOTS; ++s) {
    const int j = s * 64 + lane;
    gr[s] = 0u;
    if (s < ns && j < p) {
      const int g = ga.gof[j];
      gr[s] = (unsigned)ga.gstart[g] | ((unsigned)ga.gstart[g + 1] << 16);
    }
  }
  const int stride = (int)gridDim.x * L0_WAVES;
  for (int e0 = (int)blockIdx.x * L0_WAVES + wave; e0 < a.n_nodes; e0 += stride) {
    const int e = __builtin_amdgcn_readfirstlane(e0);  // the node: one per wave, so a scalar
    const int cell = a.cell[e];
    L0GnCell ce;
    ce.alpha = a.alphas[cell];
    ce.eta = a.etas[cell];
    ce.lam = a.lams[cell];
    ce.tauc = a.taus[cell];
    ce.big_M = a.big_M;
    const double big_M = a.big_M;
    unsigned st = 0;  // the states of the lane's 16 columns' groups, two bits a slot
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s) {
      const int j = s * 64 + lane;
      if (s < ns && j < p) {
        const int g = ga.gof[j];
        const unsigned long long wi = a.in_mask[(long long)e * L0_ND_WORDS + (g >> 6)], wo = a.out_mask[(long long)e * L0_ND_WORDS + (g >> 6)];
        st |= ((unsigned)((wi >> (g & 63)) & 1ull) | ((unsigned)((wo >> (g & 63)) & 1ull) << 1)) << (2 * s);
      }
    }
    double u[L0_LS_SLOTS], t[L0_LS_SLOTS], d[L0_LS_SLOTS];
    double dmax = 0.0;
    l0_lg_sync();  // (the previous node's reads of the tables are done)
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s) {
      const int j = s * 64 + lane;
      u[s] = 0.0;
      t[s] = 0.0;
      d[s] = 0.0;
      if (s < ns && j < p) {
        d[s] = G[(long long)j * ld + j];
        t[s] = cv[j];
        us[j] = 0.0;
      }
      dmax = fmax(dmax, d[s]);
    }
    dmax = l0_wave_max(dmax);
    ce.amax = dmax;
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s)  // d = 0 marks a column that keeps u_j = 0: a failed pivot, an OUT group's, a lane beyond p
      if (!(d[s] > L0_PIVOT * dmax) || ((st >> (2 * s)) & 3u) == (unsigned)L0_ND_OUT) d[s] = 0.0;
    l0_gn_refresh(t, hs, p, ns, lane, ce.eta, big_M);
    const double L0 = l0_gn_wave_values(u, t, gr, cv, us, hs, p, ns, lane, st, ce, 0.0).L;  // L_node(0): u = 0, t = c
    if (a.starts) {
#pragma unroll
      for (int s = 0; s < L0_LS_SLOTS; ++s) {
        const int j = s * 64 + lane;
        if (s < ns && j < p && d[s] > 0.0) {
          const double v = a.starts[(long long)e * p + j];
          u[s] = v < -big_M ? -big_M : (v > big_M ? big_M : v);  // clipped into the box
          us[j] = u[s];
        }
      }
      l0_nd_build(t, u, G, cv, ld, p, ns, lane);
      l0_gn_refresh(t, hs, p, ns, lane, ce.eta, big_M);
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
        bool found = false, group_move = false;
        int jf = 0, glo = 0, ghi = 0;
        double delta = 0.0, epsb = 0.0;
#pragma unroll
        for (int s = 0; s < L0_LS_SLOTS; ++s)
          if (!found && s >= s0 && s < ns) {
            const int j = s * 64 + lane;
            bool jump = false;
            double eps = 0.0, nb = 0.0;
            if (d[s] > 0.0 && j >= cursor) nb = l0_gn_step(u[s], t[s], d[s], gr[s], j, (int)((st >> (2 * s)) & 3u), us, hs, ce, jump, eps);
            const unsigned long long bal = __ballot(d[s] > 0.0 && j >= cursor && l0_lb_changed(nb, u[s]));
            if (bal) {
              const int k = __builtin_ctzll(bal);
              const double nbk = l0_bcast(nb, k), old = l0_bcast(u[s], k);
              group_move = ((__ballot(jump) >> k) & 1ull) != 0;
              found = true;
              jf = s * 64 + k;
              if (group_move) {
                epsb = l0_bcast(eps, k);
                const unsigned range = (unsigned)__builtin_amdgcn_readlane((int)gr[s], k);
                glo = (int)(range & 0xffffu);
                ghi = (int)(range >> 16);
              } else {
                if (lane == k) {
                  u[s] = nbk;
                  us[jf] = nbk;
                }
                delta = nbk - old;
              }
            }
          }
        if (!found) break;
        if (group_move) {  // every live column of the group takes eps b*(t_j) at the t of now; then the columns go into t, ascending
#pragma unroll
          for (int s = 0; s < L0_LS_SLOTS; ++s)
            if (s < ns) {
              const int j = s * 64 + lane;
              if (j >= glo && j < ghi && d[s] > 0.0) {
                u[s] = epsb * l0_gn_bstar(t[s], ce.eta, big_M);
                us[j] = u[s];
              }
            }
#pragma unroll
          for (int s = 0; s < L0_LS_SLOTS; ++s)
            if (s < ns) {
              const int j = s * 64 + lane;
              unsigned long long act = __ballot(j >= glo && j < ghi && u[s] != 0.0);
              while (act) {
                const int k = __builtin_ctzll(act);
                act &= act - 1;
                l0_ls_axpy(t, G, ld, p, ns, lane, 0.0, s * 64 + k, -l0_bcast(u[s], k));
              }
            }
          cursor = ghi;
        } else {
          l0_ls_axpy(t, G, ld, p, ns, lane, 0.0, jf, -delta);
          cursor = jf + 1;
        }
        l0_gn_refresh(t, hs, p, ns, lane, ce.eta, big_M);
      }
      ++sweeps;
      const L0NodeValues v = l0_gn_wave_values(u, t, gr, cv, us, hs, p, ns, lane, st, ce, 0.0);
      if (l0_lb_closed(v.P, v.L, ce.alpha, a.gap_tol)) break;
    }

    // |cl(S(u))| through the marks (the hs table is rebuilt below)
    l0_lg_sync();
    for (int g = lane; g < ng; g += 64) {
      int any = 0;
      const int hi = ga.gstart[g + 1];
      for (int k = ga.gstart[g]; k < hi; ++k) any |= us[k] != 0.0 ? 1 : 0;
      own[g] = any;
      closed[g] = any;
    }
    l0_lg_sync();
    for (int g = lane; g < ng; g += 64)
      if (own[g]) {
        const int hi = ga.cptr[g + 1];
        for (int k = ga.cptr[g]; k < hi; ++k) closed[ga.cidx[k]] = 1;  // (every writer writes 1)
      }
    l0_lg_sync();
    int count = 0;
    for (int g = lane; g < ng; g += 64) count += closed[g];
    const double ncl = (double)l0_lg_wave_isum(count);
    l0_lg_sync();

    // the certificate: t rebuilt from u alone, L, P and F on it; the node's own row of every output
    l0_nd_build(t, u, G, cv, ld, p, ns, lane);
    l0_gn_refresh(t, hs, p, ns, lane, ce.eta, big_M);
    const L0NodeValues v = l0_gn_wave_values(u, t, gr, cv, us, hs, p, ns, lane, st, ce, ncl);
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
