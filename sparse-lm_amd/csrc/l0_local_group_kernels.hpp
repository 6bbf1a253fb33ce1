// The l0 LOCAL SEARCH WITH GROUPS AND A HIERARCHY on chip (slm_solve_l0_local_groups, engine_l0.hip; the rule and its host twin
// l0_lg_solve: l0_host.hpp, "local groups"; DESIGN 4d "Local search with groups").  For a cell (alpha, eta), H = G + 2 eta I,
//     F(beta) = 1/2 beta^T H beta - c^T beta + alpha |cl(S(beta))|,   |beta_j| <= big_M,
// S the groups that hold a non-zero, cl the closure under the hierarchy: a group descent (a step fits a whole group, values it
// exactly and keeps it iff the value beats alpha times what it adds to |cl(S)|), then one-for-one GROUP swaps until none helps.
// Nothing is proven, and the screen that spares an inactive group its trial fit is a heuristic (L0_LG_SCREEN).
//
// The mapping is l0_local_kernel's (l0_local_kernels.hpp): one WAVEFRONT per (row set, cell, start) problem, a grid-stride loop
// over the problems, column j in lane j & 63, slot j >> 6, every slot index a compile-time constant; the Grams read in place
// with their leading dimension, up to 16 row sets by scalar pointer choice, each problem owning its row of every output.
// Groups are contiguous column ranges (gstart), so a column's group needs no table: membership is a range test.  Beside beta, r
// and d the registers hold r' (the residual with a group taken out) and the saved beta and r of a swap's trial.
//
// What is indexed at run time lives in LDS, PER WAVE: nz[g], held[g] (ints, 1024 each) and a column scratch of 1024 doubles --
// 16 KB a wave, 64 KB a workgroup.  The waves of a workgroup share nothing and meet at no barrier: a wave's LDS traffic is in
// program order, l0_lg_sync only keeps the compiler from moving it.  The tables are set up again for every problem a wave takes.
// Sums over a group -- C_g, v_g -- go through the scratch and are added by ONE lane (C_g: the lane that owns the group) or by
// every lane alike (v_g) walking the column range in ascending order: the order of the twin, no floating-point atomic.
//
// A step's cost: |g| dependent row reads per inner pass that changes something, |g| independent ones for r'.  After a step that
// changed r or a table, every lane re-screens its groups (g = lane, lane + 64, ..) at once; the next group that gets a step is
// the lowest flagged one at or after the cursor: the sequence of the sequential rule.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "l0_host.hpp"            // L0_LG_*, L0_LS_*, l0_ls_coord: shared with the host twin
#include "l0_local_kernels.hpp"   // l0_ls_axpy, l0_ls_wave_min

namespace slm {

struct L0LgArgs {
  const double* G[L0_LS_ROW_SETS];  // [p][ld] per row set: a filed Gram in place, or the call's eliminated copy
  const double* c[L0_LS_ROW_SETS];  // [p] per row set
  double yy[L0_LS_ROW_SETS];
  const double* alphas;  // [n_cells]
  const double* etas;    // [n_cells]
  const double* starts;  // [n_problems][p] inside the box, or NULL: zero
  const int* gstart;     // [ng + 1]: group g is the columns gstart[g] .. gstart[g + 1] - 1
  const int* cptr;       // [ng + 1]: the closed need lists, CSR (all zero without a hierarchy)
  const int* cidx;       // [cptr[ng]], every entry in 0 .. ng - 1
  double* beta_out;      // [n_problems][p]
  double* F_out;         // [n_problems]
  int* stat_out;         // [n_problems][L0_LG_STATS]: sweeps, swaps, status word, |cl(S)|, non-zero columns, group trials
  long long ld;
  int p, ng, n_problems, n_starts, swaps, n_cells;
  double big_M;
};

// what a wave's helpers share: the problem's scalars and the wave's own LDS
struct L0LgWave {
  const double* G;
  const int *gstart, *cptr, *cidx;
  int *nz, *held;
  double* scr;
  long long ld;
  int p, ns, ng, lane;
  double eta2, big_M, tol, alpha;
};
struct L0LgRegs {
  double beta[L0_LS_SLOTS], r[L0_LS_SLOTS], d[L0_LS_SLOTS];
};

static __device__ __forceinline__ void l0_lg_sync() {  // one wave: order, not arrival
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
static __device__ __forceinline__ int l0_lg_wave_isum(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
// entry j = 64 slot + k of a register row, in every lane (j wave-uniform)
static __device__ __forceinline__ double l0_lg_at(const double (&x)[L0_LS_SLOTS], int j) {
  double v = 0.0;
#pragma unroll
  for (int t = 0; t < L0_LS_SLOTS; ++t)
    if (t == (j >> 6)) v = x[t];
  return l0_bcast(v, j & 63);
}
static __device__ __forceinline__ void l0_lg_axpy(double (&x)[L0_LS_SLOTS], const L0LgWave& w, int j, double by) {
  l0_ls_axpy(x, w.G, w.ld, w.p, w.ns, w.lane, w.eta2, j, by);
}

// m_g for a wave-uniform g (the lanes share the list), and for a lane's own g (the lane walks it alone)
static __device__ __forceinline__ int l0_lg_price(const L0LgWave& w, int g) {
  if (w.held[g] > 0) return 0;
  const int own = w.nz[g] > 0 ? 1 : 0, hi = w.cptr[g + 1];
  int m = 0;
  for (int k = w.cptr[g] + w.lane; k < hi; k += 64) {
    const int h = w.cidx[k];
    m += w.nz[h] == 0 && w.held[h] == own;
  }
  return 1 + l0_lg_wave_isum(m);
}
static __device__ __forceinline__ int l0_lg_price_lane(const L0LgWave& w, int g) {
  if (w.held[g] > 0) return 0;
  const int own = w.nz[g] > 0 ? 1 : 0, hi = w.cptr[g + 1];
  int m = 1;
  for (int k = w.cptr[g]; k < hi; ++k) {
    const int h = w.cidx[k];
    m += w.nz[h] == 0 && w.held[h] == own;
  }
  return m;
}
// held_h += by for h in need*(g): the entries of a closed list are distinct, so the lanes write different words
static __device__ __forceinline__ void l0_lg_hold(const L0LgWave& w, int g, int by) {
  const int hi = w.cptr[g + 1];
  for (int k = w.cptr[g] + w.lane; k < hi; k += 64) w.held[w.cidx[k]] += by;
  l0_lg_sync();
}
// the coordinate gains at the current r into the scratch (0 for a column that stays out)
static __device__ __forceinline__ void l0_lg_gains(const L0LgRegs& s, const L0LgWave& w) {
#pragma unroll
  for (int t = 0; t < L0_LS_SLOTS; ++t)
    if (t < w.ns) {
      const int j = t * 64 + w.lane;
      if (j < w.p) w.scr[j] = s.d[t] > 0.0 ? l0_ls_coord(s.r[t], s.d[t], w.big_M).gain : 0.0;
    }
  l0_lg_sync();
}
static __device__ __forceinline__ double l0_lg_walk(const L0LgWave& w, int g) {  // the scratch summed over group g, ascending
  double C = 0.0;
  const int hi = w.gstart[g + 1];
  for (int j = w.gstart[g]; j < hi; ++j) C += w.scr[j];
  return C;
}
static __device__ __forceinline__ int l0_lg_count(const L0LgRegs& s, const L0LgWave& w, int lo, int hi) {
  int n = 0;
#pragma unroll
  for (int t = 0; t < L0_LS_SLOTS; ++t)
    if (t < w.ns) {
      const int j = t * 64 + w.lane;
      n += __popcll(__ballot(j >= lo && j < hi && s.beta[t] != 0.0));
    }
  return n;
}
// the inner passes over the columns lo .. hi - 1; the largest |delta| sqrt(d) of any pass
static __device__ __forceinline__ double l0_lg_fit(L0LgRegs& s, const L0LgWave& w, int lo, int hi, bool& changed) {
  double worst = 0.0;
  for (int pass = 0; pass < L0_LG_INNER; ++pass) {
    double mp = 0.0;
    for (int j = lo; j < hi; ++j) {
      const double dj = l0_lg_at(s.d, j);
      if (!(dj > 0.0)) continue;
      const double bj = l0_lg_at(s.beta, j), rj = l0_lg_at(s.r, j);
      const double b = l0_ls_coord(rj + dj * bj, dj, w.big_M).b, delta = b - bj;
      if (delta == 0.0) continue;
#pragma unroll
      for (int t = 0; t < L0_LS_SLOTS; ++t)
        if (t == (j >> 6) && w.lane == (j & 63)) s.beta[t] = b;
      l0_lg_axpy(s.r, w, j, -delta);
      changed = true;
      mp = fmax(mp, fabs(delta) * sqrt(dj));
    }
    worst = fmax(worst, mp);
    if (mp <= w.tol) break;
  }
  return worst;
}
// v = 1/2 beta_g^T (r_g + r'_g); rp <- r' = r + sum_{j in g} H[:, j] beta_j
static __device__ __forceinline__ double l0_lg_value(const L0LgRegs& s, const L0LgWave& w, int lo, int hi, double (&rp)[L0_LS_SLOTS]) {
#pragma unroll
  for (int t = 0; t < L0_LS_SLOTS; ++t) rp[t] = s.r[t];
  for (int j = lo; j < hi; ++j) {
    const double bj = l0_lg_at(s.beta, j);
    if (bj != 0.0) l0_lg_axpy(rp, w, j, bj);
  }
#pragma unroll
  for (int t = 0; t < L0_LS_SLOTS; ++t)
    if (t < w.ns) {
      const int j = t * 64 + w.lane;
      if (j >= lo && j < hi) w.scr[j] = s.beta[t] * (s.r[t] + rp[t]);
    }
  l0_lg_sync();
  double v = 0.0;
  for (int j = lo; j < hi; ++j) v += w.scr[j];
  l0_lg_sync();  // (the scratch is free again)
  return 0.5 * v;
}
static __device__ __forceinline__ void l0_lg_empty(L0LgRegs& s, const L0LgWave& w, int lo, int hi, const double (&rp)[L0_LS_SLOTS]) {
#pragma unroll
  for (int t = 0; t < L0_LS_SLOTS; ++t) {
    const int j = t * 64 + w.lane;
    if (j >= lo && j < hi) s.beta[t] = 0.0;
    s.r[t] = rp[t];
  }
}
static __device__ __forceinline__ void l0_lg_set(const L0LgWave& w, int* table, int g, int v) {
  if (w.lane == 0) table[g] = v;
  l0_lg_sync();
}

static __global__ __launch_bounds__(64 * L0_WAVES) void l0_local_group_kernel(L0LgArgs a) {
  __shared__ int nz_s[L0_WAVES][L0_LS_PMAX], held_s[L0_WAVES][L0_LS_PMAX];
  __shared__ double scr_s[L0_WAVES][L0_LS_PMAX];
  const int wave = (int)(threadIdx.x >> 6);
  L0LgWave w;
  w.lane = threadIdx.x & 63;
  w.p = a.p;
  w.ns = (a.p + 63) >> 6;
  w.ng = a.ng;
  w.ld = a.ld;
  w.big_M = a.big_M;
  w.gstart = a.gstart;
  w.cptr = a.cptr;
  w.cidx = a.cidx;
  w.nz = nz_s[wave];
  w.held = held_s[wave];
  w.scr = scr_s[wave];
  const int lane = w.lane, p = w.p, ns = w.ns, ng = w.ng;
  const int stride = (int)gridDim.x * L0_WAVES;
  for (int q = (int)blockIdx.x * L0_WAVES + wave; q < a.n_problems; q += stride) {
    const int rc = q / a.n_starts;                                  // r * n_cells + e
    const int rs = __builtin_amdgcn_readfirstlane(rc / a.n_cells);  // the row set: one per wave, so a scalar
    const int cell = rc - rs * a.n_cells;
    w.G = a.G[rs];
    const double* __restrict__ cv = a.c[rs];
    w.tol = L0_CD_TOL * sqrt(a.yy[rs]);
    w.alpha = a.alphas[cell];
    w.eta2 = 2.0 * a.etas[cell];
    const double alpha = w.alpha, tol = w.tol;
    L0LgRegs s;
    double rp[L0_LS_SLOTS], sb[L0_LS_SLOTS], sr[L0_LS_SLOTS];
    double dmax = 0.0;
#pragma unroll
    for (int t = 0; t < L0_LS_SLOTS; ++t) {
      const int j = t * 64 + lane;
      s.beta[t] = 0.0;
      s.r[t] = 0.0;
      s.d[t] = 0.0;
      if (t < ns && j < p) {
        s.d[t] = w.G[(long long)j * w.ld + j] + w.eta2;
        s.r[t] = cv[j];
        if (a.starts) s.beta[t] = a.starts[(long long)q * p + j];
      }
      dmax = fmax(dmax, s.d[t]);
    }
    dmax = l0_wave_max(dmax);
#pragma unroll
    for (int t = 0; t < L0_LS_SLOTS; ++t)
      if (!(s.d[t] > L0_PIVOT * dmax)) {  // d = 0 marks a column that stays out (and the lanes beyond p)
        s.d[t] = 0.0;
        s.beta[t] = 0.0;
      }
    // r = c - H beta of the start, column by column in ascending order
#pragma unroll
    for (int t = 0; t < L0_LS_SLOTS; ++t)
      if (t < ns) {
        unsigned long long act = __ballot(s.beta[t] != 0.0);
        while (act) {
          const int k = __builtin_ctzll(act);
          act &= act - 1;
          l0_lg_axpy(s.r, w, t * 64 + k, -l0_bcast(s.beta[t], k));
        }
      }
    // the tables of this problem: nz from the start (through the scratch: a lane counts its own groups), then held
    l0_lg_sync();  // (the previous problem's reads are done)
#pragma unroll
    for (int t = 0; t < L0_LS_SLOTS; ++t)
      if (t < ns) {
        const int j = t * 64 + lane;
        if (j < p) w.scr[j] = s.beta[t] != 0.0 ? 1.0 : 0.0;
      }
    for (int g = lane; g < ng; g += 64) w.held[g] = 0;
    l0_lg_sync();
    for (int g = lane; g < ng; g += 64) w.nz[g] = (int)l0_lg_walk(w, g);
    l0_lg_sync();
    for (int g = lane; g < ng; g += 64)
      if (w.nz[g] > 0) {
        const int hi = w.cptr[g + 1];
        for (int k = w.cptr[g]; k < hi; ++k) atomicAdd(&w.held[w.cidx[k]], 1);  // (integers in LDS: several lanes may hold one group)
      }
    l0_lg_sync();

    int sweeps = 0, swaps = 0, status = 0, trials = 0;
    for (;;) {
      // ---- 1. the group descent to its fixed point ----------------------------------------------------------------------------
      for (int sw = 0;; ++sw) {
        if (sw == L0_CD_SWEEPS) {
          status |= L0_LS_SWEEPS_OUT;
          break;
        }
        bool moved = false, dirty = true;
        double maxd = 0.0;
        int cursor = 0;
        unsigned flags = 0;  // bit k: group 64 k + lane gets a step at the current r and tables
        for (;;) {
          if (dirty) {
            l0_lg_gains(s, w);
            flags = 0;
            for (int k = 0; k * 64 < ng; ++k) {
              const int g = k * 64 + lane;
              if (g >= ng) continue;
              bool step = w.nz[g] > 0 || w.held[g] > 0;
              if (!step) {
                const double C = l0_lg_walk(w, g);
                if (C > alpha / L0_LG_SCREEN)  // (m_g >= 1 here: only then is the list worth a walk)
                  step = C > alpha * (double)l0_lg_price_lane(w, g) / L0_LG_SCREEN;
              }
              if (step) flags |= 1u << k;
            }
            l0_lg_sync();
            dirty = false;
          }
          const int k0 = cursor > lane ? (cursor - lane + 63) >> 6 : 0;
          const unsigned left = k0 < 16 ? flags & (~0u << k0) : 0u;
          const int g = l0_ls_wave_min(left ? __builtin_ctz(left) * 64 + lane : 0x7fffffff);
          if (g == 0x7fffffff) break;
          cursor = g + 1;
          const int lo = w.gstart[g], hi = w.gstart[g + 1];
          const bool was = w.nz[g] > 0;
          if (!was && w.held[g] == 0) ++trials;
          const int m = l0_lg_price(w, g);
          bool changed = false;
          const double worst = l0_lg_fit(s, w, lo, hi, changed);
          const double v = l0_lg_value(s, w, lo, hi, rp);
          if (v > alpha * (double)m) {
            const int now = l0_lg_count(s, w, lo, hi);
            if ((now > 0) != was) {
              l0_lg_hold(w, g, now > 0 ? 1 : -1);
              moved = true;
              changed = true;
            }
            l0_lg_set(w, w.nz, g, now);
            maxd = fmax(maxd, worst);
          } else {
            l0_lg_empty(s, w, lo, hi, rp);
            l0_lg_set(w, w.nz, g, 0);
            if (was) {
              l0_lg_hold(w, g, -1);
              moved = true;
            }
            changed = true;
          }
          dirty = changed;
        }
        ++sweeps;
        if (!moved && maxd <= tol) break;
      }
      if (!a.swaps || status) break;
      // ---- 2. the group swap scan: the first i that an empty group replaces with a gain ------------------------------------------
      bool swapped = false;
      for (int i = 0; i < ng && !swapped; ++i) {
        const int nzi = w.nz[i];
        if (nzi == 0 || w.held[i] > 0) continue;
#pragma unroll
        for (int t = 0; t < L0_LS_SLOTS; ++t) {
          sb[t] = s.beta[t];
          sr[t] = s.r[t];
        }
        const int ilo = w.gstart[i], ihi = w.gstart[i + 1];
        const int mi = l0_lg_price(w, i);
        const double vi = l0_lg_value(s, w, ilo, ihi, rp);
        l0_lg_empty(s, w, ilo, ihi, rp);
        l0_lg_set(w, w.nz, i, 0);
        l0_lg_hold(w, i, -1);
        // the candidate: every lane's best over its own empty groups, then the wave's (ties: the lowest group)
        l0_lg_gains(s, w);
        double best = -HUGE_VAL;
        int jb = 0x7fffffff;
        for (int k = 0; k * 64 < ng; ++k) {
          const int g = k * 64 + lane;
          if (g >= ng || g == i || w.nz[g] > 0) continue;
          const double C = l0_lg_walk(w, g);
          if (w.held[g] == 0 && !(C - alpha > best)) continue;  // (m_g >= 1: it cannot lead)
          const double score = C - alpha * (double)l0_lg_price_lane(w, g);
          if (score > best) {  // (ascending k: the lane keeps its lowest g on ties)
            best = score;
            jb = g;
          }
        }
        l0_lg_sync();
        const double lead = l0_wave_max(best);
        const int j = l0_ls_wave_min(best == lead ? jb : 0x7fffffff);
        bool ok = false;
        int jlo = 0, jhi = 0;
        if (j != 0x7fffffff) {
          jlo = w.gstart[j];
          jhi = w.gstart[j + 1];
          const int mj = l0_lg_price(w, j);
          bool changed = false;
          ++trials;
          l0_lg_fit(s, w, jlo, jhi, changed);
          const double vj = l0_lg_value(s, w, jlo, jhi, rp), av = fabs(vi);
          ok = vj - alpha * (double)mj > vi - alpha * (double)mi + L0_LS_SWAP_TOL * (av > alpha ? av : alpha);
        }
        if (ok) {
          const int now = l0_lg_count(s, w, jlo, jhi);
          l0_lg_set(w, w.nz, j, now);
          if (now > 0) l0_lg_hold(w, j, 1);
          ++swaps;
          swapped = true;
        } else {
#pragma unroll
          for (int t = 0; t < L0_LS_SLOTS; ++t) {
            s.beta[t] = sb[t];
            s.r[t] = sr[t];
          }
          l0_lg_set(w, w.nz, i, nzi);
          l0_lg_hold(w, i, 1);
        }
      }
      if (!swapped) break;
      if (swaps == L0_LS_SWAPS) {
        status |= L0_LS_SWAPS_OUT;
        break;
      }
    }

    // F = 1/2 beta^T H beta - c^T beta + alpha |cl(S)| with H beta = c - r; the problem's own row of every output
    double acc = 0.0;
    int nnz = 0, closed = 0;
#pragma unroll
    for (int t = 0; t < L0_LS_SLOTS; ++t)
      if (t < ns) {
        const int j = t * 64 + lane;
        if (j < p) {
          acc += s.beta[t] * (cv[j] + s.r[t]);
          nnz += s.beta[t] != 0.0;
          a.beta_out[(long long)q * p + j] = s.beta[t];
        }
      }
    for (int g = lane; g < ng; g += 64) closed += w.nz[g] > 0 || w.held[g] > 0;
    acc = l0_wave_sum(acc);
    nnz = l0_lg_wave_isum(nnz);
    closed = l0_lg_wave_isum(closed);
    if (lane == 0) {
      a.F_out[q] = -0.5 * acc + alpha * (double)closed;
      int* stat = a.stat_out + (long long)q * L0_LG_STATS;
      stat[0] = sweeps;
      stat[1] = swaps;
      stat[2] = status;
      stat[3] = closed;
      stat[4] = nnz;
      stat[5] = trials;
    }
  }
}

}  // namespace slm
