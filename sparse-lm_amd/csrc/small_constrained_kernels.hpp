// Linear constraints lo <= A b <= hi on the l1 estimators (the reference's add_constraints, src/sparselm/model/_base.py:
// 469-510) on chip: the splitting of sparselm_amd/model/_constrained.py with ALL of its sweeps in one launch, for the
// problem sizes of small_kernels.hpp.
//
//     b  <- argmin 1/(2n)||X b - y||^2 + sum_j a_j |b_j| + rho/2 ||A b - s + u||^2
//     v  =  A b;   vh = 1.6 v + (1 - 1.6) s
//     s  <- clip(vh + u, lo, hi);   u <- u + vh - s;   lambda = rho u
//
// The Gram matrix G = X^T X / n is built once in LDS and turned into the b-step's matrix G + rho K (K = A^T A, kept in
// global memory with A) in place; a change of rho adds (rho' - rho) K, and the exit takes rho K off again for the loss.
// The b-step is then a weighted Lasso with linear term c + rho A^T (s - u): the b-step of small_bstep.hpp -- shared with
// small_split_kernels.hpp -- on the matrix in LDS as it stands.  What is here is the splitting itself: the products with A
// and A^T, the s / u steps, the residuals, the re-balancing of rho and the stopping rule of _constrained.py.  s, u, lo and
// hi live in registers: lane l holds rows l, l + 64, ... (m <= 512: eight per lane).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "small_bstep.hpp"

namespace slm {

constexpr int SC_MMAX = 512;          // constraint rows
constexpr int SC_RPL = SC_MMAX / 64;  // rows per lane
constexpr int SC_STATE = 2 * SC_MMAX + 8;  // s [SC_MMAX], u [SC_MMAX], rho, valid, m, direct b-steps, factorisations

struct ConstrainedArgs {
  const double* X;     // [n][ld]
  const double* y;
  int64_t n, ld;
  int p, m;
  const int* order;    // identity (singleton groups)
  const double* a;     // [p] l1 weights
  const double* A;     // [m][p]
  const double* At;    // [p][m]
  const double* K;     // [p][p] = A^T A
  const double* lo;    // [m]
  const double* hi;    // [m]
  const double* beta0; // [p] warm start (nullptr: zero)
  double* beta_out;    // [p]
  double* lambda_out;  // [m] rho u
  slm_point_info* info;  // [1]: n_iter = sweeps, rejects = matrix-vector products, kkt / mu = primal / dual residual, L = rho
  double* state;       // [SC_STATE] kept with the dataset
  int warm;            // continue from `state` (the re-weighting rounds of AdaptiveLasso)
  double tol, tol_inner, inv_n;
  int max_sweeps, max_iters, stage_doubles;
};

constexpr double SC_RELAX = 1.6;

static __global__ __launch_bounds__(SM_THREADS) void small_constrained_kernel(ConstrainedArgs a) {
  extern __shared__ double sm_lds[];  // G [p][p], c [p], vz [p], vu [p], wv [SC_MMAX], then the stage
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = a.p, m = a.m;
  double* Gs = sm_lds;
  double* cs = Gs + p * p;
  double* vz = cs + p;
  double* vu = vz + p;
  double* wv = vu + p;
  double* stage = wv + SC_MMAX;
  __shared__ double yy_s;
  __shared__ int sm_cmd, sm_m;
  const bool built = sm_build_gram(a.X, a.y, nullptr, a.n, a.ld, p, a.order, a.inv_n, a.stage_doubles, Gs, cs, stage, &yy_s);
  // (the stage of the build is free now: partial products, then the head of the direct solves)
  SbStep bs = sb_setup(Gs, vz, vu, stage, 0, p, a.stage_doubles, &sm_cmd, &sm_m, lane, a.tol_inner, a.max_iters);
  auto face_factor = [&](int mf, bool worker) { sb_face_factor(bs, mf, worker); };  // a face of the matrix in LDS
  if (wave != 0) {
    sb_serve(bs, wave, face_factor);
    return;
  }
  const int s0 = bs.s0, s1 = bs.s1;
  const bool on0 = bs.on0, on1 = bs.on1;
  const double c0 = on0 ? cs[s0] : 0.0, c1 = on1 ? cs[s1] : 0.0;
  const double thr0 = on0 ? a.a[s0] : 0.0, thr1 = on1 ? a.a[s1] : 0.0;
  bs.thr0 = thr0;
  bs.thr1 = thr1;

  // y = (G + rho K) v, the matrix in LDS
  auto matvec = [&](double v0, double v1, double& y0, double& y1) { sb_matvec(bs, v0, v1, y0, y1); };
  // v = A x: the lane's rows, coalesced over the rows of A^T
  auto mul_A = [&](double x0, double x1, double (&v)[SC_RPL]) {
    if (on0) vu[s0] = x0;
    if (on1) vu[s1] = x1;
    sm_lds_sync();
#pragma unroll
    for (int k = 0; k < SC_RPL; ++k) {
      const int r = lane + 64 * k;
      double t = 0.0;
      if (r < m)
        for (int j = 0; j < p; ++j) t = __builtin_fma(a.At[(int64_t)j * m + r], vu[j], t);
      v[k] = t;
    }
    __builtin_amdgcn_wave_barrier();
  };
  // (A^T w, A^T z) at the lane's positions, coalesced over the columns of A; rows beyond m hold zero
  auto mul_At2 = [&](const double (&w)[SC_RPL], const double (&z)[SC_RPL], double& y0, double& y1, double& t0, double& t1) {
#pragma unroll
    for (int k = 0; k < SC_RPL; ++k) {
      const int r = lane + 64 * k;
      if (r < m) wv[r] = w[k];
    }
    sm_lds_sync();
    y0 = y1 = 0.0;
    for (int r = 0; r < m; ++r) {
      const double wr = wv[r];
      if (on0) y0 = __builtin_fma(a.A[(int64_t)r * p + s0], wr, y0);
      if (on1) y1 = __builtin_fma(a.A[(int64_t)r * p + s1], wr, y1);
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < SC_RPL; ++k) {
      const int r = lane + 64 * k;
      if (r < m) wv[r] = z[k];
    }
    sm_lds_sync();
    t0 = t1 = 0.0;
    for (int r = 0; r < m; ++r) {
      const double zr = wv[r];
      if (on0) t0 = __builtin_fma(a.A[(int64_t)r * p + s0], zr, t0);
      if (on1) t1 = __builtin_fma(a.A[(int64_t)r * p + s1], zr, t1);
    }
    __builtin_amdgcn_wave_barrier();
  };
  // Gs += f K (wavefront 0 alone: the helpers are parked at the barrier of their next command)
  auto add_K = [&](double f) {
    for (int e = lane; e < p * p; e += 64) Gs[e] = __builtin_fma(f, a.K[e], Gs[e]);
    sm_lds_sync();
  };

  slm_point_info info;
  memset(&info, 0, sizeof(info));
  info.mode = 3;
  info.status = SLM_ERR_NOT_CONVERGED;
  if (!built) {
    if (lane == 0) a.info[0] = info;
    sb_release(bs);
    return;
  }

  // ---- scales and state --------------------------------------------------------------------------------------------
  // rho starts where rho K has the trace of G (the coupling then weighs like the loss); `kap` = sqrt(trace K / p), the
  // rms column norm of A, puts kap ||b|| beside ||A b|| in the primal scale; ||c|| floors the dual one (see _constrained.py)
  const double trG = sm_sum((on0 ? Gs[s0 * p + s0] : 0.0) + (on1 ? Gs[s1 * p + s1] : 0.0));
  const double trK = sm_sum((on0 ? a.K[s0 * p + s0] : 0.0) + (on1 ? a.K[s1 * p + s1] : 0.0));
  const double kap = sqrt(trK / (double)p);
  const double cnorm = sqrt(sm_sum(c0 * c0 + c1 * c1));
  double lo_r[SC_RPL], hi_r[SC_RPL], s_r[SC_RPL], u_r[SC_RPL];
#pragma unroll
  for (int k = 0; k < SC_RPL; ++k) {
    const int r = lane + 64 * k;
    lo_r[k] = r < m ? a.lo[r] : 0.0;
    hi_r[k] = r < m ? a.hi[r] : 0.0;
    s_r[k] = 0.0;
    u_r[k] = 0.0;
  }
  SbState st;
  memset(&st, 0, sizeof(st));
  st.f_key = -1.0;
  double& x0 = st.x0;
  double& x1 = st.x1;
  x0 = (on0 && a.beta0) ? a.beta0[s0] : 0.0;
  x1 = (on1 && a.beta0) ? a.beta0[s1] : 0.0;
  double rho = (trK > 0.0 && trG > 0.0) ? trG / trK : a.inv_n;
  const bool resume = a.warm && a.state[SC_MMAX * 2 + 1] == 1.0 && a.state[SC_MMAX * 2 + 2] == (double)m;
  if (resume) {
#pragma unroll
    for (int k = 0; k < SC_RPL; ++k) {
      const int r = lane + 64 * k;
      if (r < m) { s_r[k] = a.state[r]; u_r[k] = a.state[SC_MMAX + r]; }
    }
    rho = a.state[2 * SC_MMAX];
  } else {
    double v[SC_RPL];
    mul_A(x0, x1, v);
#pragma unroll
    for (int k = 0; k < SC_RPL; ++k) s_r[k] = lane + 64 * k < m ? fmin(fmax(v[k], lo_r[k]), hi_r[k]) : 0.0;
  }
  add_K(rho);
  double L = sb_lambda_max(bs, matvec);
  st.products = 12;

  // ---- the sweeps --------------------------------------------------------------------------------------------------
  int sweeps = 0;
  bool converged = false;
  double rp = 0.0, rd = 0.0;
  for (sweeps = 1; sweeps <= a.max_sweeps && !st.bad; ++sweeps) {
    double w[SC_RPL], zz[SC_RPL];
#pragma unroll
    for (int k = 0; k < SC_RPL; ++k) {
      w[k] = s_r[k] - u_r[k];
      zz[k] = 0.0;
    }
    double t0, t1, dum0, dum1;
    mul_At2(w, zz, t0, t1, dum0, dum1);
    const double ce0 = __builtin_fma(rho, t0, c0), ce1 = __builtin_fma(rho, t1, c1);
    if (!sb_direct(bs, st, matvec, face_factor, rho, L, ce0, ce1)) (void)sb_inner(bs, st, matvec, ce0, ce1, L);
    if (st.bad) break;
    double v[SC_RPL], ds_r[SC_RPL];
    mul_A(x0, x1, v);
    double s_rp = 0.0, s_v = 0.0, s_s = 0.0;
#pragma unroll
    for (int k = 0; k < SC_RPL; ++k) {
      const bool live = lane + 64 * k < m;
      const double vh = SC_RELAX * v[k] + (1.0 - SC_RELAX) * s_r[k];
      const double sn = live ? fmin(fmax(vh + u_r[k], lo_r[k]), hi_r[k]) : 0.0;
      u_r[k] = live ? u_r[k] + vh - sn : 0.0;
      ds_r[k] = sn - s_r[k];
      s_r[k] = sn;
      const double e = live ? v[k] - sn : 0.0;
      s_rp = __builtin_fma(e, e, s_rp);
      s_v = __builtin_fma(v[k], v[k], s_v);
      s_s = __builtin_fma(sn, sn, s_s);
    }
    double dl0, dl1, lu0, lu1, pe0, pe1;
    mul_At2(ds_r, u_r, dl0, dl1, lu0, lu1);
    {
      double e_r[SC_RPL];
#pragma unroll
      for (int k = 0; k < SC_RPL; ++k) e_r[k] = lane + 64 * k < m ? v[k] - s_r[k] : 0.0;
      mul_At2(e_r, e_r, pe0, pe1, pe0, pe1);
    }
    rp = sqrt(sm_sum(s_rp));
    rd = rho * sqrt(sm_sum(dl0 * dl0 + dl1 * dl1));
    const double rm = rho * sqrt(sm_sum(pe0 * pe0 + pe1 * pe1));  // how far A^T lambda still moves
    const double bn = sqrt(sm_sum(x0 * x0 + x1 * x1));
    const double ep = fmax(fmax(sqrt(sm_sum(s_v)), sqrt(sm_sum(s_s))), fmax(kap * bn, 1e-300));
    const double ed = fmax(fmax(rho * sqrt(sm_sum(lu0 * lu0 + lu1 * lu1)), cnorm), 1e-300);
    if (!(rp == rp) || !(rd == rd)) {
      st.bad = true;
      break;
    }
    if (rp <= a.tol * ep && rd <= a.tol * ed && rm <= a.tol * ed) {
      converged = true;
      break;
    }
    double factor;
    if (sb_rebalance(sweeps, rp, ep, fmax(rd, rm), ed, factor)) {
#pragma unroll
      for (int k = 0; k < SC_RPL; ++k) u_r[k] /= factor;  // (u is the multiplier divided by rho)
      add_K(rho * factor - rho);
      rho *= factor;
      L = sb_lambda_max(bs, matvec);
      st.products += 12;
    }
  }
  if (sweeps > a.max_sweeps) sweeps = a.max_sweeps;

  // record: coefficients, multipliers, loss with the matrix of the data alone
  add_K(-rho);
  double q0, q1;
  matvec(x0, x1, q0, q1);
  q0 -= c0;
  q1 -= c1;
  if (on0) a.beta_out[s0] = x0;
  if (on1) a.beta_out[s1] = x1;
#pragma unroll
  for (int k = 0; k < SC_RPL; ++k) {
    const int r = lane + 64 * k;
    if (r < m) {
      a.lambda_out[r] = rho * u_r[k];
      a.state[r] = s_r[k];
      a.state[SC_MMAX + r] = u_r[k];
    }
  }
  if (lane == 0) {
    a.state[2 * SC_MMAX] = rho;
    a.state[2 * SC_MMAX + 1] = st.bad ? 0.0 : 1.0;
    a.state[2 * SC_MMAX + 2] = (double)m;
    a.state[2 * SC_MMAX + 3] = (double)st.direct_hits;
    a.state[2 * SC_MMAX + 4] = (double)st.face_factors;
  }
  sb_record(bs, st, info, a.info, q0, q1, c0, c1, yy_s, sweeps, converged, rp, rd, rho);
  sb_release(bs);
}

}  // namespace slm
