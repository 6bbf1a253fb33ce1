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
// The b-step is then a weighted Lasso with linear term c + rho A^T (s - u): the matrix-vector product of small_kernels.hpp,
// the accelerated proximal steps + conjugate gradients on the face, and one direct solve where the face of the sweep
// before still holds -- the b-step of small_split_kernels.hpp without the group terms.  s, u, lo and hi live in registers:
// lane l holds rows l, l + 64, ... (m <= 512: eight per lane).  The residuals, the re-balancing of rho and the stopping
// rule are those of _constrained.py.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "small_kernels.hpp"

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
  double* pp = stage;
  int* fidx = reinterpret_cast<int*>(pp + 3 * p);
  double* fadd = pp + 3 * p + SM_PMAX;
  double* fdia = fadd + SM_PMAX;
  double* invd = fdia + SM_PMAX;
  double* Ff = invd + SM_PMAX;
  const int face_cap = sm_face_cap(a.stage_doubles - 3 * p - 64);
  const int mchunk = (((p + 3) >> 2) + 7) & ~7;
  if (wave != 0) {
    const int s0w = lane, s1w = lane + 64;
    const bool on0w = s0w < p, on1w = s1w < p;
    const int m_lo = wave * mchunk < p ? wave * mchunk : p, m_hi = (wave + 1) * mchunk < p ? (wave + 1) * mchunk : p;
    for (;;) {
      __syncthreads();
      const int cmd = sm_cmd;
      if (cmd == 0) break;
      if (cmd == 2) {
        sm_face_factor(Gs, p, fidx, fadd, sm_m, Ff, fdia, invd, true);
        continue;
      }
      double y0, y1;
      sm_partial(Gs, vz, p, m_lo, m_hi, on0w ? s0w : 0, on1w ? s1w : 0, p > 64, y0, y1);
      if (on0w) pp[(wave - 1) * p + s0w] = y0;
      if (on1w) pp[(wave - 1) * p + s1w] = y1;
      __syncthreads();
    }
    return;
  }
  const int s0 = lane, s1 = lane + 64;
  const bool on0 = s0 < p, on1 = s1 < p, wide = p > 64;
  const int sc0 = on0 ? s0 : 0, sc1 = on1 ? s1 : 0;
  const double c0 = on0 ? cs[s0] : 0.0, c1 = on1 ? cs[s1] : 0.0;
  const double thr0 = on0 ? a.a[s0] : 0.0, thr1 = on1 ? a.a[s1] : 0.0;

  // y = (G + rho K) v, the matrix in LDS
  auto matvec = [&](double v0, double v1, double& y0, double& y1) {
    if (on0) vz[s0] = v0;
    if (on1) vz[s1] = v1;
    if (lane == 0) sm_cmd = 1;
    __syncthreads();
    sm_partial(Gs, vz, p, 0, mchunk < p ? mchunk : p, sc0, sc1, wide, y0, y1);
    __syncthreads();
    y0 += (pp[sc0] + pp[p + sc0]) + pp[2 * p + sc0];
    if (wide) y1 += (pp[sc1] + pp[p + sc1]) + pp[2 * p + sc1];
  };
  auto release_helpers = [&]() {
    if (lane == 0) sm_cmd = 0;
    __syncthreads();
  };
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
  auto lambda_max = [&]() {  // twelve power steps on the matrix in LDS
    double v0 = on0 ? 1.0 + 0.37 * (double)(((unsigned)(s0 * 2654435761u) >> 24) & 0xffu) / 255.0 : 0.0;
    double v1 = on1 ? 1.0 + 0.37 * (double)(((unsigned)(s1 * 2654435761u) >> 24) & 0xffu) / 255.0 : 0.0;
    double lam = 0.0;
    for (int it = 0; it < 12; ++it) {
      double y0, y1;
      matvec(v0, v1, y0, y1);
      if (!on0) y0 = 0.0;
      if (!on1) y1 = 0.0;
      lam = sqrt(sm_sum(y0 * y0 + y1 * y1));
      const double inv = lam > 0.0 ? 1.0 / lam : 0.0;
      v0 = y0 * inv;
      v1 = y1 * inv;
    }
    const double Lr = lam * 1.05;
    return Lr > 0.0 ? Lr : 1.0;
  };

  slm_point_info info;
  memset(&info, 0, sizeof(info));
  info.mode = 3;
  info.status = SLM_ERR_NOT_CONVERGED;
  if (!built) {
    if (lane == 0) a.info[0] = info;
    release_helpers();
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
  double x0 = (on0 && a.beta0) ? a.beta0[s0] : 0.0, x1 = (on1 && a.beta0) ? a.beta0[s1] : 0.0;
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
  double L = lambda_max();
  long long products = 12;
  bool bad = false;

  // the b-step: weighted Lasso with matrix G + rho K and linear term (ce0, ce1), from (x0, x1)
  auto inner = [&](double ce0, double ce1, double Lp) {
    double z0 = x0, z1 = x1, tk = 1.0, qz0, qz1, zp0 = 0.0, zp1 = 0.0, qp0 = 0.0, qp1 = 0.0;
    bool have_prev = false;
    double mu_rq = 0.0, gnorm = 0.0;
    uint64_t pat_p = ~0ull, pat_n = ~0ull, pat_p1 = ~0ull, pat_n1 = ~0ull;
    int still = 0, it = 0, cg_runs = 0;
    const double tol = a.tol_inner;
    auto prox = [&](double v0, double v1, double t, double& w0, double& w1) {
      w0 = on0 ? soft(v0, t * thr0) : 0.0;
      w1 = on1 ? soft(v1, t * thr1) : 0.0;
    };
    // (plain steps that confirm an accepted point: see small_solve_kernel)
    auto confirm = [&](double v0, double v1, double rn_start, double t) {
      double rn_prev = rn_start, rhoc = 0.0, rn = rn_start, bn = 0.0;
      for (int v = 0; v < 4 && rn > 0.0; ++v) {
        double qv0, qv1, h0, h1;
        matvec(v0, v1, qv0, qv1);
        ++it;
        qv0 = on0 ? qv0 - ce0 : 0.0;
        qv1 = on1 ? qv1 - ce1 : 0.0;
        prox(v0 - t * qv0, v1 - t * qv1, t, h0, h1);
        const double e0 = h0 - v0, e1 = h1 - v1;
        rn = sqrt(sm_sum(e0 * e0 + e1 * e1));
        bn = sqrt(sm_sum(h0 * h0 + h1 * h1));
        if (v > 0) rhoc = fmax(rhoc, rn_prev > 0.0 ? rn / rn_prev : 0.0);
        rn_prev = rn;
        v0 = h0;
        v1 = h1;
      }
      x0 = v0;
      x1 = v1;
      const double err = rhoc < 1.0 ? rhoc / (1.0 - rhoc) * rn : 1e300;
      if (err <= tol * bn || rn * Lp <= kRoundFloor * (gnorm + Lp * bn)) return true;
      if (rhoc > 0.0 && rhoc < 1.0) mu_rq = mu_rq > 0.0 ? fmin(mu_rq, Lp * (1.0 - rhoc)) : Lp * (1.0 - rhoc);
      return false;
    };
    bool conv = false;
    while (it < a.max_iters && !conv) {
      matvec(z0, z1, qz0, qz1);
      ++it;
      qz0 = on0 ? qz0 - ce0 : 0.0;
      qz1 = on1 ? qz1 - ce1 : 0.0;
      if (have_prev) {
        const double dz0 = z0 - zp0, dz1 = z1 - zp1;
        const double dd = sm_sum(dz0 * dz0 + dz1 * dz1);
        if (dd > 0.0) {
          const double rq = sm_sum(dz0 * (qz0 - qp0) + dz1 * (qz1 - qp1)) / dd;
          if (rq > Lp) Lp = 1.05 * rq;
          if (rq > 0.0) mu_rq = mu_rq > 0.0 ? fmin(mu_rq, rq) : rq;
        }
      }
      const double t = 1.0 / Lp;
      double w0, w1;
      prox(z0 - t * qz0, z1 - t * qz1, t, w0, w1);
      const double e0 = z0 - w0, e1 = z1 - w1;
      const double s_kkt = sm_sum(e0 * e0 + e1 * e1), s_b = sm_sum(w0 * w0 + w1 * w1);
      if ((it & 7) == 1) gnorm = sqrt(sm_sum(qz0 * qz0 + qz1 * qz1));
      const double s_rs = sm_sum(e0 * (w0 - x0) + e1 * (w1 - x1));
      if (!(s_kkt == s_kkt) || !(s_b < 1e300)) {
        bad = true;
        break;
      }
      const double kkt = sqrt(s_kkt) * Lp, bnorm = sqrt(s_b);
      double mu_eff = mu_rq > 0.0 ? fmin(mu_rq, Lp) : Lp;
      mu_eff = fmax(mu_eff, kMuFloor * Lp);
      if (kkt <= fmax(tol * bnorm * mu_eff, kRoundFloor * (gnorm + Lp * bnorm))) {
        if (confirm(w0, w1, sqrt(s_kkt), t)) {
          conv = true;
          break;
        }
        z0 = x0; z1 = x1;
        tk = 1.0;
        have_prev = false;
        still = 0;
        pat_p = pat_n = pat_p1 = pat_n1 = ~0ull;
        continue;
      }
      const bool restart = s_rs > 0.0;
      const double tk_new = restart ? 1.0 : 0.5 * (1.0 + sqrt(1.0 + 4.0 * tk * tk));
      const double mom = restart ? 0.0 : (tk - 1.0) / tk_new;
      zp0 = z0; zp1 = z1; qp0 = qz0; qp1 = qz1;
      have_prev = true;
      z0 = w0 + mom * (w0 - x0);
      z1 = w1 + mom * (w1 - x1);
      x0 = w0;
      x1 = w1;
      tk = tk_new;
      const uint64_t np0 = __ballot(on0 && x0 > 0.0), nn0 = __ballot(on0 && x0 < 0.0);
      const uint64_t np1 = __ballot(on1 && x1 > 0.0), nn1 = __ballot(on1 && x1 < 0.0);
      still = (np0 == pat_p && nn0 == pat_n && np1 == pat_p1 && nn1 == pat_n1) ? still + 1 : 0;
      pat_p = np0; pat_n = nn0; pat_p1 = np1; pat_n1 = nn1;
      // conjugate gradients on the face (see small_solve_kernel)
      if (still >= SM_STILL && cg_runs < 6 && (np0 | nn0 | np1 | nn1) != 0ull) {
        ++cg_runs;
        still = 0;
        bool f0 = on0 && x0 != 0.0, f1 = on1 && x1 != 0.0;
        double q0, q1;
        matvec(x0, x1, q0, q1);
        ++it;
        q0 -= ce0;
        q1 -= ce1;
        int hits = 0;
        const int face0 = __popcll(np0 | nn0) + __popcll(np1 | nn1);
        const int cg_cap = 2 * face0 + 10;
        double rr0 = f0 ? -(q0 + copysign(thr0, x0)) : 0.0, rr1 = f1 ? -(q1 + copysign(thr1, x1)) : 0.0;
        double d0v = rr0, d1v = rr1;
        double rr = sm_sum(rr0 * rr0 + rr1 * rr1);
        const double rr_start = rr;
        for (int k = 0; k < cg_cap && it < a.max_iters && rr > 0.0; ++k) {
          double h0, h1;
          matvec(d0v, d1v, h0, h1);
          ++it;
          h0 = f0 ? h0 : 0.0;
          h1 = f1 ? h1 : 0.0;
          const double dHd = sm_sum(d0v * h0 + d1v * h1), dd = sm_sum(d0v * d0v + d1v * d1v);
          if (!(dd > 0.0)) break;
          if (dHd > 0.0) mu_rq = mu_rq > 0.0 ? fmin(mu_rq, dHd / dd) : dHd / dd;
          double alpha = dHd > 1e-14 * Lp * dd ? rr / dHd : 1e300;
          const double lim0 = (f0 && d0v * x0 < 0.0) ? -x0 / d0v : 1e300;
          const double lim1 = (f1 && d1v * x1 < 0.0) ? -x1 / d1v : 1e300;
          const double amax = sm_min(fmin(lim0, lim1));
          const bool hit = alpha >= amax;
          if (hit) alpha = amax;
          if (!(alpha < 1e299)) break;
          x0 = f0 ? __builtin_fma(alpha, d0v, x0) : x0;
          x1 = f1 ? __builtin_fma(alpha, d1v, x1) : x1;
          if (hit) {
            if (f0 && lim0 <= amax) { x0 = 0.0; f0 = false; }
            if (f1 && lim1 <= amax) { x1 = 0.0; f1 = false; }
            matvec(x0, x1, q0, q1);
            ++it;
            q0 -= ce0;
            q1 -= ce1;
            rr0 = f0 ? -(q0 + copysign(thr0, x0)) : 0.0;
            rr1 = f1 ? -(q1 + copysign(thr1, x1)) : 0.0;
            d0v = rr0;
            d1v = rr1;
            rr = sm_sum(rr0 * rr0 + rr1 * rr1);
            if (++hits > face0) break;
            continue;
          }
          rr0 = f0 ? __builtin_fma(-alpha, h0, rr0) : 0.0;
          rr1 = f1 ? __builtin_fma(-alpha, h1, rr1) : 0.0;
          const double rr_new = sm_sum(rr0 * rr0 + rr1 * rr1);
          if (!(rr_new == rr_new)) {
            bad = true;
            break;
          }
          const double xn = sqrt(sm_sum(x0 * x0 + x1 * x1));
          double mu2 = mu_rq > 0.0 ? fmin(mu_rq, Lp) : Lp;
          mu2 = fmax(mu2, kMuFloor * Lp);
          if (sqrt(rr_new) <= 0.1 * fmax(tol * xn * mu2, kRoundFloor * (gnorm + Lp * xn)) || rr_new <= 1e-30 * rr_start) break;
          const double bt = rr_new / rr;
          d0v = __builtin_fma(bt, d0v, rr0);
          d1v = __builtin_fma(bt, d1v, rr1);
          rr = rr_new;
        }
        if (bad) break;
        z0 = x0; z1 = x1;
        tk = 1.0;
        have_prev = false;
        pat_p = pat_n = pat_p1 = pat_n1 = ~0ull;
      }
    }
    products += it;
    return conv;
  };

  // ---- the b-step by ONE direct solve where the face of the sweep before still holds (as in small_split_kernels.hpp)
  uint64_t fm0 = 0ull, fm1 = 0ull;  // the face the factor in LDS belongs to
  double f_rho = -1.0;
  int direct_hits = 0, face_factors = 0;
  auto direct_b = [&](double ce0, double ce1) {
    const bool f0 = on0 && x0 != 0.0, f1 = on1 && x1 != 0.0;
    const uint64_t m0 = __ballot(f0), m1 = __ballot(f1);
    const int n0 = __popcll(m0), mf = n0 + __popcll(m1);
    if (mf == 0 || mf > face_cap) return false;
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const int rk0 = __popcll(m0 & below), rk1 = n0 + __popcll(m1 & below);
    if (!(m0 == fm0 && m1 == fm1 && f_rho == rho)) {
      if (f0) { fidx[rk0] = s0; fadd[rk0] = 0.0; }
      if (f1) { fidx[rk1] = s1; fadd[rk1] = 0.0; }
      if (lane == 0) { sm_m = mf; sm_cmd = 2; }
      __syncthreads();
      sm_face_factor(Gs, p, fidx, fadd, mf, Ff, fdia, invd, false);
      fm0 = m0; fm1 = m1; f_rho = rho;
      ++face_factors;
    }
    const int i0 = lane, i1 = lane + 64;
    const bool h0 = i0 < mf, h1 = i1 < mf;
    const double il0 = h0 ? invd[i0] : 1.0, il1 = h1 ? invd[i1] : 1.0;
    if (__ballot((h0 && il0 == 0.0) || (h1 && il1 == 0.0)) != 0ull) return false;  // (a dropped pivot: a singular face)
    const double mu_est = 1.0 / sm_max(fmax(h0 ? il0 : 0.0, h1 ? il1 : 0.0));      // the smallest pivot
    double t0 = 0.0, t1 = 0.0, q0 = 0.0, q1 = 0.0;
    double r0 = f0 ? ce0 - copysign(thr0, x0) : 0.0, r1 = f1 ? ce1 - copysign(thr1, x1) : 0.0;  // right-hand side, then residual
    bool ok = false;
    for (int pass = 0; pass < 2 && !ok; ++pass) {  // (the second pass: one step of iterative refinement)
      __builtin_amdgcn_wave_barrier();
      if (f0) vu[rk0] = r0;
      if (f1) vu[rk1] = r1;
      sm_lds_sync();
      double w0 = h0 ? vu[i0] : 0.0, w1 = h1 ? vu[i1] : 0.0;
      sm_face_solve(Ff, invd, mf, lane, w0, w1);
      __builtin_amdgcn_wave_barrier();
      if (h0) vu[i0] = w0;
      if (h1) vu[i1] = w1;
      sm_lds_sync();
      t0 += f0 ? vu[rk0] : 0.0;
      t1 += f1 ? vu[rk1] : 0.0;
      if (__ballot((f0 && !(t0 * x0 > 0.0)) || (f1 && !(t1 * x1 > 0.0))) != 0ull) return false;  // a sign would change (or NaN)
      matvec(t0, t1, q0, q1);
      ++products;
      q0 = on0 ? q0 - ce0 : 0.0;
      q1 = on1 ? q1 - ce1 : 0.0;
      r0 = f0 ? -(q0 + copysign(thr0, x0)) : 0.0;
      r1 = f1 ? -(q1 + copysign(thr1, x1)) : 0.0;
      const double rn = sqrt(sm_sum(r0 * r0 + r1 * r1)), tn = sqrt(sm_sum(t0 * t0 + t1 * t1));
      const double gn = sqrt(sm_sum(q0 * q0 + q1 * q1));
      const double allow = fmax(0.1 * a.tol_inner * tn * fmax(mu_est, kMuFloor * L), kRoundFloor * (gn + L * tn));
      const bool off0 = on0 && !f0 && fabs(q0) > thr0 + allow, off1 = on1 && !f1 && fabs(q1) > thr1 + allow;
      if (__ballot(off0 || off1) != 0ull) return false;  // a coordinate off the face wants in
      ok = rn <= allow;
    }
    if (!ok) return false;
    x0 = t0;
    x1 = t1;
    ++direct_hits;
    return true;
  };

  // ---- the sweeps --------------------------------------------------------------------------------------------------
  int sweeps = 0;
  bool converged = false;
  double rp = 0.0, rd = 0.0;
  for (sweeps = 1; sweeps <= a.max_sweeps && !bad; ++sweeps) {
    double w[SC_RPL], zz[SC_RPL];
#pragma unroll
    for (int k = 0; k < SC_RPL; ++k) {
      w[k] = s_r[k] - u_r[k];
      zz[k] = 0.0;
    }
    double t0, t1, dum0, dum1;
    mul_At2(w, zz, t0, t1, dum0, dum1);
    const double ce0 = __builtin_fma(rho, t0, c0), ce1 = __builtin_fma(rho, t1, c1);
    if (!direct_b(ce0, ce1)) (void)inner(ce0, ce1, L);  // (short of its tolerance: absorbed by the sweeps)
    if (bad) break;
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
      bad = true;
      break;
    }
    if (rp <= a.tol * ep && rd <= a.tol * ed && rm <= a.tol * ed) {
      converged = true;
      break;
    }
    if (sweeps == 5 || sweeps == 10 || sweeps == 20 || sweeps == 40 || sweeps == 80 || sweeps == 160 || sweeps == 320) {
      const double ratio = (rp / ep) / fmax(fmax(rd, rm) / ed, 1e-300);
      if (ratio > 5.0 || ratio < 0.2) {
        const double factor = fmin(10.0, fmax(0.1, sqrt(ratio)));
#pragma unroll
        for (int k = 0; k < SC_RPL; ++k) u_r[k] /= factor;  // (u is the multiplier divided by rho)
        add_K(rho * factor - rho);
        rho *= factor;
        L = lambda_max();
        products += 12;
      }
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
    a.state[2 * SC_MMAX + 1] = bad ? 0.0 : 1.0;
    a.state[2 * SC_MMAX + 2] = (double)m;
    a.state[2 * SC_MMAX + 3] = (double)direct_hits;
    a.state[2 * SC_MMAX + 4] = (double)face_factors;
  }
  const double loss = 0.5 * sm_sum((on0 ? x0 * (q0 - c0) : 0.0) + (on1 ? x1 * (q1 - c1) : 0.0)) + 0.5 * yy_s;
  const double bn = sqrt(sm_sum(x0 * x0 + x1 * x1));
  if (lane == 0) {
    info.n_iter = sweeps;
    info.status = bad ? SLM_ERR_NON_FINITE : (converged ? SLM_OK : SLM_ERR_NOT_CONVERGED);
    info.resid = fmax(rp, rd);
    info.beta_norm = bn;
    info.loss = loss;
    info.L = rho;
    info.rejects = (int32_t)(products > 2000000000ll ? 2000000000ll : products);
    info.kkt = rp;
    info.mu = rd;
    a.info[0] = info;
  }
  release_helpers();
}

}  // namespace slm
