// The b-step of the two on-chip splittings (small_split_kernels.hpp, small_constrained_kernels.hpp): a weighted Lasso
//
//     argmin_x  1/2 x^T H x - ce^T x + sum_j thr_j |x_j|
//
// on a matrix H whose base part lies in LDS (the Gram matrix of sm_build_gram, with whatever the kernel has added to it in
// place), warm-started from the sweep before.  Wavefront 0 iterates with every vector in registers -- lane l holds
// positions l and l + 64 -- and wavefronts 1..3 serve its matrix-vector products and its factorisations (sb_serve):
//   * sb_direct: where the face of the sweep before still holds, ONE direct solve on it;
//   * sb_inner:  otherwise accelerated proximal steps, conjugate gradients once the sign pattern stands still, plain
//                steps that confirm an accepted point -- the iteration and the stopping rule of small_solve_kernel
//                without its group norms.
// What differs between the two splittings comes in as a functor: the kernel's product y = H v (sb_matvec, plus its own
// terms), how a face of H is factored, what the cached factor is keyed by, and the bound on lambda_max(H).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "small_kernels.hpp"

namespace slm {

// Where things are: the matrix and the vectors in LDS, the workspace of the direct solves, the words that command the
// helper wavefronts, this lane's two positions, and the options of the inner iteration.
struct SbStep {
  const double* Gs;  // [p][p]
  double* vz;        // [p] operand of a product
  double* vu;        // [p] scratch of wavefront 0
  double* pp;        // [3][p] the partial products of wavefronts 1..3
  int* fidx;         // direct solves on a face (sm_face_factor): positions, ridge terms, diagonal, inverted pivots, factor
  double *fadd, *fdia, *invd, *Ff;
  int* cmd;          // command word of the helpers: 0 leave, 1 multiply, 2 factor a face of *fm unknowns
  int* fm;
  int p, mchunk, face_cap, lane;
  int s0, s1, sc0, sc1;  // (lanes beyond p read column 0; what they accumulate is never used)
  bool on0, on1, wide;
  double thr0, thr1;  // l1 weights of the lane's positions (set by wavefront 0)
  double tol_inner;
  int max_iters;
};

// `pp`: the stage of the build, free once the Gram matrix stands; the head of the direct solves lies behind the partial
// products, `fidx` at int `fidx_at` of it.
__device__ __forceinline__ SbStep sb_setup(const double* Gs, double* vz, double* vu, double* pp, int fidx_at, int p, int stage_doubles,
                                           int* cmd, int* fm, int lane, double tol_inner, int max_iters) {
  SbStep bs;
  bs.Gs = Gs; bs.vz = vz; bs.vu = vu; bs.pp = pp;
  bs.fidx = reinterpret_cast<int*>(pp + 3 * p) + fidx_at;
  bs.fadd = pp + 3 * p + SM_PMAX;
  bs.fdia = bs.fadd + SM_PMAX;
  bs.invd = bs.fdia + SM_PMAX;
  bs.Ff = bs.invd + SM_PMAX;
  bs.cmd = cmd; bs.fm = fm;
  bs.p = p;
  bs.mchunk = (((p + 3) >> 2) + 7) & ~7;
  bs.face_cap = sm_face_cap(stage_doubles - 3 * p - 64);
  bs.lane = lane;
  bs.s0 = lane; bs.s1 = lane + 64;
  bs.on0 = bs.s0 < p; bs.on1 = bs.s1 < p; bs.wide = p > 64;
  bs.sc0 = bs.on0 ? bs.s0 : 0; bs.sc1 = bs.on1 ? bs.s1 : 0;
  bs.thr0 = bs.thr1 = 0.0;
  bs.tol_inner = tol_inner;
  bs.max_iters = max_iters;
  return bs;
}

// What wavefront 0 carries from sweep to sweep, in its registers.
struct SbState {
  double x0, x1;           // the iterate
  long long products;      // matrix-vector products so far
  bool bad;                // a non-finite iterate
  uint64_t fm0, fm1;       // the face the factor in LDS belongs to, and the key it was made under
  double f_key;
  int direct_hits, face_factors;
};

__device__ __forceinline__ void sb_face_factor(const SbStep& bs, int m, bool worker, const int* fgrp = nullptr, double bd = 0.0) {
  sm_face_factor(bs.Gs, bs.p, bs.fidx, bs.fadd, m, bs.Ff, bs.fdia, bs.invd, worker, fgrp, bd);
}

// Wavefronts 1..3: wait at the barrier, multiply a quarter of the rows or factor a face when the command word says so
// (`factor(m, worker)`: the kernel's sm_face_factor), leave when it says zero.
template <class Factor>
__device__ __forceinline__ void sb_serve(const SbStep& bs, int wave, Factor factor) {
  const int p = bs.p;
  const int m_lo = wave * bs.mchunk < p ? wave * bs.mchunk : p, m_hi = (wave + 1) * bs.mchunk < p ? (wave + 1) * bs.mchunk : p;
  for (;;) {
    __syncthreads();
    const int cmd = *bs.cmd;
    if (cmd == 0) break;
    if (cmd == 2) {
      factor(*bs.fm, true);
      continue;
    }
    double y0, y1;
    sm_partial(bs.Gs, bs.vz, p, m_lo, m_hi, bs.sc0, bs.sc1, bs.wide, y0, y1);
    if (bs.on0) bs.pp[(wave - 1) * p + bs.s0] = y0;
    if (bs.on1) bs.pp[(wave - 1) * p + bs.s1] = y1;
    __syncthreads();
  }
}
__device__ __forceinline__ void sb_release(const SbStep& bs) {
  if (bs.lane == 0) *bs.cmd = 0;
  __syncthreads();
}

// y = G v with the matrix in LDS: v goes through LDS, the four wavefronts take a quarter of the rows each
__device__ __forceinline__ void sb_matvec(const SbStep& bs, double v0, double v1, double& y0, double& y1) {
  const int p = bs.p;
  if (bs.on0) bs.vz[bs.s0] = v0;
  if (bs.on1) bs.vz[bs.s1] = v1;
  if (bs.lane == 0) *bs.cmd = 1;
  __syncthreads();
  sm_partial(bs.Gs, bs.vz, p, 0, bs.mchunk < p ? bs.mchunk : p, bs.sc0, bs.sc1, bs.wide, y0, y1);
  __syncthreads();
  y0 += (bs.pp[bs.sc0] + bs.pp[p + bs.sc0]) + bs.pp[2 * p + bs.sc0];
  if (bs.wide) y1 += (bs.pp[bs.sc1] + bs.pp[p + bs.sc1]) + bs.pp[2 * p + bs.sc1];
}

// lambda_max of the matrix behind `matvec`: twelve power steps, 5 % on top
template <class Matvec>
__device__ __forceinline__ double sb_lambda_max(const SbStep& bs, Matvec matvec) {
  const bool on0 = bs.on0, on1 = bs.on1;
  double v0 = on0 ? 1.0 + 0.37 * (double)(((unsigned)(bs.s0 * 2654435761u) >> 24) & 0xffu) / 255.0 : 0.0;
  double v1 = on1 ? 1.0 + 0.37 * (double)(((unsigned)(bs.s1 * 2654435761u) >> 24) & 0xffu) / 255.0 : 0.0;
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
  const double L = lam * 1.05;
  return L > 0.0 ? L : 1.0;
}

// The b-step by iteration, from (st.x0, st.x1): linear term (ce0, ce1), `Lp` a bound on lambda_max (raised where the
// curvature measured along the steps says so).  Returns whether the point was confirmed; one that was not is short of
// its tolerance only, and the sweeps absorb that.
template <class Matvec>
__device__ __forceinline__ bool sb_inner(const SbStep& bs, SbState& st, Matvec matvec, double ce0, double ce1, double Lp) {
  const bool on0 = bs.on0, on1 = bs.on1;
  const double thr0 = bs.thr0, thr1 = bs.thr1;
  double& x0 = st.x0;
  double& x1 = st.x1;
  double z0 = x0, z1 = x1, tk = 1.0, qz0, qz1, zp0 = 0.0, zp1 = 0.0, qp0 = 0.0, qp1 = 0.0;
  bool have_prev = false;
  double mu_rq = 0.0, gnorm = 0.0;
  uint64_t pat_p = ~0ull, pat_n = ~0ull, pat_p1 = ~0ull, pat_n1 = ~0ull;
  int still = 0, it = 0, cg_runs = 0;
  const double tol = bs.tol_inner;
  auto prox = [&](double v0, double v1, double t, double& w0, double& w1) {
    w0 = on0 ? soft(v0, t * thr0) : 0.0;
    w1 = on1 ? soft(v1, t * thr1) : 0.0;
  };
  // plain steps that confirm an accepted point: the rate they contract at bounds the distance to the minimiser
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
  while (it < bs.max_iters && !conv) {
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
      st.bad = true;
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
    // conjugate gradients on the face: H_AA x_A = ce_A - thr_A sign(x_A), steps cut at the first sign change (that
    // coordinate leaves the face); the proximal steps that follow confirm the point or extend the face
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
      for (int k = 0; k < cg_cap && it < bs.max_iters && rr > 0.0; ++k) {
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
          st.bad = true;
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
      if (st.bad) break;
      z0 = x0; z1 = x1;
      tk = 1.0;
      have_prev = false;
      pat_p = pat_n = pat_p1 = pat_n1 = ~0ull;
    }
  }
  st.products += it;
  return conv;
}

// The b-step by ONE direct solve where the face of the sweep before still holds.  Between sweeps only the linear term
// moves; once the splitting has found the support, the b-step's minimiser keeps its face and its signs, and
// H_AA t_A = ce_A - thr_A s_A gives it exactly: L D L^T of the face (`factor(m, worker)`: the kernel's sm_face_factor; kept
// as long as the face and `key` -- whatever H changes with -- stand), two triangular solves, one product for the optimality
// conditions: the gradient on the face below what the iteration's stopping rule asks (with the smallest pivot for the
// curvature, `Lt` for lambda_max(H)), |q_j| <= thr_j off it, every sign kept.  Anything else returns false and leaves the
// sweep to sb_inner.
template <class Matvec, class Factor>
__device__ __forceinline__ bool sb_direct(const SbStep& bs, SbState& st, Matvec matvec, Factor factor, double key, double Lt,
                                          double ce0, double ce1) {
  const bool on0 = bs.on0, on1 = bs.on1;
  const int lane = bs.lane;
  const double thr0 = bs.thr0, thr1 = bs.thr1;
  double* vu = bs.vu;
  const double x0 = st.x0, x1 = st.x1;
  const bool f0 = on0 && x0 != 0.0, f1 = on1 && x1 != 0.0;
  const uint64_t m0 = __ballot(f0), m1 = __ballot(f1);
  const int n0 = __popcll(m0), m = n0 + __popcll(m1);
  if (m == 0 || m > bs.face_cap) return false;
  const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const int rk0 = __popcll(m0 & below), rk1 = n0 + __popcll(m1 & below);
  if (!(m0 == st.fm0 && m1 == st.fm1 && st.f_key == key)) {
    if (f0) { bs.fidx[rk0] = bs.s0; bs.fadd[rk0] = 0.0; }
    if (f1) { bs.fidx[rk1] = bs.s1; bs.fadd[rk1] = 0.0; }
    if (lane == 0) { *bs.fm = m; *bs.cmd = 2; }
    __syncthreads();
    factor(m, false);
    st.fm0 = m0; st.fm1 = m1; st.f_key = key;
    ++st.face_factors;
  }
  const int i0 = lane, i1 = lane + 64;
  const bool h0 = i0 < m, h1 = i1 < m;
  const double il0 = h0 ? bs.invd[i0] : 1.0, il1 = h1 ? bs.invd[i1] : 1.0;
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
    sm_face_solve(bs.Ff, bs.invd, m, lane, w0, w1);
    __builtin_amdgcn_wave_barrier();
    if (h0) vu[i0] = w0;
    if (h1) vu[i1] = w1;
    sm_lds_sync();
    t0 += f0 ? vu[rk0] : 0.0;
    t1 += f1 ? vu[rk1] : 0.0;
    if (__ballot((f0 && !(t0 * x0 > 0.0)) || (f1 && !(t1 * x1 > 0.0))) != 0ull) return false;  // a sign would change (or NaN)
    matvec(t0, t1, q0, q1);
    ++st.products;
    q0 = on0 ? q0 - ce0 : 0.0;
    q1 = on1 ? q1 - ce1 : 0.0;
    r0 = f0 ? -(q0 + copysign(thr0, x0)) : 0.0;
    r1 = f1 ? -(q1 + copysign(thr1, x1)) : 0.0;
    const double rn = sqrt(sm_sum(r0 * r0 + r1 * r1)), tn = sqrt(sm_sum(t0 * t0 + t1 * t1));
    const double gn = sqrt(sm_sum(q0 * q0 + q1 * q1));
    const double allow = fmax(0.1 * bs.tol_inner * tn * fmax(mu_est, kMuFloor * Lt), kRoundFloor * (gn + Lt * tn));
    const bool off0 = on0 && !f0 && fabs(q0) > thr0 + allow, off1 = on1 && !f1 && fabs(q1) > thr1 + allow;
    if (__ballot(off0 || off1) != 0ull) return false;  // a coordinate off the face wants in
    ok = rn <= allow;
  }
  if (!ok) return false;
  st.x0 = t0;
  st.x1 = t1;
  ++st.direct_hits;
  return true;
}

// Re-balancing of rho (the rule of model/_split.py): after sweeps 5, 10, 20, ..., 320, where the relative primal residual
// rp / ep and the relative dual one rd / ed are more than a factor 5 apart.  Returns whether rho moves, and by what; what
// goes with rho -- the scaled multiplier, the matrix -- is the kernel's.
__device__ __forceinline__ bool sb_rebalance(int sweeps, double rp, double ep, double rd, double ed, double& factor) {
  if (!(sweeps == 5 || sweeps == 10 || sweeps == 20 || sweeps == 40 || sweeps == 80 || sweeps == 160 || sweeps == 320)) return false;
  const double ratio = (rp / ep) / fmax(rd / ed, 1e-300);
  if (!(ratio > 5.0 || ratio < 0.2)) return false;
  factor = fmin(10.0, fmax(0.1, sqrt(ratio)));
  return true;
}

// The record of a call: n_iter = sweeps, rejects = matrix-vector products, kkt / mu = primal / dual residual, L = rho;
// the loss from (q0, q1) = G x - c with the matrix of the data alone.
__device__ __forceinline__ void sb_record(const SbStep& bs, const SbState& st, slm_point_info info, slm_point_info* out, double q0,
                                          double q1, double c0, double c1, double yy, int sweeps, bool converged, double rp,
                                          double rd, double rho) {
  const double x0 = st.x0, x1 = st.x1;
  const double loss = 0.5 * sm_sum((bs.on0 ? x0 * (q0 - c0) : 0.0) + (bs.on1 ? x1 * (q1 - c1) : 0.0)) + 0.5 * yy;
  const double bn = sqrt(sm_sum(x0 * x0 + x1 * x1));
  if (bs.lane == 0) {
    info.n_iter = sweeps;
    info.status = st.bad ? SLM_ERR_NON_FINITE : (converged ? SLM_OK : SLM_ERR_NOT_CONVERGED);
    info.resid = fmax(rp, rd);
    info.beta_norm = bn;
    info.loss = loss;
    info.L = rho;
    info.rejects = (int32_t)(st.products > 2000000000ll ? 2000000000ll : st.products);
    info.kkt = rp;
    info.mu = rd;
    out[0] = info;
  }
}

}  // namespace slm
