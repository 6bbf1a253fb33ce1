// SparseGroupLasso(standardize=True) on chip: the operator splitting of sparselm_amd/model/_split.py -- the reference's
// lambda1 ||b||_1 + lambda2 sum_g w_g ||X_g b_g||_2 (src/sparselm/model/_lasso.py:616-639 with the standardised group
// norms of :249-252) -- with ALL of its sweeps in one launch, for the problem sizes of small_kernels.hpp.
//
//     b      <- argmin 1/(2n)||X b - y||^2 + sum_j a_j |b_j| + rho/2 sum_g ||M_g b_g - gamma_g + u_g||^2
//     gamma  <- group soft-threshold of (M b + u) at b_g / rho
//     u      <- u + M b - gamma                                   (over-relaxed; M_g^T M_g = X_g^T X_g)
//
// On the host every sweep is an upload of new targets, an engine solve and a numpy step: 0.3 ms a sweep, 88 sweeps for
// a 100 x 80 fit.  Here the Gram matrix G = X^T X / n is built once in LDS; M_g is the (transposed) Cholesky factor of
// n G_gg -- any square root of X_g^T X_g gives the same norms; a pivot at rounding level drops its direction, as the
// host's SVD truncation does -- so the b-step is a weighted Lasso with matrix G + rho n blockdiag(G_gg) and linear term
// c + rho L (gamma - u): the b-step of small_bstep.hpp -- shared with small_constrained_kernels.hpp -- with the block-diagonal
// term added behind its matrix-vector product and inside its factorisations.  What is here is the splitting itself: the
// groups' factors, the gamma / u steps, the residuals and the stopping rule of _split.py, on registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "small_bstep.hpp"

namespace slm {

struct SplitSglArgs {
  const double* X;     // [n][ld]
  const double* y;
  const double* rw;    // row weights of the dataset (nullptr: ones)
  int64_t n, ld;
  int p, G, singleton;
  const int* order;    // group-sorted order, group of a feature, first position of a group
  const int* gid;
  const int* gstart;
  const double* a;     // [p] l1 weights
  const double* b;     // [G] group weights
  const double* beta0; // [p] warm start (nullptr: zero)
  double* beta_out;    // [p]
  double* gn_out;      // [G] ||X_g b_g||_2 (nullptr: not wanted)
  slm_point_info* info;  // [1]: n_iter = sweeps, rejects = matrix-vector products, resid = max(primal, dual residual)
  double* state;       // [2 ld + 4]: gamma, u (group-sorted order), rho, valid, direct b-steps, factorisations -- kept with the dataset
  int warm;            // continue from `state` (the re-weighting loop of the adaptive estimator)
  double tol, tol_inner, inv_n;
  int max_sweeps, max_iters, gmax, stage_doubles;
};

constexpr double SS_RELAX = 1.6;

static __global__ __launch_bounds__(SM_THREADS) void small_stdsgl_kernel(SplitSglArgs a) {
  extern __shared__ double sm_lds[];  // G [p][p], c [p], vz [p], vu [p], L [p][gmax], then the stage
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = a.p, G = a.G, gm = a.gmax;
  double* Gs = sm_lds;
  double* cs = Gs + p * p;
  double* vz = cs + p;
  double* vu = vz + p;
  double* Ll = vu + p;          // row r of a group's Cholesky factor L (L L^T = n G_gg) at position gs + r: [p][gm]
  double* stage = Ll + p * gm;  // the stage of the build; afterwards the partial products of wavefronts 1..3
  __shared__ double yy_s, sm_bd;
  __shared__ int sm_cmd, sm_m;
  const bool built = sm_build_gram(a.X, a.y, a.rw, a.n, a.ld, p, a.order, a.inv_n, a.stage_doubles, Gs, cs, stage, &yy_s);
  // (the stage of the build is free now; the group of every position lies in front of the head of the direct solves)
  SbStep bs = sb_setup(Gs, vz, vu, stage, SM_PMAX, p, a.stage_doubles, &sm_cmd, &sm_m, lane, a.tol_inner, a.max_iters);
  int* gpos = reinterpret_cast<int*>(stage + 3 * p);
  // a face of the b-step's matrix: entries inside a group count (1 + rho_n) times; rho_n reaches the helpers through sm_bd
  auto face_factor = [&](int mf, bool worker) { sb_face_factor(bs, mf, worker, gpos, sm_bd); };
  if (wave != 0) {
    sb_serve(bs, wave, face_factor);
    return;
  }
  const int s0 = bs.s0, s1 = bs.s1;
  const bool on0 = bs.on0, on1 = bs.on1;
  const int j0 = on0 ? a.order[s0] : 0, j1 = on1 ? a.order[s1] : 0;
  const int g0 = a.singleton ? j0 : a.gid[j0], g1 = a.singleton ? j1 : a.gid[j1];
  int gs0 = s0, gn0 = 1, gs1 = s1, gn1 = 1;
  if (!a.singleton) {
    if (on0) { gs0 = a.gstart[g0]; gn0 = a.gstart[g0 + 1] - gs0; }
    if (on1) { gs1 = a.gstart[g1]; gn1 = a.gstart[g1 + 1] - gs1; }
  }
  const int r0 = s0 - gs0, r1 = s1 - gs1;  // row of the position inside its group
  const double c0 = on0 ? cs[s0] : 0.0, c1 = on1 ? cs[s1] : 0.0;
  const double thr0 = on0 ? a.a[j0] : 0.0, thr1 = on1 ? a.a[j1] : 0.0;
  const double bg0 = on0 ? a.b[g0] : 0.0, bg1 = on1 ? a.b[g1] : 0.0;
  const double nrows = 1.0 / a.inv_n;
  double rho_n = 0.0;  // rho * n: the weight of blockdiag(G_gg) in the b-step's matrix

  bs.thr0 = thr0;
  bs.thr1 = thr1;

  // y = (G + rho_n blockdiag(G_gg)) v
  auto matvec = [&](double v0, double v1, double& y0, double& y1) {
    sb_matvec(bs, v0, v1, y0, y1);
    if (rho_n != 0.0) {
      if (on0) {
        double t = 0.0;
        for (int m = 0; m < gn0; ++m) t = __builtin_fma(Gs[(gs0 + m) * p + s0], vz[gs0 + m], t);
        y0 = __builtin_fma(rho_n, t, y0);
      }
      if (on1) {
        double t = 0.0;
        for (int m = 0; m < gn1; ++m) t = __builtin_fma(Gs[(gs1 + m) * p + s1], vz[gs1 + m], t);
        y1 = __builtin_fma(rho_n, t, y1);
      }
    }
  };
  // products with the groups' factors: (L^T v)_k = sum_{m >= k} L[m][k] v_m and (L w)_m = sum_{k <= m} L[m][k] w_k
  auto mul_Lt = [&](double v0, double v1, double& y0, double& y1) {  // M v
    if (on0) vu[s0] = v0;
    if (on1) vu[s1] = v1;
    sm_lds_sync();
    y0 = y1 = 0.0;
    if (on0)
      for (int m = r0; m < gn0; ++m) y0 = __builtin_fma(Ll[(gs0 + m) * gm + r0], vu[gs0 + m], y0);
    if (on1)
      for (int m = r1; m < gn1; ++m) y1 = __builtin_fma(Ll[(gs1 + m) * gm + r1], vu[gs1 + m], y1);
    __builtin_amdgcn_wave_barrier();
  };
  auto mul_L = [&](double w0, double w1, double& y0, double& y1) {  // M^T w
    if (on0) vu[s0] = w0;
    if (on1) vu[s1] = w1;
    sm_lds_sync();
    y0 = y1 = 0.0;
    if (on0)
      for (int k = 0; k <= r0; ++k) y0 = __builtin_fma(Ll[s0 * gm + k], vu[gs0 + k], y0);
    if (on1)
      for (int k = 0; k <= r1; ++k) y1 = __builtin_fma(Ll[s1 * gm + k], vu[gs1 + k], y1);
    __builtin_amdgcn_wave_barrier();
  };
  auto group_norm = [&](double v0, double v1, double& n0, double& n1) {  // norm of every position's group
    if (on0) vu[s0] = v0;
    if (on1) vu[s1] = v1;
    sm_lds_sync();
    n0 = n1 = 0.0;
    if (on0) {
      double ss = 0.0;
      for (int m = 0; m < gn0; ++m) ss = __builtin_fma(vu[gs0 + m], vu[gs0 + m], ss);
      n0 = sqrt(ss);
    }
    if (on1) {
      double ss = 0.0;
      for (int m = 0; m < gn1; ++m) ss = __builtin_fma(vu[gs1 + m], vu[gs1 + m], ss);
      n1 = sqrt(ss);
    }
    __builtin_amdgcn_wave_barrier();
  };

  if (a.gn_out != nullptr)
    for (int g = lane; g < G; g += 64) a.gn_out[g] = 0.0;  // (groups without columns)
  slm_point_info info;
  memset(&info, 0, sizeof(info));
  info.mode = 2;
  info.status = SLM_ERR_NOT_CONVERGED;
  if (!built) {
    if (lane == 0) a.info[0] = info;
    sb_release(bs);
    return;
  }

  // ---- the groups' Cholesky factors, all groups in step over the column index -------------------------------------
  for (int e = lane; e < p * gm; e += 64) Ll[e] = 0.0;
  sm_lds_sync();
  for (int j = 0; j < gm; ++j) {
    double va = 0.0, vb = 0.0;
    const bool act0 = on0 && j < gn0 && r0 >= j, act1 = on1 && j < gn1 && r1 >= j;
    if (act0) {
      va = nrows * Gs[s0 * p + gs0 + j];
      for (int k = 0; k < j; ++k) va = __builtin_fma(-Ll[s0 * gm + k], Ll[(gs0 + j) * gm + k], va);
    }
    if (act1) {
      vb = nrows * Gs[s1 * p + gs1 + j];
      for (int k = 0; k < j; ++k) vb = __builtin_fma(-Ll[s1 * gm + k], Ll[(gs1 + j) * gm + k], vb);
    }
    // (a pivot at rounding level: the column is linearly dependent on the ones before -- its direction is dropped)
    if (act0 && r0 == j) Ll[s0 * gm + j] = va > 1e-12 * nrows * Gs[s0 * p + s0] ? sqrt(va) : 0.0;
    if (act1 && r1 == j) Ll[s1 * gm + j] = vb > 1e-12 * nrows * Gs[s1 * p + s1] ? sqrt(vb) : 0.0;
    sm_lds_sync();
    if (act0 && r0 > j) {
      const double pv = Ll[(gs0 + j) * gm + j];
      Ll[s0 * gm + j] = pv > 0.0 ? va / pv : 0.0;
    }
    if (act1 && r1 > j) {
      const double pv = Ll[(gs1 + j) * gm + j];
      Ll[s1 * gm + j] = pv > 0.0 ? vb / pv : 0.0;
    }
    sm_lds_sync();
  }

  const double L = sb_lambda_max(bs, matvec);  // lambda_max(G): rho_n = 0 here

  // ---- state ------------------------------------------------------------------------------------------------------
  SbState st;
  memset(&st, 0, sizeof(st));
  st.f_key = -1.0;
  double& x0 = st.x0;
  double& x1 = st.x1;
  x0 = (on0 && a.beta0) ? a.beta0[j0] : 0.0;
  x1 = (on1 && a.beta0) ? a.beta0[j1] : 0.0;
  double gam0 = 0.0, gam1 = 0.0, u0 = 0.0, u1 = 0.0, rho = a.inv_n;
  const bool resume = a.warm && a.state != nullptr && a.state[2 * a.ld + 1] == 1.0;
  if (resume) {
    if (on0) { gam0 = a.state[s0]; u0 = a.state[a.ld + s0]; }
    if (on1) { gam1 = a.state[s1]; u1 = a.state[a.ld + s1]; }
    rho = a.state[2 * a.ld];
  } else if (a.beta0 != nullptr) {
    mul_Lt(x0, x1, gam0, gam1);
  }
  if (on0) gpos[s0] = g0;
  if (on1) gpos[s1] = g1;

  // ---- the sweeps --------------------------------------------------------------------------------------------------
  int sweeps = 0;
  bool converged = false;
  double rp = 0.0, rd = 0.0;
  for (sweeps = 1; sweeps <= a.max_sweeps && !st.bad; ++sweeps) {
    rho_n = rho * nrows;
    if (lane == 0) sm_bd = rho_n;  // (read by the helpers behind the barrier of a factorisation)
    const double Lt = L * (1.0 + rho_n);
    double t0, t1;
    mul_L(gam0 - u0, gam1 - u1, t0, t1);
    const double ce0 = __builtin_fma(rho, t0, c0), ce1 = __builtin_fma(rho, t1, c1);
    if (!sb_direct(bs, st, matvec, face_factor, rho_n, Lt, ce0, ce1)) (void)sb_inner(bs, st, matvec, ce0, ce1, Lt);
    if (st.bad) break;
    double v0, v1;
    mul_Lt(x0, x1, v0, v1);
    const double vh0 = SS_RELAX * v0 + (1.0 - SS_RELAX) * gam0, vh1 = SS_RELAX * v1 + (1.0 - SS_RELAX) * gam1;
    double nr0, nr1;
    group_norm(vh0 + u0, vh1 + u1, nr0, nr1);
    const double sh0 = on0 ? (nr0 * rho > bg0 ? 1.0 - bg0 / (rho * nr0) : 0.0) : 0.0;
    const double sh1 = on1 ? (nr1 * rho > bg1 ? 1.0 - bg1 / (rho * nr1) : 0.0) : 0.0;
    const double gn0v = (vh0 + u0) * sh0, gn1v = (vh1 + u1) * sh1;
    u0 += vh0 - gn0v;
    u1 += vh1 - gn1v;
    double dl0, dl1, lu0, lu1;
    mul_L(gn0v - gam0, gn1v - gam1, dl0, dl1);
    mul_L(u0, u1, lu0, lu1);
    rp = sqrt(sm_sum((v0 - gn0v) * (v0 - gn0v) + (v1 - gn1v) * (v1 - gn1v)));
    rd = rho * sqrt(sm_sum(dl0 * dl0 + dl1 * dl1));
    gam0 = gn0v;
    gam1 = gn1v;
    const double ep = fmax(fmax(sqrt(sm_sum(v0 * v0 + v1 * v1)), sqrt(sm_sum(gam0 * gam0 + gam1 * gam1))), 1e-300);
    const double ed = fmax(rho * sqrt(sm_sum(lu0 * lu0 + lu1 * lu1)), 1e-300);
    if (!(rp == rp) || !(rd == rd)) {
      st.bad = true;
      break;
    }
    if (rp <= a.tol * ep && rd <= a.tol * ed) {
      converged = true;
      break;
    }
    double factor;
    if (sb_rebalance(sweeps, rp, ep, rd, ed, factor)) {
      u0 /= factor;  // (u is the multiplier divided by rho)
      u1 /= factor;
      rho *= factor;
    }
  }
  if (sweeps > a.max_sweeps) sweeps = a.max_sweeps;

  // gamma is exactly group-sparse, M b only to the residual: a group whose gamma_g vanished is out
  {
    double ng0, ng1;
    group_norm(gam0, gam1, ng0, ng1);
    if (ng0 == 0.0) x0 = 0.0;
    if (ng1 == 0.0) x1 = 0.0;
  }
  // record: coefficients, ||X_g b_g||, loss with the matrix of the data alone
  rho_n = 0.0;
  double q0, q1, v0, v1, nv0, nv1;
  matvec(x0, x1, q0, q1);
  q0 -= c0;
  q1 -= c1;
  mul_Lt(x0, x1, v0, v1);
  group_norm(v0, v1, nv0, nv1);
  if (on0) a.beta_out[j0] = x0;
  if (on1) a.beta_out[j1] = x1;
  if (a.gn_out != nullptr) {
    if (on0 && r0 == 0) a.gn_out[g0] = nv0;
    if (on1 && r1 == 0) a.gn_out[g1] = nv1;
  }
  if (a.state != nullptr) {
    if (on0) { a.state[s0] = gam0; a.state[a.ld + s0] = u0; }
    if (on1) { a.state[s1] = gam1; a.state[a.ld + s1] = u1; }
    if (lane == 0) {
      a.state[2 * a.ld] = rho;
      a.state[2 * a.ld + 1] = st.bad ? 0.0 : 1.0;
      a.state[2 * a.ld + 2] = (double)st.direct_hits;
      a.state[2 * a.ld + 3] = (double)st.face_factors;
    }
  }
  sb_record(bs, st, info, a.info, q0, q1, c0, c1, yy_s, sweeps, converged, rp, rd, rho);
  sb_release(bs);
}

}  // namespace slm
