// The scalar state machine of one tail-kernel call (tail_kernels.hpp): what a lane decides from the workgroup sums of an
// iteration -- the spectral scheme's acceptance test and step, the FISTA curvature guard and restart, the stopping rule,
// the walk over the path points -- and nothing per feature.  Like host_logic.hpp it is free of HIP types so that g++
// compiles it alone: tests/host_logic_test.cpp runs every function on the CPU under the sanitizers, and
// fista_tail_kernel / fista_tail_stream_kernel call THESE functions -- what is tested is what runs.  The schemes and the
// stopping rule are described at fista_tail_kernel.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/slm_engine.h"

#ifndef SLM_HD
#if defined(__HIPCC__)
#define SLM_HD __host__ __device__
#else
#define SLM_HD
#endif
#endif
// (a call that is not inlined passes the snapshot and the outcome through memory: scratch, on the device)
#define SLM_INLINE inline __attribute__((always_inline))
// (the loops over the ring are unrolled on the device so that hist[] stays in registers; g++ does not know the pragma)
#if defined(__HIPCC__)
#define SLM_UNROLL _Pragma("unroll")
#else
#define SLM_UNROLL
#endif

namespace slm {

constexpr int BB_HIST = 5;
constexpr int BB_REJECT_LIMIT = 3;    // rejected candidates before a lane falls back to FISTA
constexpr int BB_POINT_LIMIT = 60;    // spectral iterations on one point before falling back
constexpr double BB_SIGMA = 1e-4;
// Strong-convexity estimates below kMuFloor * lambda_max are not trusted: p > n problems, duplicated
// columns -- the objective is then flat along some direction of the face (mu = 0: the minimiser is not
// unique and no residual bounds the distance to "it"); the rule then bounds the residual itself.
constexpr double kMuFloor = 1e-6;

// What a call reads of its lane's PathCtl (the fields keep PathCtl's names and meaning), and the scalars of the call itself.
struct TailSnap {
  int32_t point, n_points, pt_lo, stride, tail_pt;
  int32_t iter, max_iter;
  int64_t total_iter;
  uint32_t flags;
  int32_t mode, have_base, rejects, n_hist;
  double t, L, tol, ak, Lhat, pen_z, mu, mu_rq, loss_base;
  double hist[BB_HIST];
  double loss_z;       // smooth loss at z (this call's gradient evaluation)
  bool hit_max;        // this is the last iteration the point may take
  bool cold;           // SLM_FLAG_COLD_START
  bool provisional;    // the gradient is an estimate: no point is accepted on it (TailArgs::provisional)
  double bnorm_floor;  // see tail_snap_call
  double round_floor;  // kRoundFloor of tail_kernels.hpp (the working-set and on-chip solvers stop by it too)
};

// The per-call scalars of a snapshot whose PathCtl fields are set.
SLM_HD SLM_INLINE void tail_snap_call(TailSnap& c, double loss_z, bool provisional, double round_floor) {
  c.round_floor = round_floor;
  c.loss_z = loss_z;
  c.provisional = provisional;
  c.cold = (c.flags & SLM_FLAG_COLD_START) != 0;
  c.hit_max = (c.iter + 1 >= c.max_iter);
  // ||beta|| in the stopping rule never drops below 1e-10 of the scale the data give a coefficient
  // vector (rms residual / sqrt(L)): at alpha ~ alpha_max the minimiser is a rounding-level number
  // (~1e-16) and "tol relative to it" would ask for more digits than fp64 has.
  c.bnorm_floor = 1e-10 * sqrt(2.0 * fmax(loss_z, 0.0) / fmax(c.L, c.Lhat));
}

// The outcome of a call: the control block's next values and what the point's record reports.
struct TailNext {
  int32_t mode, have_base, rejects, n_hist;
  double t, L, ak, Lhat, pen_z, mu_rq, loss_base;
  double hist[BB_HIST];
  bool finalize, conv, nonfinite;
  bool did_restart, l_bad;
  bool fallback;  // the spectral scheme hands the lane to FISTA in this call
  bool stored;    // gprev now holds this call's gradient (all but a rejected candidate)
  double resid, bnorm, kkt, mu_eff;
  double mom;     // FISTA: momentum of the next extrapolated point
};

SLM_HD SLM_INLINE TailNext tail_next(const TailSnap& c) {
  TailNext n;
  n.mode = c.mode; n.have_base = c.have_base; n.rejects = c.rejects; n.n_hist = c.n_hist;
  n.t = c.t; n.L = c.L; n.ak = c.ak; n.Lhat = c.Lhat; n.pen_z = c.pen_z; n.mu_rq = c.mu_rq; n.loss_base = c.loss_base;
  SLM_UNROLL
  for (int k = 0; k < BB_HIST; ++k) n.hist[k] = c.hist[k];
  n.finalize = n.conv = n.nonfinite = n.did_restart = n.l_bad = n.fallback = false;
  n.stored = true;
  n.resid = n.bnorm = n.kkt = n.mu_eff = n.mom = 0.0;
  return n;
}

// ================= spectral (BB) scheme =========================================================
//  s[0] = ||z - beta||^2   s[1] = <z - beta, g - gbase>   s[2] = ||g - gbase||^2   s[3] = #non-finite g
//  s[4] = penalty value at z (only computed at the start of a path point, when no candidate
//         carried it over)
//  s[5] = ||g||^2 (rounding floor of the stopping rule)
// Accept or reject the candidate z: the inverse step ak, the curvature bounds, the ring of the last BB_HIST accepted
// objective values, and whether the lane now falls back to FISTA (n.fallback).  Returns `accept`.
SLM_HD SLM_INLINE bool bb_decide(const TailSnap& c, TailNext& n, const double (&s)[6]) {
  const double Fz = c.loss_z + (c.have_base ? c.pen_z : s[4]);
  n.nonfinite = s[3] > 0.0 || !isfinite(Fz);
  bool accept;
  if (!c.have_base) {
    accept = true;  // z is the start point of this path point: it becomes the base
    n.n_hist = 0;
  } else {
    double fmax_hist = c.hist[0];
    SLM_UNROLL
    for (int k = 1; k < BB_HIST; ++k)
      if (k < c.n_hist) fmax_hist = fmax(fmax_hist, c.hist[k]);
    accept = Fz <= fmax_hist - 0.5 * BB_SIGMA * c.ak * s[0];
    if (accept) {
      if (s[0] > 0.0) {
        n.Lhat = fmax(c.Lhat, sqrt(s[2] / s[0]));
        n.ak = s[1] > 0.0 ? s[1] / s[0] : n.Lhat;
      }
      n.ak = fmin(fmax(n.ak, 1e-6 * n.Lhat), 1e6 * n.Lhat);
      // (a step at the rounding level of the iterate or of the gradient measures nothing)
      if (s[1] > 0.0 && s[0] * n.Lhat * n.Lhat > 1e-20 * s[5] && s[2] > 1e-20 * s[5])
        n.mu_rq = c.mu_rq > 0.0 ? fmin(c.mu_rq, n.ak) : n.ak;
    } else {
      n.ak = fmin(2.0 * c.ak, 1e6 * c.Lhat);
      n.rejects = c.rejects + 1;
    }
  }
  if (accept) {  // push F(z) into the ring of the last BB_HIST accepted values
    if (n.n_hist < BB_HIST) {
      SLM_UNROLL
      for (int k = 0; k < BB_HIST; ++k) n.hist[k] = k == n.n_hist ? Fz : n.hist[k];  // (a choice of values: a conditional store
                                                                                     //  becomes a choice of addresses, and hist[] goes to memory)
      n.n_hist += 1;
    } else {
      SLM_UNROLL
      for (int k = 0; k + 1 < BB_HIST; ++k) n.hist[k] = n.hist[k + 1];
      n.hist[BB_HIST - 1] = Fz;
    }
    n.have_base = 1;
    n.loss_base = c.loss_z;
  }
  n.stored = accept;
  n.fallback = !n.nonfinite && (n.rejects >= BB_REJECT_LIMIT || c.iter + 1 > BB_POINT_LIMIT);
  return accept;
}

// The switch to FISTA (n.fallback): it restarts from the base point with the largest curvature seen.  A point out of
// iterations is reported as it stands (the caller fills resid / bnorm).
SLM_HD SLM_INLINE void bb_fallback(const TailSnap& c, TailNext& n) {
  n.mode = 0;
  n.t = 1.0;
  n.L = fmax(c.L, n.Lhat);
  n.finalize = c.hit_max;
}

// Stopping rule of the spectral scheme on the new candidate c = prox(base - gradient / ak):
//  q[0] = ||c - base||^2   q[1] = ||c||^2   q[2] = pen(c)   q[3] = #non-finite
SLM_HD SLM_INLINE void bb_stop(const TailSnap& c, TailNext& n, const double (&s)[6], const double (&q)[4]) {
  n.nonfinite = n.nonfinite || q[3] > 0.0 || !isfinite(q[0]) || !isfinite(q[1]);
  n.pen_z = q[2];
  n.resid = sqrt(q[0]) * fmax(1.0, n.ak / n.Lhat);
  n.bnorm = sqrt(q[1]);
  n.kkt = sqrt(q[0]) * n.ak;  // ||G_s(base)||, s = 1 / ak
  n.mu_eff = fmin(n.ak, n.Lhat);
  if (n.mu_rq > 0.0) n.mu_eff = fmin(n.mu_eff, n.mu_rq);
  if (c.mu > 0.0) n.mu_eff = fmin(n.mu_eff, c.mu);
  n.mu_eff = fmax(n.mu_eff, kMuFloor * n.Lhat);
  // (second term: a prox step at the rounding level of the gradient itself cannot be improved)
  n.conv = !c.provisional && n.kkt <= fmax(c.tol * fmax(n.bnorm, c.bnorm_floor) * n.mu_eff, c.round_floor * (sqrt(s[5]) + n.Lhat * n.bnorm));
  n.finalize = n.nonfinite || n.conv || c.hit_max;
}

// ================= FISTA scheme =================================================================
//  s[0] = ||b+ - z||^2   s[1] = ||b+||^2   s[2] = (z - b+).(b+ - b)   s[3] = ||g - gprev||^2
//  s[4] = ||z - zprev||^2   s[5] = ||z||^2   s[6] = #non-finite
//  s[7] = ||g||^2   s[8] = <g - gprev, z - zprev>
// b+ = prox(z - g / L): the curvature guard on L, the restart, the momentum of the next point and the stopping rule.
SLM_HD SLM_INLINE void fista_decide(const TailSnap& c, TailNext& n, const double (&s)[9]) {
  n.loss_base = c.loss_z;  // (zprev = z)
  n.nonfinite = s[6] > 0.0 || !isfinite(s[0]) || !isfinite(s[1]) || !isfinite(c.loss_z);
  // Curvature guard: ||A dz|| / ||dz|| is a lower bound on lambda_max(A), A = X^T W X / n.  If it
  // exceeds L the step 1/L was too long: raise L, discard the step and restart from beta.
  if (c.total_iter > 0 && s[4] > 1e-12 * s[5] && s[4] > 0.0) {
    const double curv = sqrt(s[3] / s[4]);
    if (curv > c.L * (1.0 + 1e-9)) {
      n.l_bad = true;
      n.L = 1.02 * curv;
    }
    // curvature along the move of the extrapolated point: a Rayleigh quotient of X^T W X / n, i.e. an upper
    // estimate of the strong convexity on the face the iteration is on
    if (s[8] > 0.0 && s[3] > 1e-20 * s[7]) n.mu_rq = c.mu_rq > 0.0 ? fmin(c.mu_rq, s[8] / s[4]) : s[8] / s[4];
  }
  n.did_restart = !(c.flags & SLM_FLAG_NO_RESTART) && s[2] > 0.0;
  const double t_use = n.did_restart ? 1.0 : c.t;
  const double t_new = 0.5 * (1.0 + sqrt(1.0 + 4.0 * t_use * t_use));
  n.mom = (t_use - 1.0) / t_new;
  n.resid = sqrt(s[0]);
  n.bnorm = sqrt(s[1]);
  n.kkt = n.resid * c.L;  // ||G_s(z)||, s = 1 / L
  n.mu_eff = c.mu > 0.0 ? fmin(c.mu, c.L) : c.L;
  if (n.mu_rq > 0.0) n.mu_eff = fmin(n.mu_eff, n.mu_rq);
  n.mu_eff = fmax(n.mu_eff, kMuFloor * c.L);
  n.conv = !c.provisional && !n.l_bad && (n.kkt <= fmax(c.tol * fmax(n.bnorm, c.bnorm_floor) * n.mu_eff, c.round_floor * (sqrt(s[7]) + c.L * n.bnorm)));
  n.finalize = n.nonfinite || n.conv || c.hit_max;
  n.t = n.l_bad ? 1.0 : t_new;
}

// What the record of a finalized point says of its outcome.
SLM_HD SLM_INLINE int tail_status(const TailNext& n) {
  return (n.conv && !n.nonfinite) ? SLM_OK : (n.nonfinite ? SLM_ERR_NON_FINITE : SLM_ERR_NOT_CONVERGED);
}

// Where the lane goes once a point is finalized.
struct TailRoute {
  bool secant;      // the next point may start from the secant through the last two solutions (slm_path_point::extrap)
  bool range_end;   // no regular point of the range is left and no tail point either: the lane has finished its range
  bool goes_idle;   // shared-path mode: the lane waits for steal_kernel to hand it new work or retire it
  int32_t next_point;
};

SLM_HD SLM_INLINE TailRoute tail_route(const TailSnap& c, const TailNext& n, bool steal) {
  TailRoute r;
  const int32_t stride = c.stride > 1 ? c.stride : 1;
  // (interleaved lanes: the neighbouring points belong to other lanes and finish in this same launch,
  //  so there is no secant through them -- the next point starts from this lane's last solution)
  r.secant = n.finalize && !c.cold && !n.nonfinite && stride == 1 && c.point - c.pt_lo >= 1 && c.point + 1 < c.n_points;
  const bool walk_end = c.point + stride >= c.n_points;  // (the tail point itself lies beyond n_points)
  r.range_end = n.finalize && !n.nonfinite && walk_end && (c.tail_pt < 0 || c.point == c.tail_pt);
  r.goes_idle = r.range_end && steal;
  r.next_point = (walk_end && c.tail_pt >= 0 && c.point != c.tail_pt) ? c.tail_pt : c.point + stride;
  return r;
}

}  // namespace slm
