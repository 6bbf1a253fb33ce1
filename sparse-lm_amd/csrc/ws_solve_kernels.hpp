// The working-set model solver (ws_kernels.hpp (iv): WsCtl, the Gram and the constants live there); engine_path.hip launches it.
#pragma once
#include "host_logic.hpp"
#include "ws_kernels.hpp"

namespace slm {

// Workgroup sums of the model solver: only the threads of the first `nwc` wavefronts (4 or 8: the ones with q == 0, a
// position each) bring a value, every thread gets bit-identical totals.  block_sum makes all sixteen wavefronts scan
// their zeros and fold sixteen partial sums each: 1.8 us per iteration for seven values, issue-bound on the fp64 DPP adds
// of four wavefronts per SIMD (in-kernel clock marks).  Here the scan runs where the values are, and a lane reads ONE
// partial sum per value and folds it with its quad (or half-row) by commutative pairings.
template <int NV>
__device__ __forceinline__ void ws_sum(double (&v)[NV], double (*lds)[TAIL_WAVES], int nwc) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wave < nwc) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_sum_lane63(v[k]);
  }
  __syncthreads();  // protect lds from the previous use
  if (wave < nwc && lane == 63) {
#pragma unroll
    for (int k = 0; k < NV; ++k) lds[k][wave] = v[k];
  }
  __syncthreads();
  if (nwc == 4) {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = group_sum_all<4>(lds[k][lane & 3]);
  } else {
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = group_sum_all<8>(lds[k][lane & 7]);
  }
}

// ---------------------------------------------------------------------------------------------
// (iv) refinement: one workgroup per lane minimises the penalised quadratic model over W.
// Threads q KP + k work on working-set position k (q splits the matrix-vector product; TPC = 4 parts, or 2 beyond 256
// positions).  Up to WS_KLDS columns the Gram is copied into LDS first, so an inner iteration never leaves the CU.
// ---------------------------------------------------------------------------------------------
// GROUPED: the dataset has real groups (compiled apart from the per-feature variant: each instance carries one
// direct step, and the registers of the other's never weigh on its iteration loop).
// DIRECT = false: the iteration alone.  A lane whose solve would take a direct step is left, untouched, to the
// DIRECT instance launched right behind (WsCtl::want_full; returns false).  Most solves never take one, and the
// kernel without the factorisation is a fifth of the code, keeps its registers (the full one spills 250 of them
// at 128 per thread) and leaves no scratch lines for the end of the kernel to write back.
// LDS of the model solver: one block per workgroup, handed to ws_refine_lane by the kernel
struct WsSolveLds {
  double delta[WS_KCAP];
  double uim[WS_KCAP];
  double part[WS_THREADS];
  double Gl[WS_KLDS * WS_KLDS];
  // direct step (newton_kernels.hpp)
  NtShared nts;
  double nv[WS_KCAP];   // right-hand side / solution, indexed by rank in the face
  double xsl[WS_KCAP];  // direct step with group norms: the base point,
  double rgl[WS_KCAP];  // the norm of each position's group there,
  double pbl[WS_KCAP];  // and its group weight
  double scale2;        // the length scale of the problem on W (see the iteration)
  int nz[WS_KCAP];
  int act[WS_KCAP];      // position of the ii-th face coordinate
  int rank_of[WS_KCAP];  // rank of a position in the face, or -1
  int nnz, m;
};

// A thread's fixed view of its lane's solve (handed on by value: by reference the instances with direct steps took
// 16 and 4 bytes of scratch more).
// 4 threads per position up to 256 positions, 2 beyond (1024 threads, WS_KCAP = 512)
// Thread q KP + k works on position k, KP = WS_THREADS / TPC: the lanes of a wavefront hold CONSECUTIVE
// positions and one q, so a Gram row segment is one coalesced 512-byte load.  (With the TPC threads of a
// position next to each other the lanes alternated between TPC rows 4 KiB apart and every lane became
// its own memory request: 28 us per product at K = 272, in-kernel clock marks.)
struct WsThread {
  int tid, k, q, K, TPC, KP;
  int nwc;            // wavefronts whose threads account for a position (q == 0): 4 or 8 -- ws_sum
  bool live, mine;    // position k holds a feature; this is the thread that accounts for it in reductions
  int jj;             // its feature (0 when not live)
  double z0, g0;      // expansion point and gradient there
  double pa, pb, pd;  // l1, group and ridge weight at the current path point
  int gsk, glk;       // first position and members of k's group
  bool group_pen, singleton, g_lds;  // a group or ridge term; every feature its own group; the Gram sits in sh.Gl
  const double* Gm;
  WsCtl* ws;
  int lane_id;
  double* ntF;        // factor of this lane's direct solves (nullptr: none); the inverses of its diagonal blocks follow it
  double (*red)[TAIL_WAVES];
  WsSolveLds& sh;
  __device__ __forceinline__ double* ntD() const { return ntF + (int64_t)NT_TILES * 256; }
};

// Wave 0: the positions kk < K with flag[kk] != 0 into `list`, in position order (ballots); `rank` (nullable) receives the
// place of each.  Returns their number.
__device__ __forceinline__ int ws_pack(const double* flag, int K, int* list, int* rank) {
  const int lane = threadIdx.x;
  int base = 0;
  for (int c0 = 0; c0 < K; c0 += 64) {
    const int kk = c0 + lane;
    const bool on = kk < K && flag[kk] != 0.0;
    const uint64_t m = __ballot(on);
    if (on) {
      const int ii = base + __popcll(m & ((1ull << lane) - 1ull));
      list[ii] = kk;
      if (rank) rank[kk] = ii;
    }
    base += __popcll(m);
  }
  return base;
}

// G (val - z0) for the vector held as `val` at every position.  Every call is followed by a
// block_sum before the next one, so delta is never overwritten while it is being read.
__device__ __forceinline__ double ws_matvec(WsThread c, double val, bool dense) {
  WsSolveLds& sh = c.sh;
  const int k = c.k, q = c.q, K = c.K, TPC = c.TPC;
  const double* Gm = c.Gm;
  if (q == 0) sh.delta[k] = (k < K) ? val - c.z0 : 0.0;
  __syncthreads();
  double acc = 0.0;
  if (c.g_lds) {
    if (k < K) {
#pragma unroll 4
      for (int cc = q; cc < K; cc += TPC) acc = __builtin_fma(sh.Gl[cc * K + k], sh.delta[cc], acc);
    }
  } else if (dense) {
    // Gram through L2 (K > WS_KLDS): the loads of a batch are issued together, then consumed in the same
    // order as before (one FMA chain).  Left to the compiler the loop ran one load at a time: 28 us per
    // product at K = 272 (in-kernel clock marks), i.e. 0.3 ms of power iteration per selection.
    // (the last batch is a full one too, its entries past the end read the batch's first row again and count with a
    //  factor of zero: left to a loop of its own the tail ran one load at a time, 0.2 us each -- twelve of them per
    //  product at K = 176, half the power iteration)
    if (k < K) {
      for (int cc = __builtin_amdgcn_readfirstlane(q); cc < K; cc += 16 * TPC) {
        double gv[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) gv[u] = Gm[(cc + u * TPC < K ? cc + u * TPC : cc) * WS_KCAP + k];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = __builtin_fma(gv[u], cc + u * TPC < K ? sh.delta[cc + u * TPC] : 0.0, acc);
      }
    }
  } else {
    if (c.tid < 64) {  // compact list of the non-zero entries
      const int n = ws_pack(sh.delta, K, sh.nz, nullptr);
      if (c.tid == 0) sh.nnz = n;
    }
    __syncthreads();
    // (q, the list and its length are the same for all lanes of a wavefront: told to the compiler, the sixteen row
    //  numbers and the in-range tests live in scalar registers)
    const int nnz = __builtin_amdgcn_readfirstlane(sh.nnz);
    const int qs = __builtin_amdgcn_readfirstlane(q);
    // (full batches to the end, as above: the headline's solves have 10-60 non-zeros, FEWER than the 16 TPC a batch
    //  used to need -- every one of their products ran in the one-load-at-a-time tail, 2.4 us of a 5.6 us iteration.
    //  Twelve per batch: sixteen cost the kernel without direct steps 28 bytes of scratch.)
    if (k < K) {
      for (int m = qs; m < nnz; m += 12 * TPC) {
        int cc[12];
        double gv[12];
#pragma unroll
        for (int u = 0; u < 12; ++u) cc[u] = __builtin_amdgcn_readfirstlane(sh.nz[m + u * TPC < nnz ? m + u * TPC : m]);
#pragma unroll
        for (int u = 0; u < 12; ++u) gv[u] = Gm[cc[u] * WS_KCAP + k];
#pragma unroll
        for (int u = 0; u < 12; ++u) acc = __builtin_fma(gv[u], m + u * TPC < nnz ? sh.delta[cc[u]] : 0.0, acc);
      }
    }
  }
  // the TPC parts of a position sit in different wavefronts: fold them through LDS, in a fixed order
  sh.part[c.tid] = acc;
  __syncthreads();
  double tot = sh.part[k];
  for (int qq = 1; qq < TPC; ++qq) tot += sh.part[qq * c.KP + k];
  return tot;
}

// prox of the lane's penalty at the current path point, step s, on the W coordinates
__device__ __forceinline__ double ws_prox(WsThread c, double v, double s) {
  double u = c.live ? soft(v, s * c.pa) : 0.0;
  if (c.group_pen) {
    if (c.singleton) {
      const double nrm = fabs(u);
      const double sc = nrm > 0.0 ? fmax(0.0, 1.0 - s * c.pb / nrm) : 0.0;
      u *= sc / (1.0 + s * c.pd);
    } else {
      __syncthreads();
      if (c.q == 0) c.sh.uim[c.k] = u;
      __syncthreads();
      double ss = 0.0;
      for (int m = 0; m < c.glk; ++m) {
        const double t = c.sh.uim[c.gsk + m];
        ss = __builtin_fma(t, t, ss);
      }
      const double nrm = sqrt(ss);
      const double sc = (nrm > 0.0 ? fmax(0.0, 1.0 - s * c.pb / nrm) : 0.0) / (1.0 + s * c.pd);
      u *= sc;
    }
  }
  return u;
}

// penalty value of the vector held as `val` (thread-partial: counted once per position / group)
__device__ __forceinline__ double ws_pen_part(WsThread c, double val) {
  const int k = c.k;
  double pv = 0.0;
  if (c.mine) {
    pv = c.pa * fabs(val);
    if (c.group_pen && c.singleton) pv += c.pb * fabs(val) + 0.5 * c.pd * val * val;
  }
  if (c.group_pen && !c.singleton) {
    __syncthreads();
    if (c.q == 0) c.sh.uim[k] = c.live ? val : 0.0;
    __syncthreads();
    if (c.mine && c.gsk == k) {  // first member of the group
      double ss = 0.0;
      for (int m = 0; m < c.glk; ++m) ss = __builtin_fma(c.sh.uim[k + m], c.sh.uim[k + m], ss);
      pv += c.pb * sqrt(ss) + 0.5 * c.pd * ss;
    }
  }
  return pv;
}

// model value (relative to the expansion point) and penalty of the vector held as `val`, thread-partial (one product)
__device__ __forceinline__ void ws_value_parts(WsThread c, double val, double* out) {
  const double gd = ws_matvec(c, val, false);
  out[0] = c.mine ? (val - c.z0) * (c.g0 + 0.5 * gd) : 0.0;
  out[1] = ws_pen_part(c, val);
}

__device__ __forceinline__ double ws_block_min(WsThread c, double val) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) val = fmin(val, __shfl_xor(val, off, 64));
  __syncthreads();
  if ((c.tid & 63) == 0) c.red[0][c.tid >> 6] = val;
  __syncthreads();
  double mm = c.red[0][0];
#pragma unroll
  for (int wv = 1; wv < TAIL_WAVES; ++wv) mm = fmin(mm, c.red[0][wv]);
  return mm;
}

// sum of `val` over the members of this position's group
__device__ __forceinline__ double ws_group_sum(WsThread c, double val) {
  __syncthreads();
  if (c.q == 0 && c.k < WS_KCAP) c.sh.uim[c.k] = (c.k < c.K && c.live) ? val : 0.0;
  __syncthreads();
  double ss = 0.0;
  if (c.live)
    for (int m2 = 0; m2 < c.glk; ++m2) ss += c.sh.uim[c.gsk + m2];
  return ss;
}

// device clock ticks since the mark before, added to slots[slot] by the thread that keeps the account
__device__ __forceinline__ void ws_tick(bool keeper, unsigned long long* slots, unsigned long long& tk, int slot) {
  if (keeper) {
    const unsigned long long now = wall_clock64();
    slots[slot] += now - tk;
    tk = now;
  }
}

// The linear system of a direct step on the free set F (`is_free`, per position): the free positions ranked in position
// order, H_FF = G_FF + the ridge diagonal (GROUPED: + the curvature of the norms of the active groups at the base point xb,
// rg = the norm of this position's group there) assembled tile by tile and factored, d = H_FF^-1 pg.
// m unknowns, T 16-tiles per side, mp = 16 T; my_rank: rank of this thread's position in F, or -1; dk: its entry of d (0 outside F)
struct WsFace { int m, T, mp, my_rank; double dk; };
// Returns 1, 0 when F is empty (my_rank = -1, dk = 0), -1 when H_FF is not positive definite.
template <bool GROUPED>
__device__ __forceinline__ int ws_face_solve(WsThread c, bool is_free, double pg, double xb, double rg, double Lmax,
                                             WsFace& f, unsigned long long& tk) {
  WsSolveLds& sh = c.sh;
  const int tid = c.tid, k = c.k, q = c.q, K = c.K;
  // free positions in position order
  __syncthreads();
  if (q == 0 && k < WS_KCAP) {
    sh.nv[k] = is_free ? 1.0 : 0.0;
    sh.rank_of[k] = -1;
  }
  __syncthreads();
  if (tid < 64) {
    const int n = ws_pack(sh.nv, K, sh.act, sh.rank_of);
    if (tid == 0) sh.m = n;
  }
  __syncthreads();
  const int m = f.m = sh.m;
  if (m == 0) {
    f.dk = 0.0;
    f.my_rank = -1;
    return 0;
  }
  const int T = f.T = (m + 15) >> 4;
  f.mp = 16 * T;
  const int my_rank = f.my_rank = (k < K) ? sh.rank_of[k] : -1;
  __syncthreads();
  if (tid < f.mp) sh.nv[tid] = 0.0;
  if (q == 0 && k < WS_KCAP) {
    sh.delta[k] = c.pd;  // (matvec is done with delta: it now carries the ridge diagonal)
    if constexpr (GROUPED) {
      sh.xsl[k] = (k < K && c.live) ? xb : 0.0;
      sh.rgl[k] = rg;
      sh.pbl[k] = c.pb;
      sh.nz[k] = c.gsk;  // (group id; the mat-vec rebuilds its own list when it next runs)
    }
  }
  __syncthreads();
  if (q == 0 && my_rank >= 0) sh.nv[my_rank] = pg;
  if constexpr (!GROUPED) ws_tick(tid == 0, c.ws->nt_ticks[c.lane_id], tk, 0);
  // H_FF, tile by tile (G is symmetric: read along rows)
  const int ntl = T * (T + 1) / 2;
  for (int e = tid; e < ntl * 256; e += WS_THREADS) {
    const int tl = e >> 8, wi = e & 255;
    int I, J;
    slm_host::triangle_tile_fast(tl, &I, &J);
    const int l6 = wi & 63, st = wi >> 6;
    const int ii = 16 * I + (l6 & 15), ij = 16 * J + (l6 >> 4) + 4 * st;
    double hv;
    if (ii < m && ij < m) {
      const int pi = sh.act[ii], pj = sh.act[ij];
      hv = c.Gm[pj * WS_KCAP + pi];
      if (ii == ij) hv += sh.delta[pi];
      if constexpr (GROUPED) {
        if (sh.nz[pi] == sh.nz[pj]) {  // same group: curvature of its norm
          const double rr = sh.rgl[pi];
          hv += (sh.pbl[pi] / rr) * ((ii == ij ? 1.0 : 0.0) - sh.xsl[pi] * sh.xsl[pj] / (rr * rr));
        }
      }
    } else {
      hv = ii == ij ? 1.0 : 0.0;
    }
    c.ntF[e] = hv;
  }
  __syncthreads();
  if constexpr (!GROUPED) ws_tick(tid == 0, c.ws->nt_ticks[c.lane_id], tk, 1);
  if (!nt_factor(c.ntF, c.ntD(), T, 1e-12 * Lmax, sh.nts)) {
    if (tid == 0) atomicAdd(&c.ws->newton_nopd, 1);
    return -1;
  }
  if constexpr (!GROUPED) ws_tick(tid == 0, c.ws->nt_ticks[c.lane_id], tk, 2);
  nt_solve(c.ntF, c.ntD(), T, sh.nv);  // nv = H_FF^-1 pg
  if constexpr (!GROUPED) ws_tick(tid == 0, c.ws->nt_ticks[c.lane_id], tk, 3);
  if (tid == 0) {
    atomicAdd(&c.ws->newton_factors, 1);
    c.ws->nt_factors[c.lane_id] += 1;
    atomicAdd(&c.ws->newton_unknowns, m);
  }
  f.dk = my_rank >= 0 ? sh.nv[my_rank] : 0.0;
  return 1;
}

// The base point xb minus t times the step of a face coordinate, stopped at zero (cut) where a coordinate whose sign is
// part of the face (kink) would leave its orthant xi or land on its boundary
__device__ __forceinline__ double ws_arc(double xb, double t, double dk, bool on_face, bool kink, double xi, double& cut) {
  if (!on_face) return xb;
  const double xc = xb - t * dk;
  if (!(kink && xc * xi <= 0.0)) return xc;
  if (xb != 0.0 || xc != 0.0) cut = 1.0;
  return 0.0;
}

// A trial point of a direct step: the candidate xc (cut: this thread's coordinate was projected) is accepted when it is
// finite and its model value + penalty lies below m_old.  `projected`: some coordinate of an accepted point was cut.
__device__ __forceinline__ bool ws_trial(WsThread c, double xc, double cut, double m_old, bool& projected) {
  const double gdn = ws_matvec(c, xc, false);
  double sv[4] = {0.0, 0.0, 0.0, 0.0};
  if (c.mine) {
    sv[0] = (xc - c.z0) * (c.g0 + 0.5 * gdn);
    sv[2] = cut;
    if (!isfinite(xc)) sv[3] = 1.0;
  }
  sv[1] = ws_pen_part(c, xc);
  block_sum<4>(sv, c.red);
  if (!(sv[3] == 0.0 && sv[0] + sv[1] < m_old)) return false;
  projected = sv[2] > 0.0;
  return true;
}

// H_FF is the Hessian on the face of the new point: its smallest eigenvalue, two inverse-iteration steps from the step itself
__device__ __forceinline__ double ws_face_mu(WsThread c, const WsFace& f) {
  __syncthreads();
  return nt_lambda_min(c.ntF, c.ntD(), f.T, f.mp, c.sh.nv, c.red, 2);
}

// ---- direct step: projected Newton on the free coordinates ---------------------------------------
// Free set F: the non-zero coordinates of x plus the zero ones whose model gradient exceeds their
// threshold (they want to leave zero); orthant: sign(x), or the side such a coordinate wants to move to.
// Inside the orthant the model + penalty is a smooth quadratic: d = H_FF^-1 (pseudo-gradient) by a Cholesky
// solve, then x - t d projected back onto the orthant (a coordinate that would change sign stops at zero),
// t = 1, 1/2, ... until the model value falls (two-metric projection: F holds no coordinate that the
// gradient pins at zero, so the projected arc is a descent arc).  When nothing is projected at t = 1 the
// result IS the minimiser over that face.  Returns 1 when x moved, 0 when there was nothing to do, -1 when
// H_FF is not positive definite or no trial lowered the model (the iteration simply carries on).  mu_out:
// estimate of the smallest eigenvalue of the face Hessian (0 = not computed).  This is the variant for
// per-feature penalties (and singleton "groups"); real group norms: ws_direct_step_group further down.
// resolve_cap: solves per call while the free set is being made consistent (WS_NEWTON_RESOLVE, or 1: see the end).
__device__ __forceinline__ int ws_direct_step(WsThread c, double& x, double Lmax, double* mu_out, bool want_mu,
                                              int& resolve_cap) {
  const bool live = c.live, mine = c.mine;
  const double z0 = c.z0, g0 = c.g0, pd = c.pd;
  *mu_out = 0.0;
  const double thr = c.pa + c.pb;  // (singleton groups: b acts as a second l1 weight)
  // On an ill-conditioned face the Newton direction lives on cancellations between near-collinear columns:
  // projecting some of its coordinates away leaves a step that is no descent step at any useful length.
  // So the free set is made consistent first, active-set fashion: a zero coordinate stays in F only if the
  // solve moves it to the side it wants to go, a non-zero one only if the solve does not carry it across
  // zero -- the others are set to / kept at zero (and stay out of F for the rest of this call), the
  // pseudo-gradient is re-evaluated there and the system is solved again (WS_NEWTON_RESOLVE times at most:
  // then the projected arc has to do).
  double xb = x;          // base point of the solve: x with the coordinates dropped so far at zero
  bool banned = false;    // this position was dropped: it stays at zero and out of F
  double m_old = 0.0;     // model value at x (relative to the expansion point)
  double d_first = 0.0, t_first = 2.0, pg_first = 0.0;  // first solve: direction, step to the first sign change from x, pg
  bool tiny_first = false;
  WsFace f = {0, 0, 0, -1, 0.0};
  double xi = 1.0;
  unsigned long long tk = wall_clock64();
  for (int resolve = 0; resolve < resolve_cap; ++resolve) {
    ws_tick(c.tid == 0, c.ws->nt_ticks[c.lane_id], tk, 4);
    const double gdb = ws_matvec(c, xb, false);  // G (xb - z0)
    const double gx = g0 + gdb;                  // model gradient at xb
    if (resolve == 0) {
      double sv[2] = {mine ? (x - z0) * (g0 + 0.5 * gdb) : 0.0, 0.0};
      sv[1] = ws_pen_part(c, x);
      block_sum<2>(sv, c.red);
      m_old = sv[0] + sv[1];
    }
    double pg;  // pseudo-gradient of this position at xb; xi: the orthant it may move in
    if (xb != 0.0) {
      xi = xb > 0.0 ? 1.0 : -1.0;
      pg = gx + thr * xi + pd * xb;
    } else {
      pg = fabs(gx) > thr * (1.0 + 1e-12) ? gx - copysign(thr, gx) : 0.0;
      xi = pg > 0.0 ? -1.0 : 1.0;
    }
    // of the zero coordinates that want to leave zero only the strongest enter now (within WS_NEWTON_ENTER of
    // the largest violation): on correlated designs most violators stop violating once a few of them have
    // moved, and a free set full of them solves for a direction that means nothing
    const double viol = (live && !banned && xb == 0.0) ? fabs(pg) : 0.0;
    const double viol_max = -ws_block_min(c, -viol);
    const bool is_free = live && !banned && (xb != 0.0 || (viol > 0.0 && viol >= WS_NEWTON_ENTER * viol_max));
    const int rc = ws_face_solve<false>(c, is_free, pg, xb, 0.0, Lmax, f, tk);
    if (rc < 0) return -1;
    if (rc == 0) {
      if (resolve == 0) return 0;
      break;  // everything was dropped: the base point itself is the candidate
    }
    if (resolve == 0) {
      // (a zero coordinate the first solve sent the wrong way stays where it is)
      d_first = f.my_rank >= 0 && (x != 0.0 || f.dk * pg > 0.0) ? f.dk : 0.0;
      pg_first = pg;
      // a coordinate the solve carries across zero ends the straight segment -- unless it sits so close to
      // zero (the dust a prox-gradient step leaves on every violator) that the segment would have no
      // length: those go to zero outright and take no part in the direction
      tiny_first = f.my_rank >= 0 && x != 0.0 && x * f.dk > 0.0 && fabs(x) < 1e-6 * fabs(f.dk);
      if (tiny_first) d_first = 0.0;
      else if (f.my_rank >= 0 && x != 0.0 && x * f.dk > 0.0 && fabs(f.dk) >= fabs(x)) t_first = x / f.dk;
    }
    // zero coordinates the solve would move to the wrong side (or not at all), non-zero ones it would carry
    // across zero
    const bool wrong = f.my_rank >= 0 && (xb == 0.0 ? !(f.dk * pg > 0.0) : (xb - f.dk) * xi <= 0.0);
    double cnt[1] = {mine && wrong ? 1.0 : 0.0};
    block_sum<1>(cnt, c.red);
    if (cnt[0] == 0.0 || resolve == resolve_cap - 1) break;
    if (wrong) {
      banned = true;
      xb = 0.0;
    }
  }
  t_first = fmin(1.0, ws_block_min(c, t_first));
  {
    // the model along x - t d_first, 0 <= t <= t_first (no coordinate changes sign there), is the parabola
    // m_old - t <pg, d> + t^2/2 <d, H d>: with the wrong-way coordinates held back d is not the Newton direction
    // of what moves, so the full segment need not descend -- its minimiser does
    const double gd = ws_matvec(c, z0 + d_first, false);  // G d_first
    double sv[2] = {0.0, 0.0};
    if (mine) {
      sv[0] = pg_first * d_first;
      sv[1] = d_first * (gd + pd * d_first);
    }
    block_sum<2>(sv, c.red);
    if (c.tid == 0) {
      if (!(t_first > 1e-14)) atomicAdd(&c.ws->newton_ref[0], 1);
      else if (!(sv[0] > 0.0)) atomicAdd(&c.ws->newton_ref[1], 1);
      else if (!(sv[1] > 0.0)) atomicAdd(&c.ws->newton_ref[2], 1);
    }
    t_first = (sv[0] > 0.0 && sv[1] > 0.0) ? fmin(t_first, sv[0] / sv[1]) : 0.0;
  }
  // trial points: the base point minus the (projected) step at t = 1, 1/2, 1/4, then -- from x itself, along
  // the first solve -- the straight segment up to the first sign change (a guaranteed descent step: nothing
  // is projected on it)
  double xn = x;
  bool moved = false, projected = false, full = false;
  for (int trial = 0; trial < 4 && !moved; ++trial) {
    if (trial == 3 && !(t_first > 1e-14)) break;
    double xc, cut = 0.0;
    if (trial < 3) {
      const double tt = trial == 0 ? 1.0 : (trial == 1 ? 0.5 : 0.25);
      xc = ws_arc(xb, tt, f.dk, f.my_rank >= 0, true, xi, cut);
    } else {
      xc = x - t_first * d_first;
      if (tiny_first || (x != 0.0 && xc * x <= 0.0)) xc = 0.0;  // the coordinate that reaches zero there
      cut = 1.0;
    }
    if (ws_trial(c, xc, cut, m_old, projected)) {
      moved = true;
      full = trial == 0;
      xn = xc;
      if (c.tid == 0) atomicAdd(&c.ws->newton_trial[trial], 1);
      // dropping every inconsistent coordinate at once did not settle the free set and the step fell back
      // to the segment: on this face (strong cancellations) the following steps go there directly
      if (trial == 3) resolve_cap = 1;
    }
  }
  ws_tick(c.tid == 0, c.ws->nt_ticks[c.lane_id], tk, 4);
  if (!moved && c.tid == 0 && t_first > 1e-14) atomicAdd(&c.ws->newton_ref[3], 1);
  if (!moved) return -1;
  if (want_mu && full && !projected && f.m > 0) {
    *mu_out = ws_face_mu(c, f);
    ws_tick(c.tid == 0, c.ws->nt_ticks[c.lane_id], tk, 5);
  }
  x = xn;
  return 1;
}

// ---- direct step with group norms (GroupLasso, SparseGroupLasso, ridged; round 2) ----------------------
// On the face of the iterate -- its active groups, inside them the non-zero coordinates with their signs when
// there is an l1 term -- the objective is smooth but no longer quadratic: the norm of an active group adds the
// curvature (b_g / r_g)(I - u u^T), r_g = ||x_g||, u = x_g / r_g.  One call is one damped Newton step there:
// H = G_FF + d + those blocks, d = H^-1 (gradient of the smooth face objective), trial points x - t d for
// t = 1, 1/2, 1/4, 1/8 with the same projections as above (a coordinate with an l1 kink stops at zero; a group the
// step would carry through the origin goes to zero as a whole), the first that lowers model + penalty wins.
// Groups that are zero but want in (||soft(g_g, a)|| > b_g, the strongest violators only) first receive their
// prox-gradient value -- the penalty has no gradient at a zero group -- and join the face.  The free set is made
// consistent by dropping what the solve sends the wrong way, as in the l1 case.
// (It also serves a lane of a dataset with real groups whose current point has no group term: b = 0 adds no curvature.)
__device__ __forceinline__ int ws_direct_step_group(WsThread c, double& x, double Lmax, double* mu_out, bool want_mu,
                                                    int resolve_cap) {
  const bool live = c.live, mine = c.mine;
  const double z0 = c.z0, g0 = c.g0, pa = c.pa, pb = c.pb, pd = c.pd;
  *mu_out = 0.0;
  const bool kink = pa > 0.0;  // this coordinate has an l1 term: its sign is part of the face
  double xb = x, m_old = 0.0, xi = 0.0;
  bool banned = false;
  WsFace f = {0, 0, 0, -1, 0.0};
  unsigned long long tk = 0;  // (this step marks no clock ticks)
  for (int resolve = 0; resolve < resolve_cap; ++resolve) {
    double gx = g0 + ws_matvec(c, xb, false);
    if (resolve == 0) {
      double sv[2] = {mine ? (x - z0) * (g0 + 0.5 * (gx - g0)) : 0.0, 0.0};
      sv[1] = ws_pen_part(c, x);
      block_sum<2>(sv, c.red);
      m_old = sv[0] + sv[1];
    }
    double r2 = ws_group_sum(c, xb * xb);
    bool g_active = r2 > 0.0;
    const double sk = (live && !banned && !g_active) ? soft(gx, pa) : 0.0;
    const double S = sqrt(ws_group_sum(c, sk * sk));
    double viol = 0.0;
    if (live && !banned) {
      if (!g_active) viol = fmax(0.0, S - pb);
      else if (xb == 0.0 && kink) viol = fmax(0.0, fabs(gx) - pa);
    }
    const double viol_max = -ws_block_min(c, -viol);
    if (resolve == 0 && viol_max > 0.0) {
      const bool enter = live && !banned && !g_active && viol > 0.0 && viol >= WS_NEWTON_ENTER * viol_max;
      double cnt[1] = {mine && enter ? 1.0 : 0.0};
      block_sum<1>(cnt, c.red);
      if (cnt[0] > 0.0) {  // (uniform: every thread takes the same branch)
        if (enter) {
          const double st = 1.0 / Lmax;
          xb = -st * sk * (1.0 - pb / S) / (1.0 + st * pd);
        }
        gx = g0 + ws_matvec(c, xb, false);
        r2 = ws_group_sum(c, xb * xb);
        g_active = r2 > 0.0;
      }
    }
    const double rg = sqrt(r2);
    double pg = 0.0;
    bool is_free = false;
    xi = 0.0;
    if (live && !banned && g_active) {
      if (xb != 0.0) {
        xi = kink ? (xb > 0.0 ? 1.0 : -1.0) : 0.0;
        pg = gx + pa * (xb > 0.0 ? 1.0 : -1.0) + (pb / rg + pd) * xb;
        is_free = true;
      } else if (!kink) {
        pg = gx;  // no l1 term: the objective is smooth in this coordinate at zero
        is_free = gx != 0.0;
      } else {
        const double e = fabs(gx) - pa;
        if (e > 0.0 && e >= WS_NEWTON_ENTER * viol_max) {
          pg = gx - copysign(pa, gx);
          xi = pg > 0.0 ? -1.0 : 1.0;
          is_free = true;
        }
      }
    }
    const int rc = ws_face_solve<true>(c, is_free, pg, xb, rg, Lmax, f, tk);
    if (rc < 0) return -1;
    if (rc == 0) {
      if (resolve == 0) return 0;
      break;
    }
    // what the solve sends the wrong way: a kinked coordinate across (or to the wrong side of) zero, a whole
    // group through the origin
    bool wrong = false;
    if (f.my_rank >= 0 && kink) wrong = xb == 0.0 ? !(f.dk * pg > 0.0) : (xb - f.dk) * xi <= 0.0;
    const double radial = ws_group_sum(c, live && !banned ? (xb - f.dk) * xb : 0.0);
    const bool g_wrong = live && !banned && g_active && !(radial > 0.0);
    double cnt[1] = {mine && (wrong || g_wrong) ? 1.0 : 0.0};
    block_sum<1>(cnt, c.red);
    if (cnt[0] == 0.0 || resolve == resolve_cap - 1) break;
    if (wrong || g_wrong) {
      banned = true;
      xb = 0.0;
    }
  }
  double xn = x;
  bool moved = false, projected = false, full = false;
  double tt = 1.0;
  for (int trial = 0; trial < 4 && !moved; ++trial, tt *= 0.5) {
    double cut = 0.0;
    double xc = ws_arc(xb, tt, f.dk, f.my_rank >= 0, kink, xi, cut);
    const double radial = ws_group_sum(c, live ? xc * xb : 0.0);
    const double r2b = ws_group_sum(c, xb * xb);
    if (live && r2b > 0.0 && !(radial > 0.0)) {  // the group would pass through the origin: it goes to zero
      if (xc != 0.0) cut = 1.0;
      xc = 0.0;
    }
    if (ws_trial(c, xc, cut, m_old, projected)) {
      moved = true;
      full = trial == 0;
      xn = xc;
      if (c.tid == 0) atomicAdd(&c.ws->newton_trial[trial < 3 ? trial : 2], 1);
    }
  }
  if (!moved) return -1;
  if (want_mu && full && !projected && f.m > 0) *mu_out = ws_face_mu(c, f);
  x = xn;
  return 1;
}

template <bool GROUPED>
__device__ __forceinline__ int ws_direct(WsThread c, double& x, double Lmax, double* mu_out, bool want_mu, int& resolve_cap) {
  if constexpr (GROUPED) return ws_direct_step_group(c, x, Lmax, mu_out, want_mu, resolve_cap);
  else return ws_direct_step(c, x, Lmax, mu_out, want_mu, resolve_cap);
}

// ---- lambda_max of this Gram (once per selection): power iteration from a fixed start ---------
__device__ __forceinline__ double ws_lambda_max(WsThread c, int power_iters) {
  const int k = c.k, K = c.K;
  double vec = (k < K) ? 1.0 + 0.37 * (double)(((k * 2654435761u) >> 24) & 0xffu) / 255.0 : 0.0;
  double lam = 0.0;
  for (int itp = 0; itp < power_iters; ++itp) {
    const double y = ws_matvec(c, vec + c.z0, true);  // matvec works on (val - z0)
    double s[1] = {c.q == 0 && k < K ? y * y : 0.0};
    ws_sum<1>(s, c.red, c.nwc);
    lam = sqrt(s[0]);
    vec = lam > 0.0 ? y / lam : 0.0;
  }
  return lam * 1.1;  // from below; the curvature guard in the loop covers the rest
}

// What the iteration hands to the acceptance and the write-back
struct WsIterate {
  double x, L;      // the point reached, the curvature bound at the end
  bool settled;     // the iteration met its own tolerance: its point minimises the model
  int n_inner;
  // smallest Rayleigh quotient <dv, G dv> / <dv, dv> along the moves of the iteration: an upper estimate
  // of the smallest eigenvalue on the face that closes in as the slow modes come to dominate the moves
  double rq_min;
  int rq_n;
  double mu_face;   // from the factor of a direct step (0: none taken)
  int n_direct, n_direct_bad;
};

// ---- FISTA on the model ------------------------------------------------------------------------
// Returns 1, 0 when a step was not finite (nothing is to be written), -1 when this solve would take a direct step and the
// instance has none (DIRECT = false: WsCtl::want_full is set, nothing of the solve has been written).
template <bool GROUPED, bool DIRECT>
__device__ __forceinline__ int ws_iterate(WsThread c, const WsArgs& w, double x_start, double Lw, double tol, int hard_now,
                                          WsIterate& r) {
  double L = Lw;
  double Ls = L;  // curvature the next step is taken with (L, or less while the steps are spectral)
  double x = x_start, v = x_start, t = 1.0;
  double v_prev = 0.0, gv_prev = 0.0;
  bool have_prev = false;
  bool settled = false;
  int n_inner = 0;
  double rq_min = 0.0;
  int rq_n = 0;
  double mu_face = 0.0;
  int since_direct = 0, n_direct = 0, n_direct_bad = 0;
  int resolve_cap = WS_NEWTON_RESOLVE;
  bool direct_on = c.ntF != nullptr;
  // direct mode: the iterate only moves by direct steps; the prox-gradient step of every round is just the
  // convergence test (taken when it passes).  Taking it regardless would wreck the next direct step: from a
  // face minimiser one prox-gradient step gives EVERY violator a tiny non-zero value, and a free set full of
  // those solves for a direction that means nothing.  A solve starts in this mode when an earlier refinement of ITS LANE
  // of this call needed direct steps (WsCtl::hard_lane).
  bool direct_mode = direct_on && hard_now != 0;
  // the length scale of the problem on W: a gradient step from the expansion point, ||g0_W|| / L (what "rounding level" is
  // measured against where the iterate itself is zero or dust)
  // (kept in LDS, not in a register across the loop: the kernel sits at the 128 registers of a 1 024-thread workgroup, and a
  //  value more across the iteration was 12 bytes of scratch per thread)
  {
    double sg[1] = {c.mine ? c.g0 * c.g0 : 0.0};
    ws_sum<1>(sg, c.red, c.nwc);
    if (c.tid == 0) c.sh.scale2 = sg[0] / (Lw * Lw);
    __syncthreads();
  }
  // The first WS_BB_ITERS steps carry no momentum and take their length from the curvature along the move
  // before: on the well-conditioned faces of an easy path that is there in half the steps of the accelerated
  // iteration, which takes over if it is not.
  bool spectral = !direct_mode && w.bb_steps != 0;
  int it_end = WS_INNER_MAX;
  for (int it = 0; it < it_end; ++it) {
    ++n_inner;
    const double gv = c.g0 + ws_matvec(c, v, false);
    const double u = ws_prox(c, v - gv / Ls, 1.0 / Ls);
    //  s[0] = ||u - v||^2  s[1] = ||u||^2  s[2] = (v - u).(u - x)  s[3] = #non-finite
    //  s[4] = ||v - v_prev||^2  s[5] = ||gv - gv_prev||^2   (curvature along the last move of v)
    //  s[6] = <v - v_prev, gv - gv_prev>
    double s[7] = {0, 0, 0, 0, 0, 0, 0};
    if (c.mine) {
      const double rr = u - v;
      s[0] = rr * rr;
      s[1] = u * u;
      s[2] = -rr * (u - x);
      if (!isfinite(u)) s[3] = 1.0;
      if (have_prev) {
        const double dv = v - v_prev, dg = gv - gv_prev;
        s[4] = dv * dv;
        s[5] = dg * dg;
        s[6] = dv * dg;
      }
    }
    ws_sum<7>(s, c.red, c.nwc);
    if (s[3] > 0.0 || !isfinite(s[0])) return 0;
    v_prev = v;
    gv_prev = gv;
    have_prev = true;
    if (s[4] > 1e-20 * fmax(s[1], c.sh.scale2) && s[4] > 0.0) {  // (a move at the rounding level measures nothing)
      const double rq = s[6] / s[4];
      if (rq > 0.0 && (rq_n == 0 || rq < rq_min)) rq_min = rq;
      rq_n += 1;
    }
    // (a move at the rounding level measures no curvature either -- and "rounding level" has to be told on the scale of
    //  the PROBLEM, not of the iterate: the point at alpha_max solves to rounding dust (|g_j| - alpha = 1e-16 for the
    //  first feature), its moves are dust against dust, ||dg|| / ||dv|| of one of them sent L from 1.7 to 44 -- through
    //  WsCtl::Lw for every later refinement of the call, whose Rayleigh quotients then all "said" ill-conditioned: 170
    //  direct steps of 200 unknowns on an iid design, 26 ms for an 8-pass path, soak seed 29)
    const bool real_move = s[4] > 1e-20 * fmax(s[1], c.sh.scale2) && s[4] > 0.0;
    if (real_move && sqrt(s[5] / s[4]) > L) {  // the bound was too low
      L = 1.05 * sqrt(s[5] / s[4]);
      if (!spectral) {  // an accelerated step of 1/L was too long: redo it from x (a spectral step claims nothing of L)
        Ls = L;
        v = x;
        t = 1.0;
        continue;
      }
    }
    if (spectral) {
      // the next step is as long as the curvature along this move allows (Barzilai-Borwein, first form),
      // never longer than WS_BB_MAX_STEP steps of 1/L
      const double rq = s[4] > 1e-20 * s[1] ? s[6] / s[4] : L;
      Ls = fmin(L, fmax(rq, L / WS_BB_MAX_STEP));
      if (it + 1 >= WS_BB_ITERS) {  // not there in the steps such a face takes: momentum from here
        spectral = false;
        Ls = L;
      }
    }
    // (a spectral step is longer than 1/L and moves at least as far from the same point: the test is the stricter for it)
    // (... or the step is rounding noise on the problem's scale, the floor of fista_tail_kernel's stopping rule: a solution
    //  that IS dust -- the path's first point -- has converged, it does not iterate thirty times and take a direct step)
    const bool inner_conv = sqrt(s[0]) <= fmax(WS_INNER_TOL * tol * sqrt(s[1]), kRoundFloor * (sqrt(c.sh.scale2) + sqrt(s[1])));
    if (DIRECT && direct_mode && !inner_conv) {
      bool stepped = false;
      if (n_direct < WS_NEWTON_MAX) {
        double mu_new = 0.0;
        const int rc = ws_direct<GROUPED>(c, x, L, &mu_new, mu_face == 0.0, resolve_cap);
        n_direct += 1;
        if (rc > 0) {
          if (mu_new > 0.0) mu_face = mu_new;
          stepped = true;
        } else if (rc < 0) {
          n_direct_bad += 1;
        }
      }
      if (stepped) {
        v = x;
        t = 1.0;
        continue;
      }
      // no usable step from this point (e.g. the coordinates it had to hold back carried the descent): one
      // prox-gradient step moves the iterate somewhere else and the next round tries again; after
      // WS_NEWTON_REFUSALS of those, or at the cap, the iteration finishes the job
      if (n_direct_bad >= WS_NEWTON_REFUSALS || n_direct >= WS_NEWTON_MAX) {
        direct_mode = false;
        direct_on = false;
        since_direct = 0;
        it_end = min(it_end, it + WS_AFTER_DIRECT);
      }
    }
    const bool restart = s[2] > 0.0;
    const double t_use = restart ? 1.0 : t;
    const double t_new = 0.5 * (1.0 + sqrt(1.0 + 4.0 * t_use * t_use));
    const double mom = spectral ? 0.0 : (t_use - 1.0) / t_new;
    v = u + mom * (u - x);
    x = u;
    t = t_new;
    if (inner_conv) {
      settled = true;
      break;
    }
    since_direct += 1;
    if (direct_on && n_direct < WS_NEWTON_MAX &&
        (since_direct >= WS_NEWTON_AFTER || (rq_n >= 5 && rq_min < WS_NEWTON_RQ * L))) {
      if (!DIRECT) {  // (nothing of this solve has been written yet)
        if (c.tid == 0) c.ws->want_full[c.lane_id] = 1;
        return -1;
      }
      double mu_new = 0.0;
      const int rc = ws_direct<GROUPED>(c, x, L, &mu_new, mu_face == 0.0, resolve_cap);
      since_direct = 0;
      n_direct += 1;
      if (rc > 0) {
        if (mu_new > 0.0) mu_face = mu_new;
        v = x;
        t = 1.0;
        direct_mode = true;
      } else if (rc < 0) {
        n_direct_bad += 1;
        if (n_direct_bad >= WS_NEWTON_REFUSALS) {  // singular face / useless steps: the iteration finishes the job
          direct_on = false;
          if (n_direct > n_direct_bad) it_end = min(it_end, it + WS_AFTER_DIRECT);
        }
      }
    }
  }
  r = WsIterate{x, L, settled, n_inner, rq_min, rq_n, mu_face, n_direct, n_direct_bad};
  return 1;
}

// An iteration that ran out of steps is accepted only if the model says its point is no worse than the start (two
// products with the Gram, 14 us per call).  Not spent on a point that met the tolerance -- a minimiser of the model is
// no worse than anything -- unless the START already met it (one iteration): that point is one proximal step from
// where the lane stood, now and then a hair worse, and taking it resets the lane's step history for nothing.  On
// paths whose ends outgrow the working set such solves are common (a fifth to a half of all) and accepting them
// unseen cost 4-6 passes of 24-58 (tools/headline_soak.py); the headline path has none.
__device__ __forceinline__ bool ws_no_worse(WsThread c, double x_start, double x) {
  double m_start;  // model values relative to the expansion point
  {
    double s[2];
    ws_value_parts(c, x_start, s);
    ws_sum<2>(s, c.red, c.nwc);
    m_start = s[0] + s[1];
  }
  double s[3];
  ws_value_parts(c, x, s);
  s[2] = c.mine && !isfinite(x) ? 1.0 : 0.0;
  ws_sum<3>(s, c.red, c.nwc);
  const double m_end = s[0] + s[1];
  return !(s[2] > 0.0) && m_end <= m_start;
}

// the refined point: model minimiser on W, the expansion point elsewhere (eight features per round: their loads
// go out together -- one feature at a time every load waited for the one before it, 11 us per call)
__device__ __forceinline__ void ws_write_point(WsThread c, const TailArgs& a, const WsArgs& w, int mode, double x) {
  const int p = a.p;
  for (int f0 = c.tid; f0 < p; f0 += 8 * WS_THREADS) {
    int ps[8];
    double zo[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int f = f0 + u * WS_THREADS;
      const int ff = f < p ? f : 0;
      ps[u] = f < p ? w.pos[ff] : 0;
      zo[u] = a.zprev[ff];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int f = f0 + u * WS_THREADS;
      if (f < p && ps[u] < 0) {
        a.z[f] = zo[u];
        if (mode == 0) a.beta[f] = zo[u];
      }
    }
  }
  if (c.mine) {
    a.z[c.jj] = x;
    if (mode == 0) a.beta[c.jj] = x;
  }
}

// The decline tests, lambda_max of a new Gram, the iteration, its acceptance, the write-back; false: left to the DIRECT instance
template <bool GROUPED, bool DIRECT>
__device__ __forceinline__ bool ws_refine_lane(TailArgs a, const WsArgs& w, double (*red)[TAIL_WAVES], WsSolveLds& sh) {
  const int lane_id = blockIdx.x;
  PathCtl* ctl = a.ctl + lane_id;
  WsCtl* ws = w.ws;
  if (!ws->valid || ws->building || ws->disabled) return true;
  const int tid = threadIdx.x;
  const int K = __builtin_amdgcn_readfirstlane(ws->K);
  const int set = w.set_of[lane_id];
  const double* Gm = w.Gm + (int64_t)set * (WS_KCAP * WS_KCAP);
  {
    const int64_t off = (int64_t)lane_id * a.ld;
    a.beta += off; a.z += off; a.zprev += off; a.gprev += off;
    a.a0 += off; a.b0 += off; a.d0 += off;
    a.pts += ctl->pt_off;
  }
  // A lane whose plain step left W (and W could not be extended) is not refined: resetting those
  // coordinates below would undo its progress.  Neither is a lane that keeps being sent back to the
  // same path point (the model solve did not reach the tolerance, e.g. a near-singular Gram): it
  // finishes the point with plain steps.
  if (ws->stale) {
    double out[1] = {0.0};
    for (int j = tid; j < a.p; j += WS_THREADS)
      if (w.pos[j] < 0 && a.z[j] != a.zprev[j]) out[0] += 1.0;
    block_sum<1>(out, red);
    if (out[0] != 0.0) return true;
  }
  const int point_now = ctl->point + ctl->pt_off;
  // (a point whose refinements keep being sent back because W had to grow -- strongly correlated designs
  // discover their support in waves -- is a different matter from one the model cannot settle)
  const int reps = (ws->last_point[lane_id] == point_now && ws->last_cols[lane_id] == ws->Kreal) ? ws->repeats[lane_id] : 0;
  if (reps >= WS_MAX_REPEATS) return true;
  const int hard_now = w.hard_call ? ws->hard : ws->hard_lane[lane_id];
  if (!DIRECT && w.nt != nullptr && hard_now != 0) {  // a refinement of this lane needed direct steps: so may this one
    if (tid == 0) ws->want_full[lane_id] = 1;
    return false;
  }

  unsigned long long tk_s = wall_clock64();
  const bool keeper = tid == 0 && lane_id == 0;  // WsCtl::solve_ticks: the parts of lane 0's refinements
  const slm_path_point pt = a.pts[ctl->point];
  const int mode = ctl->mode;
  const double tol = ctl->tol;
  const bool g_lds = K <= WS_KLDS;
  if (g_lds) {
    for (int e = tid; e < K * K; e += WS_THREADS) {
      const int r = e / K, cc = e - r * K;
      sh.Gl[e] = Gm[r * WS_KCAP + cc];
    }
  }

  const int tsh = K <= 256 ? 2 : 1;
  const int KP = WS_THREADS >> tsh;
  const int k = tid & (KP - 1), q = tid >> (10 - tsh);
  static_assert(WS_THREADS == 1024, "q = tid >> (10 - tsh)");
  const int j = k < K ? w.idx[k] : -1;
  const bool live = j >= 0;
  const int jj = live ? j : 0;
  const int gix = a.singleton ? jj : a.gid[jj];
  const double x_start = live ? a.z[jj] : 0.0;
  double* ntF = w.nt != nullptr ? w.nt + (int64_t)lane_id * NT_SCRATCH : nullptr;
  const WsThread c = {tid, k, q, K, 1 << tsh, KP, KP >> 6,
                      live, live && q == 0, jj,
                      live ? a.zprev[jj] : 0.0, live ? a.gprev[jj] : 0.0,
                      live ? pt.sa * a.a0[jj] : 0.0, live ? pt.sb * a.b0[gix] : 0.0, live ? pt.sd * a.d0[gix] : 0.0,
                      live ? w.gs[k] : 0, live ? w.gl[k] : 1,
                      (pt.sb != 0.0) || (pt.sd != 0.0), a.singleton != 0, g_lds, Gm, ws, lane_id,
                      ntF, red, sh};
  __syncthreads();  // Gl complete

  ws_tick(keeper, ws->solve_ticks, tk_s, 0);
  double Lw = ws->Lw[set];
  if (!(Lw > 0.0)) {
    Lw = ws_lambda_max(c, w.power_iters);
    if (!(Lw > 0.0)) return true;  // empty / zero Gram: nothing to refine
  }
  ws_tick(keeper, ws->solve_ticks, tk_s, 1);
  ws_tick(keeper, ws->solve_ticks, tk_s, 2);
  WsIterate r;
  const int rc = ws_iterate<GROUPED, DIRECT>(c, w, x_start, Lw, tol, hard_now, r);
  if (rc < 0) return false;
  ws_tick(keeper, ws->solve_ticks, tk_s, 3);
  if (rc == 0) return true;
  if ((!r.settled || r.n_inner == 1) && !ws_no_worse(c, x_start, r.x)) return true;
  ws_write_point(c, a, w, mode, r.x);
  if (tid == 0) {
    if (mode == 1) ctl->have_base = 0;  // the refined point becomes the base of the spectral scheme
    else ctl->t = 1.0;
    ctl->zzero = 0;
    ws->last_point[lane_id] = point_now;
    ws->served[lane_id] = 1;
    ws->repeats[lane_id] = reps + 1;
    ws->last_cols[lane_id] = ws->Kreal;
    // (the lanes of a set end within microseconds of each other: read-compare-write let the smaller of two bounds
    // land last now and then, and the next pass started from a different L -- positive doubles order as integers)
    if (r.L > 0.0) atomicMax(reinterpret_cast<unsigned long long*>(&ws->Lw[set]), (unsigned long long)__double_as_longlong(r.L));
    atomicAdd(&ws->refined, 1);
    atomicAdd(&ws->inner_iters, r.n_inner);
    atomicAdd(&ws->iters_hist[r.n_inner < 31 ? r.n_inner : 31], 1);
    if (r.n_direct) atomicAdd(&ws->newton_steps, r.n_direct - r.n_direct_bad);
    if (r.n_direct > r.n_direct_bad) {
      ws->hard_next = 1;  // (same value from every lane: the order of the stores is immaterial)
      ws->hard_lane[lane_id] = 1;
    }
    if (r.n_direct_bad) atomicAdd(&ws->newton_fails, r.n_direct_bad);
    // strong convexity on the face of the refined point, for the stopping rule of the pass that verifies it
    // (fista_tail_kernel): from the factor when a direct step stood, else from the iteration's own moves
    // (halved: both are estimates from above); 0 = unknown.
    ctl->mu = r.mu_face > 0.0 ? 0.5 * r.mu_face : (r.rq_n >= 3 ? 0.5 * r.rq_min : 0.0);
  }
  ws_tick(keeper, ws->solve_ticks, tk_s, 4);
  return true;
}

// MODE 0: the iteration alone (lanes that would take a direct step are left, untouched, with WsCtl::want_full set);
// MODE 1: the solver with direct steps, for the lanes MODE 0 left -- a launch of its own behind it.  (Round 6 tried both in
// one launch: the idle second launch is 4.8 us of the chain between two passes, but the light instance compiled into one
// kernel with the factorisation was no faster for per-feature penalties and 0.35 ms per pass slower for grouped ones --
// its registers went to scratch memory; tools/ab_knobs.py, profiles/r06_fusion_ab.txt.)
template <bool GROUPED, int MODE>
__global__ __launch_bounds__(WS_THREADS) void ws_solve_kernel(TailArgs a, WsArgs w) {
  __shared__ double red[8][TAIL_WAVES];
  __shared__ WsSolveLds sh;
  const int lane_id = blockIdx.x;
  PathCtl* ctl = a.ctl + lane_id;
  if (ctl->done != 0 || ctl->idle != 0 || a.gdone[0] != 0) return;
  const unsigned long long tk_in = wall_clock64();
  if (MODE == 1) {  // only the lanes the light kernel left
    const int mine = w.ws->want_full[lane_id] | w.one_solver;
    __syncthreads();
    if (!mine) return;
    if (threadIdx.x == 0) w.ws->want_full[lane_id] = 0;
  }
  // (every return inside is taken by the whole workgroup)
  if (MODE == 0) {
    if (!ws_refine_lane<GROUPED, false>(a, w, red, sh)) return;
  } else {
    (void)ws_refine_lane<GROUPED, true>(a, w, red, sh);
  }
  __syncthreads();
  // Is the point the next pass evaluates zero outside W?  Then its residual needs only the gathered
  // columns (resid_ws_kernel) and the pass over X is the accumulate-only xtr_ring_kernel.
  const WsCtl* ws = w.ws;
  const bool w_ok = ws->valid && !ws->building && !ws->disabled;
  double out[1] = {0.0};
  if (w_ok) {
    const double* z = a.z + (int64_t)lane_id * a.ld;
    for (int j0 = threadIdx.x; j0 < a.p; j0 += 8 * WS_THREADS) {
      int ps[8];
      double zj[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = j0 + u * WS_THREADS;
        const int jj = j < a.p ? j : 0;
        ps[u] = j < a.p ? w.pos[jj] : 0;
        zj[u] = z[jj];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (ps[u] < 0 && zj[u] != 0.0) out[0] += 1.0;
    }
  }
  block_sum<1>(out, red);
  if (threadIdx.x == 0) {
    ctl->zsup = (w_ok && out[0] == 0.0) ? 1 : 0;
    w.ws->lane_ticks[lane_id] += wall_clock64() - tk_in;
  }
}

}  // namespace slm
