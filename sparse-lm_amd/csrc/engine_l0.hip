// Host side of the MI355X fit engine, sixth unit: the exact l0 estimators (csrc/l0_kernels.hpp) -- the reference's
// mixed-integer family (reference src/sparselm/model/_miqp/_best_subset.py, _regularized_l0.py), which it hands to
// Gurobi or SCIP through cvxpy.  Here: the dataset's own Gram (engine_cov.hip), the search order, the greedy seed and the
// unconstrained bound on the host (p <= 128: microseconds), ONE launch of the search, and the winner's coefficients
// recomputed in one place from the Gram on its support.
// slm_solve_l0_l1 (the reference's L1L0, _regularized_l0.py:258-410) is the same call in l1 mode: the kernel's L1 instantiation,
// the l0_l1_* functions of l0_host.hpp for seed, winner and the dual bound on all columns.
// slm_solve_l0_profile is the same search in profile mode (the kernel's PROFILE instantiation): the best support of every size
// up to max_groups from one launch, seeded per size by the same greedy selection, each size's coefficients recomputed here.
// slm_solve_l0_wide and slm_solve_l0_profile_wide are the same two calls on the kernel's WIDE instantiations: up to 128 columns
// and groups, masks of two words, a support of at most 64 independent columns (the capacity rule of l0_host.hpp).  One
// template over WIDE serves both widths; with WIDE = false it is the code there was before.
// slm_solve_l0_constrained is the search on the kernel's CON instantiation: rows lo <= A beta <= hi and a per-column box, the
// l0_con_* functions of l0_host.hpp for the seed, the bound on all columns and the winner (solve_l0_con_impl).
// slm_solve_l0_xb and slm_solve_l0_xb_wide are slm_solve_l0 and slm_solve_l0_wide on the kernel's XB instantiations: the subtree
// bound on everything not yet excluded (l0_excl_plan of l0_host.hpp hands over P = H^-1, P c and the margin delta); where H is
// not positive definite on all columns, or delta >= 1/2, they run the plain kernel and say so in info->mode.
#include "engine_internal.hpp"
#include "l0_host.hpp"
#include "l0_kernels.hpp"

namespace {

constexpr long long kL0DefaultNodes = 1ll << 30;  // the budget of a call that names none: at the 6.2e8 nodes/s measured at 25 x 30
                                                  // (profiles/l0_search.txt) a call that exhausts it stays under two seconds

// The argument checks both searches share, before anything touches the device.  alpha_name: what the l0 weight is called in
// the entry's own signature.  Leaves p and the group count.  pmax: L0_PMAX, or L0_WIDE_PMAX for the wide entries (need then
// holds two words per group, the low one first).
int l0_check_args(slm_dataset* ds, const void* out, double alpha, const char* alpha_name, double eta, double eta_l1, double big_M,
                  const double* T, const uint64_t* need, int* p_out, int* ng_out, int pmax = L0_PMAX) {
  if (!ds || !out) return fail(SLM_ERR_BAD_ARG, "NULL argument");
  if (!(alpha >= 0.0) || !std::isfinite(alpha)) return fail(SLM_ERR_BAD_ARG, "%s must be finite and >= 0", alpha_name);
  if (!(eta >= 0.0) || !std::isfinite(eta)) return fail(SLM_ERR_BAD_ARG, "eta must be finite and >= 0");
  if (!(eta_l1 >= 0.0) || !std::isfinite(eta_l1)) return fail(SLM_ERR_BAD_ARG, "eta_l1 must be finite and >= 0");
  if (!(big_M >= 0.0)) return fail(SLM_ERR_BAD_ARG, "big_M must be >= 0");
  const int64_t p64 = ds->p;
  const int ng = ds->singleton ? (int)std::min<int64_t>(p64, pmax + 1) : ds->G;
  if (need && ng <= pmax && pmax == L0_PMAX)
    for (int g = 0; g < ng; ++g)
      if (ng < 64 && (need[g] >> ng) != 0) return fail(SLM_ERR_BAD_ARG, "need[%d] names a group at or beyond n_groups = %d", g, ng);
  if (need && ng <= pmax && pmax != L0_PMAX)
    for (int g = 0; g < ng; ++g) {
      const L0Mask128 mk{need[2 * g], need[2 * g + 1]}, below = l0m_below<L0Mask128>(ng);
      if (l0m_any_outside(mk, below)) return fail(SLM_ERR_BAD_ARG, "need[%d] names a group at or beyond n_groups = %d", g, ng);
    }
  if (T)
    for (int64_t e = 0; e < p64 * p64 && p64 <= pmax; ++e)
      if (!std::isfinite(T[e])) return fail(SLM_ERR_BAD_ARG, "T contains a non-finite value");
  if (p64 > pmax || ng > pmax) {
    if (pmax != L0_PMAX)
      return fail(SLM_ERR_UNSUPPORTED, "the wide exact l0 search takes up to %d columns and %d groups (got %lld, %d)", pmax, pmax,
                  (long long)p64, ng);
    return fail(SLM_ERR_UNSUPPORTED, "the exact l0 search takes up to %d columns and %d groups (got %lld, %d)", L0_PMAX, L0_PMAX,
                (long long)p64, ng);
  }
  if (row_sharded(ds)) return fail(SLM_ERR_UNSUPPORTED, "the exact l0 search is not built for row-sharded datasets");
  *p_out = (int)p64;
  *ng_out = ng;
  return SLM_OK;
}

// What both searches work on: the dataset's Gram on the host, the search order, H = G + 2 eta T and c in that order, the
// hierarchy in that order, and the unconstrained value on all columns.
// (Mask: one word, or the wide mode's two.)
template <class Mask>
struct L0ProblemT {
  std::vector<double> G, cvec, H, c;  // G, cvec: the dataset's order; H, c: search order
  std::vector<int> cols, gstart, gorder;
  std::vector<Mask> needo;
  double q_all = 0.0, yy = 0.0;
};
using L0Problem = L0ProblemT<unsigned long long>;

// need[g] of the caller (the dataset's group order) as a mask
inline unsigned long long l0_need_of(const uint64_t* need, int g, unsigned long long) { return need[g]; }
inline L0Mask128 l0_need_of(const uint64_t* need, int g, L0Mask128) { return L0Mask128{need[2 * g], need[2 * g + 1]}; }

template <class Mask>
int l0_prepare(slm_dataset* ds, int p, int ng, double eta, const double* T, const uint64_t* need, L0ProblemT<Mask>& P) {
  slm_engine* eng = ds->eng;
  HIP_TRY(hipSetDevice(eng->device));
  hipStream_t s = eng->stream;

  // ---- the dataset's own Gram: G = X^T W X / n, c = X^T W y / n (built by the covariance code when it is not there) ------
  SLM_TRY(slm_dataset_covariance(ds, nullptr, 0));
  const double* wdev = ds->rw;
  double fp[2];
  SLM_TRY(cov_fingerprints(ds, &wdev, 1, fp));
  const int entry = cov_find(ds, fp[0], fp[1], (double)ds->n_global);
  if (entry < 0) return fail(SLM_ERR_HIP, "the dataset's Gram was not filed");
  std::vector<double>&G = P.G, &cvec = P.cvec;
  G.assign((size_t)p * p, 0.0);
  cvec.assign((size_t)p, 0.0);
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy2D(G.data(), sizeof(double) * p, ds->cov[(size_t)entry].G, sizeof(double) * ds->ld, sizeof(double) * p, (size_t)p,
                      hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cvec.data(), ds->cov[(size_t)entry].c, sizeof(double) * p, hipMemcpyDeviceToHost));
  for (double v : G)
    if (!std::isfinite(v)) return fail(SLM_ERR_NON_FINITE, "the Gram holds a non-finite value (non-finite data)");
  for (double v : cvec)
    if (!std::isfinite(v)) return fail(SLM_ERR_NON_FINITE, "X^T y holds a non-finite value (non-finite data)");

  // ---- search order: groups by descending ||c_g||^2 / tr G_gg (ties: the lower index), a group's columns contiguous --------
  std::vector<int> gid((size_t)p);
  for (int j = 0; j < p; ++j) gid[(size_t)j] = ds->h_gid.empty() ? j : ds->h_gid[(size_t)j];
  std::vector<double> num((size_t)ng, 0.0), den((size_t)ng, 0.0);
  for (int j = 0; j < p; ++j) {
    num[(size_t)gid[(size_t)j]] += cvec[(size_t)j] * cvec[(size_t)j];
    den[(size_t)gid[(size_t)j]] += G[(size_t)j * p + j];
  }
  std::vector<int>& gorder = P.gorder;
  gorder.assign((size_t)ng, 0);
  std::vector<int> gpos((size_t)ng);
  std::iota(gorder.begin(), gorder.end(), 0);
  auto score = [&](int g) { return den[(size_t)g] > 0.0 ? num[(size_t)g] / den[(size_t)g] : 0.0; };
  std::stable_sort(gorder.begin(), gorder.end(), [&](int x, int y) { return score(x) > score(y); });
  for (int k = 0; k < ng; ++k) gpos[(size_t)gorder[(size_t)k]] = k;
  std::vector<int>& cols = P.cols;  // search position -> column of X
  std::vector<int>& gstart = P.gstart;
  cols.clear();
  gstart.assign((size_t)ng + 1, 0);
  for (int k = 0; k < ng; ++k) {
    for (int j = 0; j < p; ++j)
      if (gid[(size_t)j] == gorder[(size_t)k]) cols.push_back(j);
    gstart[(size_t)k + 1] = (int)cols.size();
  }
  std::vector<double>&H = P.H, &c = P.c;
  H.assign((size_t)p * p, 0.0);
  c.assign((size_t)p, 0.0);
  for (int i = 0; i < p; ++i) {
    c[(size_t)i] = cvec[(size_t)cols[(size_t)i]];
    for (int j = 0; j < p; ++j) {
      const int ci = cols[(size_t)i], cj = cols[(size_t)j];
      // (T symmetrised: only its symmetric part acts in beta^T T beta)
      const double t = T ? 0.5 * (T[(size_t)ci * p + cj] + T[(size_t)cj * p + ci]) : (ci == cj ? 1.0 : 0.0);
      H[(size_t)i * p + j] = G[(size_t)ci * p + cj] + 2.0 * eta * t;
    }
  }
  std::vector<Mask>& needo = P.needo;
  needo.assign((size_t)ng, l0m_none<Mask>());
  if (need)
    for (int g = 0; g < ng; ++g)
      for (int h = 0; h < ng; ++h)
        if (h != g && l0m_test(l0_need_of(need, g, Mask{}), h)) l0m_set(needo[(size_t)gpos[(size_t)g]], gpos[(size_t)h]);

  // ---- the unconstrained value on all columns ------------------------------------------------------------------------------
  P.q_all = l0_q_all(H.data(), c.data(), p);
  P.yy = ds->cov[(size_t)entry].yy;
  return SLM_OK;
}

// The search's one device block: the stream is drained and the block freed however the call ends.
struct L0DevGuard {
  unsigned long long*& p;
  hipStream_t s;
  ~L0DevGuard() {
    (void)hipStreamSynchronize(s);
    dfree(p);
  }
};

// Both entries.  eta_l1 > 0 is l1 mode (the kernel's L1 instantiation, the l0_l1_* functions of l0_host.hpp); eta_l1 == 0 is the
// search without an l1 term, instruction for instruction what it was before there was one.
// WIDE: the kernel's wide instantiation (no l1 mode there), masks of two words in need, support_out and on the device.
// XB: the exclusion bound (never with an l1 term); XB = false is the code there was.  info->mode then says which bound ran:
// 5 the exclusion bound (info->beta_norm = delta), 6 q_all because H is not positive definite on all columns, 7 q_all because
// delta >= 1/2 (info->beta_norm = delta).
template <bool WIDE, bool XB = false>
int solve_l0_impl(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T, double eta_l1, double big_M,
                  const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out, double* lower_bound_out,
                  int64_t* nodes_out, slm_point_info* info) {
  using Mask = std::conditional_t<WIDE, L0Mask128, unsigned long long>;
  constexpr size_t MW = WIDE ? 2 : 1;  // words per mask
  int p = 0, ng = 0;
  SLM_TRY(l0_check_args(ds, beta_out, alpha, "alpha", eta, eta_l1, big_M, T, need, &p, &ng, WIDE ? L0_WIDE_PMAX : L0_PMAX));
  const bool l1 = !WIDE && eta_l1 > 0.0;
  const int K = max_groups < 0 ? 0 : std::min<int>(max_groups, ng);
  // the value (without alpha |S|) and coefficients of one support, as the kernel values a node
  auto value_of = [&](const std::vector<double>& H, const std::vector<double>& c, const std::vector<int>& gstart, Mask mask, bool polish,
                      double* beta) {
    if constexpr (WIDE)
      return l0_support_of(H.data(), c.data(), p, gstart, mask, big_M, polish, beta);
    else
      return l1 ? l0_l1_support(H.data(), c.data(), p, gstart, mask, eta_l1, big_M, polish, beta)
                : l0_support(H.data(), c.data(), p, gstart, mask, big_M, polish, beta);
  };
  L0ProblemT<Mask> P;
  SLM_TRY(l0_prepare(ds, p, ng, eta, T, need, P));
  slm_engine* eng = ds->eng;
  hipStream_t s = eng->stream;
  const std::vector<double>&G = P.G, &cvec = P.cvec, &H = P.H, &c = P.c;
  const std::vector<int>&cols = P.cols, &gstart = P.gstart, &gorder = P.gorder;
  const std::vector<Mask>& needo = P.needo;
  const double q_all = P.q_all;
  [[maybe_unused]] L0ExclPlan plan;
  if constexpr (XB) plan = l0_excl_plan(H.data(), c.data(), p);
  const bool xb = XB && plan.reason == 0;

  // ---- the greedy seed of the incumbent ------------------------------------------------------------------------------------
  std::vector<double> beta_s((size_t)p);
  // the subtree bound's lower bound on the value of all columns: in l1 mode the lasso dual value where it is above q_all
  const double bound = l1 ? l0_l1_lower_bound(H.data(), c.data(), p, P.yy, eta_l1, q_all) : q_all;
  double seed_val = 0.0;  // the empty support
  Mask seed_mask = l0m_none<Mask>();
  l0_greedy(H.data(), c.data(), p, gstart, needo, K, [&](Mask mask) { return value_of(H, c, gstart, mask, false, beta_s.data()); },
            [&](int size, Mask mask, double quad) {
              const double v = quad + alpha * (double)size;
              if (v < seed_val) {
                seed_val = v;
                seed_mask = mask;
              }
            });

  // ---- the search: one launch --------------------------------------------------------------------------------------------
  const int d = std::min(ng, L0_PREFIX);
  const long long n_tickets = 1ll << d;
  const int blocks = (int)std::max<long long>(1, std::min<long long>(2ll * eng->cus, (n_tickets + L0_WAVES - 1) / L0_WAVES));
  const int waves = blocks * L0_WAVES;
  // one block of 8-byte words: control | best values | best supports | H | c | need | group starts (a mask: MW words)
  // | exclusion bound: P | P c
  const size_t off_bv = L0_CTL_WORDS, off_bm = off_bv + (size_t)waves, off_H = off_bm + MW * (size_t)waves, off_c = off_H + (size_t)p * p,
               off_need = off_c + (size_t)p, off_gs = off_need + MW * (size_t)ng, off_P = off_gs + (size_t)ng + 1,
               off_bh = off_P + (xb ? (size_t)p * p : 0), words = off_bh + (xb ? (size_t)p : 0);
  std::vector<unsigned long long> h(words, 0ull);
  if (xb) {
    memcpy(&h[off_P], plan.P.data(), sizeof(double) * (size_t)p * p);
    memcpy(&h[off_bh], plan.bhat.data(), sizeof(double) * (size_t)p);
  }
  h[L0_INCUMBENT] = l0_key(seed_val);
  if constexpr (WIDE) h[L0_CAPACITY] = ~0ull;  // (lowered by a wave that refused an include for capacity)
  memcpy(&h[off_H], H.data(), sizeof(double) * (size_t)p * p);
  memcpy(&h[off_c], c.data(), sizeof(double) * (size_t)p);
  static_assert(sizeof(Mask) == MW * sizeof(unsigned long long), "a mask is MW words, the low one first");
  if (ng > 0) memcpy(&h[off_need], needo.data(), sizeof(Mask) * (size_t)ng);
  for (int g = 0; g <= ng; ++g) h[off_gs + (size_t)g] = (unsigned long long)gstart[(size_t)g];
  unsigned long long* dev = nullptr;
  SLM_TRY(dalloc(&dev, words));
  L0DevGuard guard{dev, s};
  HIP_TRY(hipMemcpyAsync(dev, h.data(), sizeof(unsigned long long) * words, hipMemcpyHostToDevice, s));
  L0Args k;
  memset(&k, 0, sizeof(k));
  k.ctl = dev;
  k.best_val = reinterpret_cast<double*>(dev + off_bv);
  k.best_mask = dev + off_bm;
  k.H = reinterpret_cast<const double*>(dev + off_H);
  k.c = reinterpret_cast<const double*>(dev + off_c);
  k.need = dev + off_need;
  k.gstart = reinterpret_cast<const long long*>(dev + off_gs);
  k.p = p; k.ng = ng; k.d = d; k.K = K;
  k.alpha = alpha; k.big_M = big_M; k.q_all = bound;
  k.eta_l1 = eta_l1;
  k.max_nodes = max_nodes > 0 ? max_nodes : kL0DefaultNodes;
  if (xb) {
    if constexpr (XB) {
      k.P = reinterpret_cast<const double*>(dev + off_P);
      k.bhat = reinterpret_cast<const double*>(dev + off_bh);
      k.xb_delta = plan.delta;
      hipLaunchKernelGGL((l0_search_kernel<false, false, WIDE, false, true>), dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, k);
    }
  } else if constexpr (WIDE)
    hipLaunchKernelGGL((l0_search_kernel<false, false, true>), dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, k);
  else if (l1)
    hipLaunchKernelGGL(l0_search_kernel<true>, dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, k);
  else
    hipLaunchKernelGGL(l0_search_kernel<false>, dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, k);
  SLM_TRY(check_launch());
  HIP_TRY(hipMemcpyAsync(h.data(), dev, sizeof(unsigned long long) * off_H, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));

  // ---- the winner: the waves' bests and the seed in a fixed order, the lower support on a bitwise tie -------------------------
  double win_val = seed_val;
  Mask win_mask = seed_mask;
  for (int wv = 0; wv < waves; ++wv) {
    double v;
    memcpy(&v, &h[off_bv + (size_t)wv], 8);
    Mask mk;
    memcpy(&mk, &h[off_bm + MW * (size_t)wv], sizeof(Mask));
    if (v < win_val || (v == win_val && l0m_less(mk, win_mask))) {
      win_val = v;
      win_mask = mk;
    }
  }
  const bool finished = h[L0_ABORTED] == 0;
  // its coefficients, recomputed here whichever wave found it
  const double quad = value_of(H, c, gstart, win_mask, true, beta_s.data());
  int n_active = 0;
  Mask support = l0m_none<Mask>();
  for (int g = 0; g < ng; ++g)
    if (l0m_test(win_mask, g)) {
      ++n_active;
      l0m_set(support, gorder[(size_t)g]);
    }
  const double objective = quad + alpha * (double)n_active;
  for (int i = 0; i < p; ++i) beta_out[cols[(size_t)i]] = beta_s[(size_t)i];
  if (support_out) memcpy(support_out, &support, sizeof(Mask));
  // wide: c_min + 1 of the capacity rule (l0_host.hpp), 0 when no include was refused because the factor was full
  const int cut = WIDE && h[L0_CAPACITY] != ~0ull ? (int)h[L0_CAPACITY] : 0;
  const bool proven = finished && l0_capacity_proven(objective, q_all, alpha, cut);
  double lower = finished ? objective : std::min(objective, bound);
  if (cut) lower = std::min(lower, l0_capacity_bound(q_all, alpha, cut));
  if (lower_bound_out) *lower_bound_out = lower;
  if (nodes_out) *nodes_out = (int64_t)h[L0_NODES];
  if (info) {
    // 1/(2n)||X beta - y||_W^2 = 1/2 beta^T G beta - c^T beta + 1/2 y^T W y / n from the Gram already on the host: no second launch
    double loss = 0.5 * P.yy;
    for (int i = 0; i < p; ++i) {
      if (beta_out[i] == 0.0) continue;
      double t = 0.0;
      for (int j = 0; j < p; ++j) t += G[(size_t)i * p + j] * beta_out[j];
      loss += beta_out[i] * (0.5 * t - cvec[(size_t)i]);
    }
    memset(info, 0, sizeof(*info));
    info->n_iter = 1;
    info->status = proven ? SLM_OK : SLM_ERR_NOT_CONVERGED;
    info->loss = loss;
    info->mode = 4;
    info->kkt = objective;
    info->mu = seed_val;
    info->L = bound;
    info->rejects = (int32_t)std::min<unsigned long long>(h[L0_DESCENTS], 0x7fffffffull);  // (l1 mode: descents run)
    if constexpr (WIDE) {
      info->rejects = cut;                   // (c_min + 1, or 0)
      info->resid = finished ? 0.0 : 1.0;  // (1: the node budget ran out -- what tells it from a result unproven for capacity alone)
    }
    double bn = 0.0;
    for (int j = 0; j < p; ++j) bn += beta_out[j] * beta_out[j];
    info->beta_norm = std::sqrt(bn);
    if constexpr (XB) {  // which bound ran, and its margin
      info->mode = plan.reason == 0 ? 5 : (plan.reason == 1 ? 6 : 7);
      info->beta_norm = plan.delta;
    }
  }
  if (!finished) return fail(SLM_ERR_NOT_CONVERGED, "the node budget (%lld) ran out before the search finished: the incumbent is returned",
                             (long long)k.max_nodes);
  if (!proven)
    return fail(SLM_ERR_NOT_CONVERGED, "a support holds at most %d independent columns: includes were refused from %d groups on, and the "
                "incumbent is above the bound %.17g on what lies behind them", L0_PMAX, cut - 1, l0_capacity_bound(q_all, alpha, cut));
  return SLM_OK;
}

// slm_solve_l0_profile: the kernel's PROFILE instantiation.  Seeds per size from the greedy selection, one launch, then per size
// the minimum over the waves' bests and the seed in a fixed order and the coefficients recomputed from H on that support.
// WIDE: the kernel's wide profile instantiation; lane k - 1 still holds size k, and no include may be refused for capacity, so
// a call whose max_groups largest groups could hold more than L0_PMAX columns is refused before anything is launched.
template <bool WIDE>
int solve_l0_profile_impl(slm_dataset* ds, double alpha_min, int32_t max_groups, double eta, const double* T, double big_M,
                          const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out, double* value_out,
                          int64_t* nodes_out, slm_point_info* info) {
  using Mask = std::conditional_t<WIDE, L0Mask128, unsigned long long>;
  constexpr size_t MW = WIDE ? 2 : 1;  // words per mask
  int p = 0, ng = 0;
  if (!support_out || !value_out) return fail(SLM_ERR_BAD_ARG, "NULL argument");
  SLM_TRY(l0_check_args(ds, beta_out, alpha_min, "alpha_min", eta, 0.0, big_M, T, need, &p, &ng, WIDE ? L0_WIDE_PMAX : L0_PMAX));
  const int rows = max_groups < 0 ? 0 : (int)max_groups;  // the outputs have rows + 1 entries; sizes above the group count stay unfilled
  const int K = std::min(rows, ng);
  if constexpr (WIDE) {
    if (K > L0_PMAX)
      return fail(SLM_ERR_UNSUPPORTED, "the wide l0 profile keeps one size per lane: max_groups up to %d (got %d)", L0_PMAX, K);
    std::vector<int> width((size_t)ng, 0);
    for (int j = 0; j < p; ++j) ++width[(size_t)(ds->h_gid.empty() ? j : ds->h_gid[(size_t)j])];
    std::sort(width.begin(), width.end(), [](int x, int y) { return x > y; });
    int most = 0;
    for (int k = 0; k < K; ++k) most += width[(size_t)k];
    if (most > L0_PMAX)
      return fail(SLM_ERR_UNSUPPORTED, "the wide l0 profile needs every support to fit the factor: the %d largest groups hold %d columns, "
                  "more than %d", K, most, L0_PMAX);
  }
  L0ProblemT<Mask> P;
  SLM_TRY(l0_prepare(ds, p, ng, eta, T, need, P));
  slm_engine* eng = ds->eng;
  hipStream_t s = eng->stream;
  const std::vector<double>&H = P.H, &c = P.c;

  // ---- the seed of every size: the supports the greedy selection passes through, valued as the kernel values a node ---------
  std::vector<double> beta_s((size_t)p);
  std::vector<double> win_val((size_t)L0_PMAX + 1, HUGE_VAL);
  std::vector<Mask> win_mask((size_t)L0_PMAX + 1, l0m_ones<Mask>());
  win_val[0] = 0.0;  // the empty support
  win_mask[0] = l0m_none<Mask>();
  l0_greedy(H.data(), c.data(), p, P.gstart, P.needo, K,
            [&](Mask mask) { return l0_support_of(H.data(), c.data(), p, P.gstart, mask, big_M, false, beta_s.data()); },
            [&](int size, Mask mask, double quad) {
              if (quad < win_val[(size_t)size] || (quad == win_val[(size_t)size] && l0m_less(mask, win_mask[(size_t)size]))) {
                win_val[(size_t)size] = quad;
                win_mask[(size_t)size] = mask;
              }
            });

  // ---- the search: one launch --------------------------------------------------------------------------------------------
  const int d = std::min(ng, L0_PREFIX);
  const long long n_tickets = 1ll << d;
  const int blocks = (int)std::max<long long>(1, std::min<long long>(2ll * eng->cus, (n_tickets + L0_WAVES - 1) / L0_WAVES));
  const int waves = blocks * L0_WAVES;
  // one block of 8-byte words: control | incumbents per size | best values [waves][64] | best supports [waves][64] | H | c | need | group starts
  // (a mask: MW words)
  const size_t off_bv = L0_PROFILE_WORDS, off_bm = off_bv + (size_t)waves * 64, off_H = off_bm + MW * (size_t)waves * 64,
               off_c = off_H + (size_t)p * p, off_need = off_c + (size_t)p, off_gs = off_need + MW * (size_t)ng, words = off_gs + (size_t)ng + 1;
  std::vector<unsigned long long> h(words, 0ull);
  for (int k = 1; k <= L0_PMAX; ++k) h[(size_t)L0_PROFILE_INC + (size_t)k - 1] = l0_key(win_val[(size_t)k]);
  memcpy(&h[off_H], H.data(), sizeof(double) * (size_t)p * p);
  memcpy(&h[off_c], c.data(), sizeof(double) * (size_t)p);
  if constexpr (WIDE) h[L0_CAPACITY] = ~0ull;
  static_assert(sizeof(Mask) == MW * sizeof(unsigned long long), "a mask is MW words, the low one first");
  if (ng > 0) memcpy(&h[off_need], P.needo.data(), sizeof(Mask) * (size_t)ng);
  for (int g = 0; g <= ng; ++g) h[off_gs + (size_t)g] = (unsigned long long)P.gstart[(size_t)g];
  unsigned long long* dev = nullptr;
  SLM_TRY(dalloc(&dev, words));
  L0DevGuard guard{dev, s};
  HIP_TRY(hipMemcpyAsync(dev, h.data(), sizeof(unsigned long long) * words, hipMemcpyHostToDevice, s));
  L0Args k;
  memset(&k, 0, sizeof(k));
  k.ctl = dev;
  k.best_val = reinterpret_cast<double*>(dev + off_bv);
  k.best_mask = dev + off_bm;
  k.H = reinterpret_cast<const double*>(dev + off_H);
  k.c = reinterpret_cast<const double*>(dev + off_c);
  k.need = dev + off_need;
  k.gstart = reinterpret_cast<const long long*>(dev + off_gs);
  k.p = p; k.ng = ng; k.d = d; k.K = K;
  k.alpha = alpha_min; k.big_M = big_M; k.q_all = P.q_all;
  k.max_nodes = max_nodes > 0 ? max_nodes : kL0DefaultNodes;
  hipLaunchKernelGGL((l0_search_kernel<false, true, WIDE>), dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, k);
  SLM_TRY(check_launch());
  HIP_TRY(hipMemcpyAsync(h.data(), dev, sizeof(unsigned long long) * off_H, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));

  // ---- per size: the waves' bests and the seed in a fixed order, the lower support on a bitwise tie ---------------------------
  for (int size = 1; size <= K; ++size)
    for (int wv = 0; wv < waves; ++wv) {
      double v;
      memcpy(&v, &h[off_bv + (size_t)wv * 64 + (size_t)size - 1], 8);
      Mask mk;
      memcpy(&mk, &h[off_bm + MW * ((size_t)wv * 64 + (size_t)size - 1)], sizeof(Mask));
      if (v < win_val[(size_t)size] || (v == win_val[(size_t)size] && l0m_less(mk, win_mask[(size_t)size]))) {
        win_val[(size_t)size] = v;
        win_mask[(size_t)size] = mk;
      }
    }
  const bool finished = h[L0_ABORTED] == 0;
  if (WIDE && h[L0_CAPACITY] != ~0ull) return fail(SLM_ERR_HIP, "the wide l0 profile refused an include for capacity (internal error)");
  // the coefficients of every size, recomputed here whichever wave found its support; a size nobody filled: +inf, all ones, zeros
  for (int size = 0; size <= rows; ++size) {
    double* beta = beta_out + (size_t)size * p;
    for (int i = 0; i < p; ++i) beta[i] = 0.0;
    const bool filled = size <= K && std::isfinite(win_val[(size_t)size]);
    value_out[size] = HUGE_VAL;
    Mask support = l0m_ones<Mask>();
    memcpy(support_out + MW * (size_t)size, &support, sizeof(Mask));
    if (!filled) continue;
    value_out[size] = l0_support_of(H.data(), c.data(), p, P.gstart, win_mask[(size_t)size], big_M, true, beta_s.data());
    support = l0m_none<Mask>();
    for (int g = 0; g < ng; ++g)
      if (l0m_test(win_mask[(size_t)size], g)) l0m_set(support, P.gorder[(size_t)g]);
    memcpy(support_out + MW * (size_t)size, &support, sizeof(Mask));
    for (int i = 0; i < p; ++i) beta[P.cols[(size_t)i]] = beta_s[(size_t)i];
  }
  if (nodes_out) *nodes_out = (int64_t)h[L0_NODES];
  if (info) {
    memset(info, 0, sizeof(*info));
    info->n_iter = 1;
    info->status = finished ? SLM_OK : SLM_ERR_NOT_CONVERGED;
    info->mode = 4;
    const int at = l0_profile_regularized(value_out, K, alpha_min), sub = l0_profile_best_subset(value_out, K);
    info->kkt = value_out[at] + alpha_min * (double)at;  // the regularised optimum at alpha_min, the smallest alpha the table serves
    info->mu = value_out[sub];                           // the best-subset optimum at the bound max_groups
    info->L = P.q_all;
  }
  if (!finished) return fail(SLM_ERR_NOT_CONVERGED, "the node budget (%lld) ran out before the search finished: the table of incumbents is returned",
                             (long long)k.max_nodes);
  return SLM_OK;
}

// slm_solve_l0_constrained: the kernel's CON instantiation (DESIGN 4d "Constrained mode").  The arguments are checked before
// anything is launched; H must be positive definite on all columns; the rows are scaled to unit norm and everything is put in
// search order; the seed, the bound F_lb on all columns and the winner come from l0_con_solve / l0_con_polish of l0_host.hpp,
// the very splitting the kernel runs.
int solve_l0_con_impl(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T, double big_M, const uint64_t* need,
                      int64_t max_nodes, const double* A, int32_t m, const double* lo, const double* hi, const double* box_lo,
                      const double* box_hi, int32_t max_qp_sweeps, double* beta_out, uint64_t* support_out, double* lower_bound_out,
                      int64_t* nodes_out, double* lambda_out, slm_point_info* info) {
  using Mask = unsigned long long;
  int p = 0, ng = 0;
  SLM_TRY(l0_check_args(ds, beta_out, alpha, "alpha", eta, 0.0, big_M, T, need, &p, &ng, L0_PMAX));
  if (m < 0) return fail(SLM_ERR_BAD_ARG, "m must be >= 0");
  if (m > 0 && (!A || !lo || !hi)) return fail(SLM_ERR_BAD_ARG, "NULL argument (A, lo, hi with m > 0)");
  for (int64_t e = 0; e < (int64_t)m * p; ++e)
    if (!std::isfinite(A[e])) return fail(SLM_ERR_BAD_ARG, "A contains a NaN or an infinity");
  for (int i = 0; i < m; ++i) {
    if (std::isnan(lo[i]) || std::isnan(hi[i])) return fail(SLM_ERR_BAD_ARG, "a bound of row %d is NaN", i);
    if (lo[i] > hi[i]) return fail(SLM_ERR_BAD_ARG, "lo > hi in row %d", i);
  }
  for (int j = 0; j < p; ++j) {
    if (box_lo && !(box_lo[j] <= 0.0))
      return fail(SLM_ERR_BAD_ARG, "box_lo[%d] must be <= 0 (a column whose interval excludes 0 is forced active: that is a row of A)", j);
    if (box_hi && !(box_hi[j] >= 0.0))
      return fail(SLM_ERR_BAD_ARG, "box_hi[%d] must be >= 0 (a column whose interval excludes 0 is forced active: that is a row of A)", j);
  }
  if (m > L0_CON_MMAX) return fail(SLM_ERR_UNSUPPORTED, "the constrained exact l0 search takes up to %d rows of A (got %d)", L0_CON_MMAX, m);
  const int K = max_groups < 0 ? 0 : std::min<int>(max_groups, ng);
  L0Problem P;
  SLM_TRY(l0_prepare(ds, p, ng, eta, T, need, P));
  slm_engine* eng = ds->eng;
  hipStream_t s = eng->stream;
  const std::vector<double>&H = P.H, &c = P.c;
  const std::vector<int>&cols = P.cols, &gstart = P.gstart, &gorder = P.gorder;
  if (!l0_con_pd(H.data(), c.data(), p))
    return fail(SLM_ERR_UNSUPPORTED, "constraints need a positive definite G + 2 eta T: a column depends on the others -- use eta > 0 (L2L0, "
                "RidgedBestSubsetSelection) or a design of full column rank");

  // ---- the constraints in search order: rows of unit norm, the box inside +-big_M ---------------------------------------------
  std::vector<double> As((size_t)m * p), At((size_t)m * p), los((size_t)m), his((size_t)m), rnorm((size_t)m, 1.0), blo((size_t)p), bhi((size_t)p);
  for (int i = 0; i < m; ++i) {
    double nn = 0.0;
    for (int j = 0; j < p; ++j) nn += A[(size_t)i * p + j] * A[(size_t)i * p + j];
    if (nn > 0.0) rnorm[(size_t)i] = std::sqrt(nn);
    for (int k = 0; k < p; ++k) {
      As[(size_t)i * p + k] = A[(size_t)i * p + cols[(size_t)k]] / rnorm[(size_t)i];
      At[(size_t)k * m + i] = As[(size_t)i * p + k];
    }
    los[(size_t)i] = lo[i] / rnorm[(size_t)i];
    his[(size_t)i] = hi[i] / rnorm[(size_t)i];
  }
  for (int k = 0; k < p; ++k) {
    blo[(size_t)k] = box_lo ? std::max(box_lo[cols[(size_t)k]], -big_M) : -big_M;
    bhi[(size_t)k] = box_hi ? std::min(box_hi[cols[(size_t)k]], big_M) : big_M;
  }
  L0ConProblem CP;
  CP.H = H.data(); CP.c = c.data(); CP.p = p;
  CP.A = As.data(); CP.m = m; CP.lo = los.data(); CP.hi = his.data();
  CP.blo = blo.data(); CP.bhi = bhi.data();
  CP.rho = l0_con_rho(H.data(), p, As.data(), m);
  CP.max_sweeps = L0_CON_SWEEPS;  // (the host's own solves -- seed, bound, winner -- always get the full cap: max_qp_sweeps starves the candidates on chip)

  // ---- F_lb, the subtree bound's proven lower bound on f(all columns); and what no feasible support's objective exceeds ------------
  L0ConPoint all;
  const double bound = l0_con_lower_bound(CP, P.q_all, &all);
  double cap = l0_con_value_cap(H.data(), c.data(), p, blo.data(), bhi.data());
  cap = cap + alpha * (double)K + 1e-9 * (cap + alpha * (double)K) + 1e-300;

  // ---- the seed: the empty support, the greedy supports, and supports of the largest groups of the all-columns solution ----------
  int scols[L0_PMAX];
  auto value_of = [&](Mask mask) {
    const int ms = l0_con_columns(gstart, mask, scols);
    const L0ConPoint R = l0_con_solve(CP, scols, ms, HUGE_VAL);
    return R.outcome == 0 ? R.primal : HUGE_VAL;
  };
  bool zero_ok = true;
  for (int i = 0; i < m; ++i) zero_ok = zero_ok && lo[i] <= 0.0 && hi[i] >= 0.0;
  double seed_val = zero_ok ? 0.0 : HUGE_VAL;
  Mask seed_mask = zero_ok ? 0ull : ~0ull;
  auto offer = [&](int size, Mask mask, double quad) {
    const double v = quad + alpha * (double)size;
    if (v < seed_val || (v == seed_val && v < HUGE_VAL && mask < seed_mask)) {
      seed_val = v;
      seed_mask = mask;
    }
  };
  l0_greedy(H.data(), c.data(), p, gstart, P.needo, K, value_of, offer);
  {
    std::vector<double> gnorm((size_t)ng, 0.0);
    for (int g = 0; g < ng; ++g)
      for (int j = gstart[(size_t)g]; j < gstart[(size_t)g + 1] && (size_t)j < all.beta.size(); ++j) gnorm[(size_t)g] += all.beta[(size_t)j] * all.beta[(size_t)j];
    std::vector<int> by((size_t)ng);
    std::iota(by.begin(), by.end(), 0);
    std::stable_sort(by.begin(), by.end(), [&](int x, int y) { return gnorm[(size_t)x] > gnorm[(size_t)y]; });
    Mask cur = 0ull, last = 0ull;
    for (int k = 0; k < ng; ++k) {
      cur |= 1ull << by[(size_t)k];
      for (bool grew = true; grew;) {  // closed under the hierarchy
        grew = false;
        for (int g = 0; g < ng; ++g)
          if (((cur >> g) & 1) && (P.needo[(size_t)g] & ~cur)) {
            cur |= P.needo[(size_t)g];
            grew = true;
          }
      }
      const int size = __builtin_popcountll(cur);
      if (size > K) break;
      if (cur != last) offer(size, cur, value_of(cur));
      last = cur;
    }
  }

  // ---- the search: one launch --------------------------------------------------------------------------------------------
  const int d = std::min(ng, L0_PREFIX);
  const long long n_tickets = 1ll << d;
  const int blocks = (int)std::max<long long>(1, std::min<long long>(2ll * eng->cus, (n_tickets + L0_WAVES - 1) / L0_WAVES));
  const int waves = blocks * L0_WAVES;
  // one block of 8-byte words: control | best values | best supports | H | c | need | group starts | A by columns | lo | hi | box
  const size_t off_bv = L0_CTL_WORDS, off_bm = off_bv + (size_t)waves, off_H = off_bm + (size_t)waves, off_c = off_H + (size_t)p * p,
               off_need = off_c + (size_t)p, off_gs = off_need + (size_t)ng, off_A = off_gs + (size_t)ng + 1, off_lo = off_A + (size_t)m * p,
               off_hi = off_lo + (size_t)m, off_blo = off_hi + (size_t)m, off_bhi = off_blo + (size_t)p, words = off_bhi + (size_t)p;
  std::vector<unsigned long long> h(words, 0ull);
  h[L0_INCUMBENT] = l0_key(std::min(seed_val, cap));
  h[L0_UNSETTLED] = ~0ull;  // (lowered by a wave whose candidate ran out of sweeps)
  memcpy(&h[off_H], H.data(), sizeof(double) * (size_t)p * p);
  memcpy(&h[off_c], c.data(), sizeof(double) * (size_t)p);
  if (ng > 0) memcpy(&h[off_need], P.needo.data(), sizeof(Mask) * (size_t)ng);
  for (int g = 0; g <= ng; ++g) h[off_gs + (size_t)g] = (unsigned long long)gstart[(size_t)g];
  if (m > 0) {
    memcpy(&h[off_A], At.data(), sizeof(double) * (size_t)m * p);
    memcpy(&h[off_lo], los.data(), sizeof(double) * (size_t)m);
    memcpy(&h[off_hi], his.data(), sizeof(double) * (size_t)m);
  }
  memcpy(&h[off_blo], blo.data(), sizeof(double) * (size_t)p);
  memcpy(&h[off_bhi], bhi.data(), sizeof(double) * (size_t)p);
  unsigned long long* dev = nullptr;
  SLM_TRY(dalloc(&dev, words));
  L0DevGuard guard{dev, s};
  HIP_TRY(hipMemcpyAsync(dev, h.data(), sizeof(unsigned long long) * words, hipMemcpyHostToDevice, s));
  L0Args k;
  memset(&k, 0, sizeof(k));
  k.ctl = dev;
  k.best_val = reinterpret_cast<double*>(dev + off_bv);
  k.best_mask = dev + off_bm;
  k.H = reinterpret_cast<const double*>(dev + off_H);
  k.c = reinterpret_cast<const double*>(dev + off_c);
  k.need = dev + off_need;
  k.gstart = reinterpret_cast<const long long*>(dev + off_gs);
  k.A = reinterpret_cast<const double*>(dev + off_A);
  k.lo = reinterpret_cast<const double*>(dev + off_lo);
  k.hi = reinterpret_cast<const double*>(dev + off_hi);
  k.blo = reinterpret_cast<const double*>(dev + off_blo);
  k.bhi = reinterpret_cast<const double*>(dev + off_bhi);
  k.rows = m; k.con_sweeps = max_qp_sweeps > 0 ? max_qp_sweeps : L0_CON_SWEEPS; k.rho = CP.rho;
  k.p = p; k.ng = ng; k.d = d; k.K = K;
  k.alpha = alpha; k.big_M = big_M; k.q_all = bound;
  k.max_nodes = max_nodes > 0 ? max_nodes : kL0DefaultNodes;
  hipLaunchKernelGGL((l0_search_kernel<false, false, false, true>), dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, k);
  SLM_TRY(check_launch());
  HIP_TRY(hipMemcpyAsync(h.data(), dev, sizeof(unsigned long long) * off_H, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));

  // ---- the winner: the waves' bests and the seed in a fixed order, the lower support on a bitwise tie -------------------------
  double win_val = seed_val;
  Mask win_mask = seed_mask;
  for (int wv = 0; wv < waves; ++wv) {
    double v;
    memcpy(&v, &h[off_bv + (size_t)wv], 8);
    const Mask mk = h[off_bm + (size_t)wv];
    if (v < win_val || (v == win_val && v < HUGE_VAL && mk < win_mask)) {
      win_val = v;
      win_mask = mk;
    }
  }
  const bool finished = h[L0_ABORTED] == 0;
  const long long n_unsettled = (long long)h[L0_UNSETTLED_COUNT];
  const double unsettled_bound = h[L0_UNSETTLED] == ~0ull ? HUGE_VAL : l0_unkey(h[L0_UNSETTLED]);
  if (nodes_out) *nodes_out = (int64_t)h[L0_NODES];
  for (int i = 0; i < p; ++i) beta_out[i] = 0.0;
  for (int i = 0; i < m && lambda_out; ++i) lambda_out[i] = 0.0;
  if (support_out) *support_out = 0;
  if (!(win_val < HUGE_VAL) && finished && n_unsettled == 0)
    return fail(SLM_ERR_BAD_ARG, "no admissible support satisfies the constraints (%d groups at most, the hierarchy, %d rows and the box)", K, m);
  // its coefficients and multipliers, recomputed here whichever wave found it: the splitting, then the exact face solve
  double objective = HUGE_VAL;
  int n_active = 0;
  if (win_val < HUGE_VAL) {
    const int ms = l0_con_columns(gstart, win_mask, scols);
    L0ConPoint R = l0_con_solve(CP, scols, ms, HUGE_VAL);
    (void)l0_con_polish(CP, scols, ms, R);
    Mask support = 0ull;
    for (int g = 0; g < ng; ++g)
      if ((win_mask >> g) & 1) {
        ++n_active;
        support |= 1ull << gorder[(size_t)g];
      }
    objective = R.primal + alpha * (double)n_active;
    for (int r = 0; r < ms; ++r) beta_out[cols[(size_t)scols[r]]] = R.beta[(size_t)r];
    for (int i = 0; i < m && lambda_out; ++i) lambda_out[i] = R.y[(size_t)i] / rnorm[(size_t)i];
    if (support_out) *support_out = support;
  }
  const bool proven = finished && objective <= unsettled_bound && objective < HUGE_VAL;
  double lower = std::min(objective, unsettled_bound);
  if (!finished) lower = std::min(lower, bound);
  if (lower_bound_out) *lower_bound_out = lower;
  if (info) {
    double loss = 0.5 * P.yy;
    for (int i = 0; i < p; ++i) {
      if (beta_out[i] == 0.0) continue;
      double t = 0.0;
      for (int j = 0; j < p; ++j) t += P.G[(size_t)i * p + j] * beta_out[j];
      loss += beta_out[i] * (0.5 * t - P.cvec[(size_t)i]);
    }
    memset(info, 0, sizeof(*info));
    info->n_iter = 1;
    info->status = proven ? SLM_OK : SLM_ERR_NOT_CONVERGED;
    info->loss = loss;
    info->mode = 4;
    info->kkt = objective;
    info->mu = seed_val;
    info->L = bound;
    info->rejects = (int32_t)std::min<unsigned long long>(h[L0_DESCENTS], 0x7fffffffull);  // candidates valued
    info->resid = (double)n_unsettled;                                                    // candidates that ran out of sweeps
    info->beta_norm = unsettled_bound;                                                    // the lowest of their bounds, +inf: none
  }
  if (!finished) return fail(SLM_ERR_NOT_CONVERGED, "the node budget (%lld) ran out before the search finished: the incumbent is returned",
                             (long long)k.max_nodes);
  if (!proven)
    return fail(SLM_ERR_NOT_CONVERGED, "%lld candidate(s) ran out of sweeps (%d each): the incumbent is above the bound %.17g on them",
                n_unsettled, k.con_sweeps, unsettled_bound);
  return SLM_OK;
}

}  // namespace

extern "C" int slm_solve_l0(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T, double big_M,
                            const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out,
                            double* lower_bound_out, int64_t* nodes_out, slm_point_info* info) {
  return solve_l0_impl<false>(ds, alpha, max_groups, eta, T, 0.0, big_M, need, max_nodes, beta_out, support_out, lower_bound_out, nodes_out, info);
}

// The same search on the kernel's wide instantiation: up to 128 columns and groups, masks of two words (the low one first).
extern "C" int slm_solve_l0_wide(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T, double big_M,
                                 const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out,
                                 double* lower_bound_out, int64_t* nodes_out, slm_point_info* info) {
  return solve_l0_impl<true>(ds, alpha, max_groups, eta, T, 0.0, big_M, need, max_nodes, beta_out, support_out, lower_bound_out, nodes_out, info);
}

// slm_solve_l0 and slm_solve_l0_wide with the exclusion bound (the kernel's XB instantiations): the same signature, contract and
// result; info->mode tells which bound ran (5: exclusion, 6 / 7: q_all) and info->beta_norm holds the margin delta.
extern "C" int slm_solve_l0_xb(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T, double big_M,
                               const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out,
                               double* lower_bound_out, int64_t* nodes_out, slm_point_info* info) {
  return solve_l0_impl<false, true>(ds, alpha, max_groups, eta, T, 0.0, big_M, need, max_nodes, beta_out, support_out, lower_bound_out, nodes_out,
                                    info);
}

extern "C" int slm_solve_l0_xb_wide(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T, double big_M,
                                    const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out,
                                    double* lower_bound_out, int64_t* nodes_out, slm_point_info* info) {
  return solve_l0_impl<true, true>(ds, alpha, max_groups, eta, T, 0.0, big_M, need, max_nodes, beta_out, support_out, lower_bound_out, nodes_out,
                                   info);
}

// The reference's L1L0 (_regularized_l0.py:258-410): no cardinality bound, no ridge term, eta_l1 ||beta||_1.
extern "C" int slm_solve_l0_l1(slm_dataset* ds, double alpha, double eta_l1, double big_M, const uint64_t* need, int64_t max_nodes,
                               double* beta_out, uint64_t* support_out, double* lower_bound_out, int64_t* nodes_out,
                               slm_point_info* info) {
  return solve_l0_impl<false>(ds, alpha, L0_PMAX, 0.0, nullptr, eta_l1, big_M, need, max_nodes, beta_out, support_out, lower_bound_out, nodes_out,
                       info);
}

// The table of the best supports of every size up to max_groups, from one search (the kernel's profile mode).
extern "C" int slm_solve_l0_profile(slm_dataset* ds, double alpha_min, int32_t max_groups, double eta, const double* T, double big_M,
                                    const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out, double* value_out,
                                    int64_t* nodes_out, slm_point_info* info) {
  return solve_l0_profile_impl<false>(ds, alpha_min, max_groups, eta, T, big_M, need, max_nodes, beta_out, support_out, value_out, nodes_out, info);
}

// The profile on the kernel's wide instantiation: masks of two words in need and support_out, max_groups up to 64.
extern "C" int slm_solve_l0_profile_wide(slm_dataset* ds, double alpha_min, int32_t max_groups, double eta, const double* T, double big_M,
                                         const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out,
                                         double* value_out, int64_t* nodes_out, slm_point_info* info) {
  return solve_l0_profile_impl<true>(ds, alpha_min, max_groups, eta, T, big_M, need, max_nodes, beta_out, support_out, value_out, nodes_out, info);
}

// The same search under linear constraints lo <= A beta <= hi and a per-column box (the kernel's constrained instantiation).
extern "C" int slm_solve_l0_constrained(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T, double big_M,
                                        const uint64_t* need, int64_t max_nodes, const double* A, int32_t m, const double* lo,
                                        const double* hi, const double* box_lo, const double* box_hi, int32_t max_qp_sweeps,
                                        double* beta_out, uint64_t* support_out, double* lower_bound_out, int64_t* nodes_out,
                                        double* lambda_out, slm_point_info* info) {
  return solve_l0_con_impl(ds, alpha, max_groups, eta, T, big_M, need, max_nodes, A, m, lo, hi, box_lo, box_hi, max_qp_sweeps, beta_out,
                           support_out, lower_bound_out, nodes_out, lambda_out, info);
}
