// Host side of the MI355X fit engine, sixth unit: the exact l0 estimators (csrc/l0_kernels.hpp) -- the reference's
// mixed-integer family (reference src/sparselm/model/_miqp/_best_subset.py, _regularized_l0.py), which it hands to
// Gurobi or SCIP through cvxpy.  Twelve entries, four functions (solve_l0_impl, solve_l0_profile_impl, solve_l0_con_impl,
// solve_l0_profile_grid_impl), ONE
// pipeline, everything around the launch on the host (p <= 128: microseconds):
//   check    l0_check_args, and what a mode adds: whatever can be refused is refused before a device is touched
//   prepare  l0_prepare: the dataset's own Gram (engine_cov.hip; l0_fetch_gram), then l0_order: the search order, H = G + 2 eta T, c
//            and the hierarchy in that order, the unconstrained value q_all on all columns
//   seed     l0_greedy of l0_host.hpp, every support valued as the kernel values a node
//   plan     l0_plan: the grid, the layout of the one device block (l0_layout), its host image, the kernel's common arguments;
//            a mode appends its sections (L0Plan::append) and seeds its control words
//   launch   l0_run: ONE launch of the mode's instantiation of l0_search_kernel, the part of the block before H read back
//   collect  l0_winner: the waves' bests and the seed under the tie rule; the winner's coefficients recomputed here from H on its
//            support; l0_caller_mask and l0_scatter take both back to the caller's groups and columns
//   prove, report  what leaves the result unproven (budget, capacity rule, unsettled candidates); l0_report, then the mode's fields
// What a mode adds to it:
//   slm_solve_l0_l1 (the reference's L1L0, _regularized_l0.py:258-410)  the kernel's L1 instantiation; the l0_l1_* functions of
//       l0_host.hpp value the seed and the winner; the subtree bound uses the lasso dual value on all columns.
//   slm_solve_l0_profile  the PROFILE instantiation: the best support of every size up to max_groups.  A seed and a winner per
//       size, 64 results per wave, the incumbents per size behind the control words.
//   slm_solve_l0_l1_profile, slm_solve_l0_l1_profile_wide  the L1 + PROFILE instantiations: L1L0 at every alpha from one search, narrow and
//       wide.  The profile's pipeline with l0_l1_support_of for the seed and the winners and l0_l1_lower_bound for the cut.
//   slm_solve_l0_wide, slm_solve_l0_profile_wide  the WIDE instantiations: up to 128 columns and groups, masks of two words, a
//       support of at most 64 independent columns (the capacity rule of l0_host.hpp).  One template over WIDE serves both widths.
//   slm_solve_l0_constrained  the CON instantiation: rows lo <= A beta <= hi and a per-column box.  The l0_con_* functions of
//       l0_host.hpp give the seed, the bound on all columns and the winner; A, lo, hi and the box are appended to the block.
//   slm_solve_l0_xb, slm_solve_l0_xb_wide  the XB instantiations: the subtree bound on everything not yet excluded.
//       l0_excl_plan of l0_host.hpp hands over P = H^-1, P c (appended to the block) and the margin delta; where H is not
//       positive definite on all columns, or delta >= 1/2, the plain kernel runs on the plain block and info->mode says so.
//   slm_solve_l0_profile_batch  the BATCH instantiation: the profiles of up to 16 row sets of the dataset (CV folds, all rows) from
//       one launch.  Per problem the profile's own pieces (l0_fetch_gram, l0_order, l0_profile_seed, l0_profile_collect) on its copy
//       of the block (l0_batch_layout of l0_host.hpp); an intercept column is eliminated per row set (l0_eliminate_last).
//   slm_solve_l0_profile_grid  the BATCH instantiations, with or without L1: one problem per (row set, eta), up to L0_GRID_MAX, from
//       one launch.  Gram and elimination once per row set; order, seed, (l1: the bound) and the copy of the block per problem.
//       slm_solve_l0_profile_batch is its call with one ridge eta.
// Beside them, and none of the above: the local search beyond 128 columns, which proves nothing (csrc/l0_local_kernels.hpp) --
// four entries, ONE body at the end of the unit (solve_l0_local_folds_impl): slm_solve_l0_local_folds, the search on up to 16 row sets
// of the dataset in one launch; slm_solve_l0_local and slm_solve_l0_local_descent, that call with one row set, the dataset's own
// rows; slm_solve_l0_local_subsets, that call with the kernel's cardinality rule: sizes where the alphas are.  (A fifth entry on that
// body, with its own kernel: slm_solve_l0_local_groups, the search with groups and a hierarchy -- csrc/l0_local_group_kernels.hpp.  A
// sixth: slm_solve_l0_local_l1, the penalised rule with an l1 term -- l0_local_l1_kernel, the family's body compiled a third time.)
#include "engine_internal.hpp"
#include "l0_host.hpp"
#include "l0_kernels.hpp"
#include "l0_local_kernels.hpp"
#include "l0_local_group_kernels.hpp"
#include "l0_local_bound_kernels.hpp"
#include "l0_local_node_kernels.hpp"
#include "l0_local_group_node_kernels.hpp"

namespace {

constexpr long long kL0DefaultNodes = 1ll << 30;  // the budget of a call that names none: at the 6.2e8 nodes/s measured at 25 x 30
                                                  // (profiles/l0_search.txt) a call that exhausts it stays under two seconds

// need[g] of the caller (the dataset's group order) as a mask
inline unsigned long long l0_need_of(const uint64_t* need, int g, unsigned long long) { return need[g]; }
inline L0Mask128 l0_need_of(const uint64_t* need, int g, L0Mask128) { return L0Mask128{need[2 * g], need[2 * g + 1]}; }

// The argument checks every entry shares, before anything touches the device.  alpha_name: what the l0 weight is called in
// the entry's own signature.  Leaves p and the group count (without the last `drop` columns and groups).  Mask: one word, or the two of the wide entries (need then holds
// two words per group, the low one first; the limits are L0_WIDE_PMAX).
template <class Mask>
int l0_check_args(slm_dataset* ds, const void* out, double alpha, const char* alpha_name, double eta, double eta_l1, double big_M,
                  const double* T, const uint64_t* need, int* p_out, int* ng_out, int drop = 0) {
  constexpr int pmax = std::is_same_v<Mask, L0Mask128> ? L0_WIDE_PMAX : L0_PMAX;
  if (!ds || !out) return fail(SLM_ERR_BAD_ARG, "NULL argument");
  if (!(alpha >= 0.0) || !std::isfinite(alpha)) return fail(SLM_ERR_BAD_ARG, "%s must be finite and >= 0", alpha_name);
  if (!(eta >= 0.0) || !std::isfinite(eta)) return fail(SLM_ERR_BAD_ARG, "eta must be finite and >= 0");
  if (!(eta_l1 >= 0.0) || !std::isfinite(eta_l1)) return fail(SLM_ERR_BAD_ARG, "eta_l1 must be finite and >= 0");
  if (!(big_M >= 0.0)) return fail(SLM_ERR_BAD_ARG, "big_M must be >= 0");
  const int64_t p64 = ds->p - drop;  // (drop: the batched profile's intercept column, last and alone in the last group, is not searched)
  const int ng = ds->singleton ? (int)std::min<int64_t>(p64, pmax + 1) : ds->G - drop;
  if (need && ng <= pmax)
    for (int g = 0; g < ng; ++g)
      if (l0m_any_outside(l0_need_of(need, g, Mask{}), l0m_below<Mask>(ng)))
        return fail(SLM_ERR_BAD_ARG, "need[%d] names a group at or beyond n_groups = %d", g, ng);
  if (T)
    for (int64_t e = 0; e < p64 * p64 && p64 <= pmax; ++e)
      if (!std::isfinite(T[e])) return fail(SLM_ERR_BAD_ARG, "T contains a non-finite value");
  if (p64 > pmax || ng > pmax)
    return fail(SLM_ERR_UNSUPPORTED, "the %sexact l0 search takes up to %d columns and %d groups (got %lld, %d)",
                pmax != L0_PMAX ? "wide " : "", pmax, pmax, (long long)p64, ng);
  if (row_sharded(ds)) return fail(SLM_ERR_UNSUPPORTED, "the exact l0 search is not built for row-sharded datasets");
  *p_out = (int)p64;
  *ng_out = ng;
  return SLM_OK;
}

// What every search works on: the dataset's Gram on the host, the search order, H = G + 2 eta T and c in that order, the
// hierarchy in that order, and the unconstrained value on all columns.
// (Mask: one word, or the wide mode's two.)
template <class Mask>
struct L0ProblemT {
  std::vector<double> G, cvec, H, c;  // G, cvec: the dataset's order; H, c: search order
  std::vector<int> cols, gstart, gorder;
  std::vector<Mask> needo;
  double q_all = 0.0, yy = 0.0;
};

// Entry `entry` of the dataset's Gram store to the host: G = X^T W X / n_eff, c = X^T W y / n_eff, yy = y^T W y / n_eff.
int l0_fetch_gram(slm_dataset* ds, int p, int entry, std::vector<double>& G, std::vector<double>& cvec, double* yy) {
  hipStream_t s = ds->eng->stream;
  if (entry < 0) return fail(SLM_ERR_HIP, "the dataset's Gram was not filed");
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
  *yy = ds->cov[(size_t)entry].yy;
  return SLM_OK;
}

// From P.G, P.cvec (the first p columns of the dataset, in its order) to the search's own order; host code only.
template <class Mask>
void l0_order(const slm_dataset* ds, int p, int ng, double eta, const double* T, const uint64_t* need, L0ProblemT<Mask>& P) {
  const std::vector<double>&G = P.G, &cvec = P.cvec;

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
}

template <class Mask>
int l0_prepare(slm_dataset* ds, int p, int ng, double eta, const double* T, const uint64_t* need, L0ProblemT<Mask>& P) {
  HIP_TRY(hipSetDevice(ds->eng->device));
  // ---- the dataset's own Gram ---------------------------------------------------------------------------------------------
  SLM_TRY(slm_dataset_covariance(ds, nullptr, 0));
  const double* wdev = ds->rw;
  double fp[2];
  SLM_TRY(cov_fingerprints(ds, &wdev, 1, fp));
  SLM_TRY(l0_fetch_gram(ds, p, cov_find(ds, fp[0], fp[1], (double)ds->n_global), P.G, P.cvec, &P.yy));
  l0_order(ds, p, ng, eta, T, need, P);
  return SLM_OK;
}

// ---- plan, launch ---------------------------------------------------------------------------------------------------------------

using L0Kernel = void (*)(L0Args);

// What one launch needs: the layout of the device block, its host image and the kernel's arguments.  The arguments' device
// pointers are set by l0_run, which allocates the block; `extra` remembers which argument each appended section is.
struct L0Plan {
  L0Layout y;
  std::vector<unsigned long long> h;  // the image of the block; after l0_run its part before H holds what the device left
  L0Args k;
  std::vector<std::pair<const double* L0Args::*, size_t>> extra;  // (kernel argument, offset) of every appended section
  // a mode's own section of n doubles behind what is there, handed to the kernel as k.*field; its offset
  size_t append(const double* L0Args::*field, const double* src, size_t n) {
    const size_t at = y.append(n);
    h.resize(y.words, 0ull);
    if (n > 0) memcpy(h.data() + at, src, sizeof(double) * n);
    extra.emplace_back(field, at);
    return at;
  }
};

// The plan every mode starts from.  slots: results per wave (1; profile mode 64); ctl_words: L0_CTL_WORDS or L0_PROFILE_WORDS;
// q_all: the lower bound on the value of all columns that the subtree bound uses.  The control words are zero: a mode seeds its own.
template <class Mask>
L0Plan l0_plan(const slm_engine* eng, const L0ProblemT<Mask>& P, int p, int ng, int K, int slots, int ctl_words, double alpha, double big_M,
               double q_all, int64_t max_nodes) {
  L0Plan plan;
  plan.y = l0_layout(p, ng, eng->cus, (int)(sizeof(Mask) / sizeof(unsigned long long)), slots, ctl_words, L0_PREFIX, L0_WAVES);
  plan.h.assign(plan.y.words, 0ull);
  l0_fill_image(plan.y, P.H.data(), P.c.data(), p, P.needo, P.gstart, plan.h.data());
  L0Args& k = plan.k;
  memset(&k, 0, sizeof(k));
  k.p = p; k.ng = ng; k.d = plan.y.d; k.K = K;
  k.alpha = alpha; k.big_M = big_M; k.q_all = q_all;
  k.max_nodes = max_nodes > 0 ? max_nodes : kL0DefaultNodes;
  return plan;
}

// The search's one device block: the stream is drained and the block freed however the round trip ends.
struct L0DevGuard {
  unsigned long long*& p;
  hipStream_t s;
  ~L0DevGuard() {
    (void)hipStreamSynchronize(s);
    dfree(p);
  }
};

// The device round trip: the block up, ONE launch of `kernel`, the part before H back into plan.h.
int l0_run(slm_engine* eng, L0Plan& plan, L0Kernel kernel) {
  hipStream_t s = eng->stream;
  const L0Layout& y = plan.y;
  unsigned long long* dev = nullptr;
  SLM_TRY(dalloc(&dev, y.words));
  L0DevGuard guard{dev, s};
  HIP_TRY(hipMemcpyAsync(dev, plan.h.data(), sizeof(unsigned long long) * y.words, hipMemcpyHostToDevice, s));
  L0Args& k = plan.k;
  k.ctl = dev;
  k.best_val = reinterpret_cast<double*>(dev + y.off_bv);
  k.best_mask = dev + y.off_bm;
  k.H = reinterpret_cast<const double*>(dev + y.off_H);
  k.c = reinterpret_cast<const double*>(dev + y.off_c);
  k.need = dev + y.off_need;
  k.gstart = reinterpret_cast<const long long*>(dev + y.off_gs);
  for (const auto& e : plan.extra) k.*e.first = reinterpret_cast<const double*>(dev + e.second);
  hipLaunchKernelGGL(kernel, dim3((unsigned)y.blocks), dim3(64 * L0_WAVES), 0, s, k);
  SLM_TRY(check_launch());
  HIP_TRY(hipMemcpyAsync(plan.h.data(), dev, sizeof(unsigned long long) * y.off_H, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return SLM_OK;
}

// ---- report ---------------------------------------------------------------------------------------------------------------------
//
// The record's common fields: n_iter = 1 launch, status (OK: proven optimal), loss, mode = 4, kkt = the objective, mu = the
// seed's objective, L = the lower bound on all columns that the subtree bound used.  What a mode then writes into the rest:
//
//   entry                 rejects                      resid                         beta_norm            mode
//   solve_l0, _l1         candidates the descent       0                             ||beta||_2           4
//                         valued (l1 mode; else 0)
//   solve_l0_wide         c_min + 1 of the capacity    1: the node budget ran out    ||beta||_2           4
//                         rule, 0: no include refused
//   solve_l0_xb[_wide]    as the entry without _xb     as the entry without _xb      the margin delta     5 the exclusion bound ran,
//                                                                                                         6 H not definite, 7 delta >= 1/2
//   solve_l0_constrained  candidates valued (qp        candidates that ran out of    the lowest bound on  4
//                         solves)                      sweeps                        those, +inf: none
//   solve_l0_profile[_wide]  0                         0                             0                    4 (loss 0; kkt: the regularised
//                                                      optimum at alpha_min; mu: the best-subset optimum at max_groups)
void l0_report(slm_point_info* info, bool proven, double loss, double objective, double seed, double bound) {
  memset(info, 0, sizeof(*info));
  info->n_iter = 1;
  info->status = proven ? SLM_OK : SLM_ERR_NOT_CONVERGED;
  info->loss = loss;
  info->mode = 4;
  info->kkt = objective;
  info->mu = seed;
  info->L = bound;
}
inline int32_t l0_count32(unsigned long long v) { return (int32_t)std::min<unsigned long long>(v, 0x7fffffffull); }

int l0_budget_ran_out(const L0Plan& plan, const char* what) {
  return fail(SLM_ERR_NOT_CONVERGED, "the node budget (%lld) ran out before the search finished: the %s is returned", plan.k.max_nodes, what);
}

// ---- the entries ----------------------------------------------------------------------------------------------------------------

// slm_solve_l0, _l1, _wide, _xb, _xb_wide.  eta_l1 > 0 is l1 mode (the kernel's L1 instantiation, the l0_l1_* functions of
// l0_host.hpp); WIDE: masks of two words in need, support_out and on the device (no l1 mode there); XB: the exclusion bound
// (never with an l1 term).
template <bool WIDE, bool XB = false>
int solve_l0_impl(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T, double eta_l1, double big_M,
                  const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out, double* lower_bound_out,
                  int64_t* nodes_out, slm_point_info* info) {
  using Mask = std::conditional_t<WIDE, L0Mask128, unsigned long long>;
  int p = 0, ng = 0;
  SLM_TRY(l0_check_args<Mask>(ds, beta_out, alpha, "alpha", eta, eta_l1, big_M, T, need, &p, &ng));
  const bool l1 = !WIDE && eta_l1 > 0.0;
  const int K = max_groups < 0 ? 0 : std::min<int>(max_groups, ng);
  L0ProblemT<Mask> P;
  SLM_TRY(l0_prepare(ds, p, ng, eta, T, need, P));
  const double *H = P.H.data(), *c = P.c.data(), q_all = P.q_all;
  // the value (without alpha |S|) and coefficients of one support, as the kernel values a node
  auto value_of = [&](Mask mask, bool polish, double* beta) {
    if constexpr (WIDE)
      return l0_support_of(H, c, p, P.gstart, mask, big_M, polish, beta);
    else
      return l1 ? l0_l1_support(H, c, p, P.gstart, mask, eta_l1, big_M, polish, beta) : l0_support(H, c, p, P.gstart, mask, big_M, polish, beta);
  };
  [[maybe_unused]] L0ExclPlan excl;
  if constexpr (XB) excl = l0_excl_plan(H, c, p);

  // ---- the greedy seed of the incumbent ------------------------------------------------------------------------------------
  std::vector<double> beta_s((size_t)p);
  // the subtree bound's lower bound on the value of all columns: in l1 mode the lasso dual value where it is above q_all
  const double bound = l1 ? l0_l1_lower_bound(H, c, p, P.yy, eta_l1, q_all) : q_all;
  double seed_val = 0.0;  // the empty support
  Mask seed_mask = l0m_none<Mask>();
  l0_greedy(H, c, p, P.gstart, P.needo, K, [&](Mask mask) { return value_of(mask, false, beta_s.data()); },
            [&](int size, Mask mask, double quad) {
              const double v = quad + alpha * (double)size;
              if (v < seed_val) {
                seed_val = v;
                seed_mask = mask;
              }
            });

  // ---- the search: one launch of the mode's kernel; where the exclusion bound cannot run, the plain kernel on the plain block --
  L0Plan plan = l0_plan(ds->eng, P, p, ng, K, 1, L0_CTL_WORDS, alpha, big_M, bound, max_nodes);
  plan.h[L0_INCUMBENT] = l0_key(seed_val);
  if constexpr (WIDE) plan.h[L0_CAPACITY] = ~0ull;  // (lowered by a wave that refused an include for capacity)
  plan.k.eta_l1 = eta_l1;
  L0Kernel kernel;
  if constexpr (WIDE) kernel = l0_search_kernel<false, false, true>;
  else kernel = l1 ? l0_search_kernel<true> : l0_search_kernel<false>;
  if constexpr (XB)
    if (excl.reason == 0) {
      plan.append(&L0Args::P, excl.P.data(), (size_t)p * p);
      plan.append(&L0Args::bhat, excl.bhat.data(), (size_t)p);
      plan.k.xb_delta = excl.delta;
      kernel = l0_search_kernel<false, false, WIDE, false, true>;
    }
  SLM_TRY(l0_run(ds->eng, plan, kernel));
  const std::vector<unsigned long long>& h = plan.h;

  // ---- the winner, its coefficients recomputed here whichever wave found it -------------------------------------------------
  double win_val = seed_val;
  Mask win_mask = seed_mask;
  l0_winner(h.data(), plan.y.off_bv, plan.y.off_bm, plan.y.waves, 1, 0, win_val, win_mask);
  const bool finished = h[L0_ABORTED] == 0;
  const double quad = value_of(win_mask, true, beta_s.data());
  int n_active = 0;
  const Mask support = l0_caller_mask(win_mask, P.gorder, &n_active);
  const double objective = quad + alpha * (double)n_active;
  l0_scatter(beta_s.data(), P.cols, beta_out);
  if (support_out) memcpy(support_out, &support, sizeof(Mask));
  // wide: c_min + 1 of the capacity rule (l0_host.hpp), 0 when no include was refused because the factor was full
  const int cut = WIDE && h[L0_CAPACITY] != ~0ull ? (int)h[L0_CAPACITY] : 0;
  const bool proven = finished && l0_capacity_proven(objective, q_all, alpha, cut);
  double lower = finished ? objective : std::min(objective, bound);
  if (cut) lower = std::min(lower, l0_capacity_bound(q_all, alpha, cut));
  if (lower_bound_out) *lower_bound_out = lower;
  if (nodes_out) *nodes_out = (int64_t)h[L0_NODES];
  if (info) {
    l0_report(info, proven, l0_gram_loss(P.G.data(), P.cvec.data(), p, P.yy, beta_out), objective, seed_val, bound);
    info->rejects = WIDE ? cut : l0_count32(h[L0_DESCENTS]);
    if constexpr (WIDE) info->resid = finished ? 0.0 : 1.0;  // (what tells an exhausted budget from a result unproven for capacity alone)
    double bn = 0.0;
    for (int j = 0; j < p; ++j) bn += beta_out[j] * beta_out[j];
    info->beta_norm = std::sqrt(bn);
    if constexpr (XB) {  // which bound ran, and its margin
      info->mode = excl.reason == 0 ? 5 : (excl.reason == 1 ? 6 : 7);
      info->beta_norm = excl.delta;
    }
  }
  if (!finished) return l0_budget_ran_out(plan, "incumbent");
  if (!proven)
    return fail(SLM_ERR_NOT_CONVERGED, "a support holds at most %d independent columns: includes were refused from %d groups on, and the "
                "incumbent is above the bound %.17g on what lies behind them", L0_PMAX, cut - 1, l0_capacity_bound(q_all, alpha, cut));
  return SLM_OK;
}

// The profile's pieces around its launch, shared by the single entries and the batched one.
constexpr int kL0BatchMax = 16;  // row sets of one batched launch: what the dataset's Gram store holds
static_assert(kL0BatchMax == L0_GRID_ROW_SETS && SLM_L0_GRID_MAX == L0_GRID_MAX, "the header, the host logic and this unit name one set of limits");
template <class Mask>
struct L0ProfileWork {
  L0ProblemT<Mask> P;
  std::vector<double> win_val;  // [L0_PMAX + 1] per size: the seed, then the winner
  std::vector<Mask> win_mask;
};
// the seed of every size: the supports the greedy selection passes through, valued as the kernel values a node
// (eta_l1 > 0, here and in l0_profile_collect: the l1 profile -- a support's value is its lasso, l0_l1_support_of)
template <class Mask>
void l0_profile_seed(L0ProfileWork<Mask>& W, int p, int K, double big_M, double eta_l1 = 0.0) {
  const L0ProblemT<Mask>& P = W.P;
  const double *H = P.H.data(), *c = P.c.data();
  std::vector<double> beta_s((size_t)p);
  auto value_of = [&](Mask mask) {
    return eta_l1 > 0.0 ? l0_l1_support_of(H, c, p, P.gstart, mask, eta_l1, big_M, false, beta_s.data())
                        : l0_support_of(H, c, p, P.gstart, mask, big_M, false, beta_s.data());
  };
  W.win_val.assign((size_t)L0_PMAX + 1, HUGE_VAL);
  W.win_mask.assign((size_t)L0_PMAX + 1, l0m_ones<Mask>());
  W.win_val[0] = 0.0;  // the empty support
  W.win_mask[0] = l0m_none<Mask>();
  l0_greedy(H, c, p, P.gstart, P.needo, K, value_of,
            [&](int size, Mask mask, double quad) {
              if (l0_better(quad, mask, W.win_val[(size_t)size], W.win_mask[(size_t)size])) {
                W.win_val[(size_t)size] = quad;
                W.win_mask[(size_t)size] = mask;
              }
            });
}
// the incumbents of the sizes 1 .. 64 behind the control words of one problem's image
template <class Mask>
void l0_profile_seed_image(const L0ProfileWork<Mask>& W, unsigned long long* h) {
  for (int k = 1; k <= L0_PMAX; ++k) h[(size_t)L0_PROFILE_INC + (size_t)k - 1] = l0_key(W.win_val[(size_t)k]);
}
// per size: the winner among the seed and the waves' results, its coefficients recomputed here; a size nobody filled: +inf, all
// ones, zeros.  h: one problem's part of the block as read back.  Then the node count and the record.
template <class Mask>
void l0_profile_collect(L0ProfileWork<Mask>& W, const unsigned long long* h, const L0Layout& y, int p, int rows, int K, double alpha_min,
                        double big_M, bool finished, double* beta_out, uint64_t* support_out, double* value_out, int64_t* nodes_out,
                        slm_point_info* info, double eta_l1 = 0.0) {
  const L0ProblemT<Mask>& P = W.P;
  const double *H = P.H.data(), *c = P.c.data();
  std::vector<double> beta_s((size_t)p);
  for (int size = 1; size <= K; ++size) l0_winner(h, y.off_bv, y.off_bm, y.waves, 64, size - 1, W.win_val[(size_t)size], W.win_mask[(size_t)size]);
  for (int size = 0; size <= rows; ++size) {
    double* beta = beta_out + (size_t)size * p;
    for (int i = 0; i < p; ++i) beta[i] = 0.0;
    const bool filled = size <= K && std::isfinite(W.win_val[(size_t)size]);
    value_out[size] = HUGE_VAL;
    Mask support = l0m_ones<Mask>();
    if (filled) {
      value_out[size] = eta_l1 > 0.0 ? l0_l1_support_of(H, c, p, P.gstart, W.win_mask[(size_t)size], eta_l1, big_M, true, beta_s.data())
                                     : l0_support_of(H, c, p, P.gstart, W.win_mask[(size_t)size], big_M, true, beta_s.data());
      support = l0_caller_mask(W.win_mask[(size_t)size], P.gorder);
      l0_scatter(beta_s.data(), P.cols, beta);
    }
    memcpy(support_out + (sizeof(Mask) / sizeof(uint64_t)) * (size_t)size, &support, sizeof(Mask));  // (a mask: one word, wide two)
  }
  if (nodes_out) *nodes_out = (int64_t)h[L0_NODES];
  if (info) {
    const int at = l0_profile_regularized(value_out, K, alpha_min), sub = l0_profile_best_subset(value_out, K);
    l0_report(info, finished, 0.0, value_out[at] + alpha_min * (double)at, value_out[sub], P.q_all);
  }
}

// slm_solve_l0_profile, _profile_wide: a seed and a winner per size.  Wide: lane k - 1 still holds size k, and no include may be
// refused for capacity, so a call whose max_groups largest groups could hold more than L0_PMAX columns is refused before anything
// is launched.
// slm_solve_l0_l1_profile, _l1_profile_wide (eta_l1 > 0): the kernel's L1 + PROFILE instantiations.  Seed and winners are valued by
// l0_l1_support_of, the subtree cut takes l0_l1_lower_bound on all columns for q_all, info->L is that bound and info->rejects the
// descents run.  The wide refusals above also keep every support's column list within the 64 lanes.  eta_l1 == 0 is the profile itself.
template <bool WIDE>
int solve_l0_profile_impl(slm_dataset* ds, double alpha_min, int32_t max_groups, double eta, const double* T, double eta_l1, double big_M,
                          const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out, double* value_out,
                          int64_t* nodes_out, slm_point_info* info) {
  using Mask = std::conditional_t<WIDE, L0Mask128, unsigned long long>;
  int p = 0, ng = 0;
  if (!support_out || !value_out) return fail(SLM_ERR_BAD_ARG, "NULL argument");
  SLM_TRY(l0_check_args<Mask>(ds, beta_out, alpha_min, "alpha_min", eta, eta_l1, big_M, T, need, &p, &ng));
  const bool l1 = eta_l1 > 0.0;
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
  L0ProfileWork<Mask> W;
  SLM_TRY(l0_prepare(ds, p, ng, eta, T, need, W.P));
  l0_profile_seed(W, p, K, big_M, eta_l1);
  // the subtree cut's lower bound on the value of all columns: with an l1 term the lasso dual value where it is above q_all
  const double bound = l1 ? l0_l1_lower_bound(W.P.H.data(), W.P.c.data(), p, W.P.yy, eta_l1, W.P.q_all) : W.P.q_all;

  // ---- the search: one launch, 64 results per wave, the incumbents of the sizes 1 .. 64 behind the control words ----------------
  L0Plan plan = l0_plan(ds->eng, W.P, p, ng, K, 64, L0_PROFILE_WORDS, alpha_min, big_M, bound, max_nodes);
  l0_profile_seed_image(W, plan.h.data());
  if constexpr (WIDE) plan.h[L0_CAPACITY] = ~0ull;
  plan.k.eta_l1 = eta_l1;
  SLM_TRY(l0_run(ds->eng, plan, l1 ? l0_search_kernel<true, true, WIDE> : l0_search_kernel<false, true, WIDE>));
  const std::vector<unsigned long long>& h = plan.h;

  const bool finished = h[L0_ABORTED] == 0;
  if (WIDE && h[L0_CAPACITY] != ~0ull) return fail(SLM_ERR_HIP, "the wide l0 profile refused an include for capacity (internal error)");
  l0_profile_collect(W, h.data(), plan.y, p, rows, K, alpha_min, big_M, finished, beta_out, support_out, value_out, nodes_out, info, eta_l1);
  if (info && l1) {
    info->L = bound;
    info->rejects = l0_count32(h[L0_DESCENTS]);
  }
  if (!finished) return l0_budget_ran_out(plan, "table of incumbents");
  return SLM_OK;
}

// slm_solve_l0_profile_grid, slm_solve_l0_profile_batch: the profiles of `count` row sets of one dataset at n_eta weights each from
// ONE launch of the kernel's BATCH instantiation (l1: the L1 one).  Problem b = r * n_eta + e (l0_grid_index) is row set r with etas[e]:
// a ridge weight (H = G_r + 2 eta T) or an l1 weight (H = G_r).  Per row set, once: its Gram (fetched before anything else:
// l0_fetch_gram), the intercept column eliminated (l0_eliminate_last).  Per problem today's pipeline, piece by piece: l0_order,
// l0_profile_seed, its copy of the block (l0_batch_layout, l0_fill_image, l0_profile_seed_image, the subtree cut's bound in
// L0_BATCH_QALL, the l1 weight in L0_BATCH_ETA); then one upload, one launch, one read-back of the block, and l0_profile_collect
// per problem.  grid = false is slm_solve_l0_profile_batch: one ridge eta, checked and reported in that entry's own words.
int solve_l0_profile_grid_impl(bool grid, slm_dataset* ds, int32_t count, const double* const* row_weights, const int64_t* n_effs,
                               int32_t intercept, int32_t n_eta, const double* etas, int32_t eta_kind, double alpha_min, int32_t max_groups,
                               const double* T, double big_M, const uint64_t* need, int64_t max_nodes, double* beta_out,
                               double* intercept_out, uint64_t* support_out, double* value_out, int64_t* nodes_out, slm_point_info* info) {
  using Mask = unsigned long long;
  int ps = 0, ng = 0;
  if (count < 1 || count > kL0BatchMax) return fail(SLM_ERR_BAD_ARG, "count must be 1 .. %d, the Gram store's capacity (got %d)", kL0BatchMax, count);
  if (grid) {
    int which = 0;
    switch (l0_grid_check(count, n_eta, etas, eta_kind, T != nullptr, &which)) {
      case L0_GRID_OK: break;
      case L0_GRID_N_ETA: return fail(SLM_ERR_BAD_ARG, "n_eta must be >= 1 (got %d)", n_eta);
      case L0_GRID_NULL: return fail(SLM_ERR_BAD_ARG, "NULL argument");
      case L0_GRID_KIND: return fail(SLM_ERR_BAD_ARG, "eta_kind must be 0 (ridge) or 1 (l1) (got %d)", eta_kind);
      case L0_GRID_T_WITH_L1: return fail(SLM_ERR_BAD_ARG, "T goes with the ridge weights (eta_kind 0): the l1 profile has no ridge term");
      case L0_GRID_ETA: return fail(SLM_ERR_BAD_ARG, "etas[%d] must be finite and >= 0", which);
      case L0_GRID_PROBLEMS:
        return fail(SLM_ERR_BAD_ARG, "count * n_eta must be at most %d problems (got %d x %d = %lld)", L0_GRID_MAX, count, n_eta,
                    (long long)count * n_eta);
      default: return fail(SLM_ERR_BAD_ARG, "count must be 1 .. %d, the Gram store's capacity (got %d)", kL0BatchMax, count);
    }
  }
  const bool l1 = eta_kind == 1;
  const int problems = count * n_eta;
  if (!support_out || !value_out || !row_weights || !n_effs) return fail(SLM_ERR_BAD_ARG, "NULL argument");
  const int drop = intercept != 0 ? 1 : 0;
  if (ds && drop) {  // the ones column: last, alone in the last group
    const int64_t p = ds->p;
    const int G = ds->singleton ? (int)std::min<int64_t>(p, 1 << 30) : ds->G;
    bool alone = p >= 1 && G >= 1;
    for (int64_t j = 0; j < p && alone && !ds->h_gid.empty(); ++j) alone = (ds->h_gid[(size_t)j] == G - 1) == (j == p - 1);
    if (!alone) return fail(SLM_ERR_BAD_ARG, "intercept: the last column must be alone in the last group");
  }
  SLM_TRY(l0_check_args<Mask>(ds, beta_out, alpha_min, "alpha_min", grid ? 0.0 : etas[0], 0.0, big_M, T, need, &ps, &ng, drop));
  const int p = ps + drop;
  const int rows = max_groups < 0 ? 0 : (int)max_groups;
  const int K = std::min(rows, ng);
  const int64_t n = ds->n;
  for (int b = 0; b < count; ++b)
    for (int64_t i = 0; i < n && row_weights[b]; ++i)
      if (!(row_weights[b][i] >= 0.0) || !std::isfinite(row_weights[b][i]))
        return fail(SLM_ERR_BAD_ARG, "row_weights[%d][%lld] must be finite and >= 0", b, (long long)i);
  slm_engine* eng = ds->eng;
  HIP_TRY(hipSetDevice(eng->device));
  hipStream_t s = eng->stream;

  // ---- the Grams: the folds' in one call when every row set brings its weights, else one by one; each fetched at once ---------
  bool all_given = true;
  for (int b = 0; b < count; ++b) all_given = all_given && row_weights[b] != nullptr;
  struct Weights {
    double* dev = nullptr;
    hipStream_t s;
    ~Weights() {
      (void)hipStreamSynchronize(s);
      dfree(dev);
    }
  } wts;
  wts.s = s;
  SLM_TRY(dalloc(&wts.dev, (size_t)count * (size_t)n));
  std::vector<const double*> wdev((size_t)count);
  std::vector<double> neff((size_t)count);
  for (int b = 0; b < count; ++b) {
    neff[(size_t)b] = row_weights[b] && n_effs[b] > 0 ? (double)n_effs[b] : (double)ds->n_global;
    wdev[(size_t)b] = ds->rw;
    if (!row_weights[b]) continue;
    wdev[(size_t)b] = wts.dev + (size_t)b * (size_t)n;
    HIP_TRY(hipMemcpyAsync(wts.dev + (size_t)b * (size_t)n, row_weights[b], sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
  }
  if (all_given) SLM_TRY(slm_dataset_covariance_folds(ds, row_weights, n_effs, count));
  std::vector<double> fp(2 * (size_t)count);
  SLM_TRY(cov_fingerprints(ds, wdev.data(), count, fp.data()));
  std::vector<L0ProfileWork<Mask>> W((size_t)problems);
  std::vector<double> xmean((size_t)count * (size_t)ps, 0.0), ymean((size_t)count, 0.0);
  std::vector<double> bound((size_t)problems, 0.0);  // what the subtree cut takes for the value of all columns: q_all, or the l1 bound
  for (int b = 0; b < count; ++b) {
    L0ProblemT<Mask>& P = W[(size_t)l0_grid_index(b, 0, n_eta)].P;  // (the row set's Gram lands in its first problem and is copied on)
    int entry = cov_find(ds, fp[2 * (size_t)b], fp[2 * (size_t)b + 1], neff[(size_t)b]);
    if (entry < 0) {  // not from the folds' call (or pushed out of the store by a later one): built here, fetched at once
      SLM_TRY(slm_dataset_covariance(ds, row_weights[b], row_weights[b] ? n_effs[b] : 0));
      entry = cov_find(ds, fp[2 * (size_t)b], fp[2 * (size_t)b + 1], neff[(size_t)b]);
    }
    SLM_TRY(l0_fetch_gram(ds, p, entry, P.G, P.cvec, &P.yy));
    if (drop) {
      std::vector<double> Gs((size_t)ps * ps), cs((size_t)ps);
      if (!l0_eliminate_last(P.G.data(), P.cvec.data(), p, P.yy, Gs.data(), cs.data(), &P.yy, xmean.data() + (size_t)b * ps, &ymean[(size_t)b]))
        return fail(SLM_ERR_BAD_ARG, "intercept: row set %d gives the last column no weight", b);
      P.G.swap(Gs);
      P.cvec.swap(cs);
    }
    for (int e = 0; e < n_eta; ++e) {
      const int at = l0_grid_index(b, e, n_eta);
      L0ProblemT<Mask>& Q = W[(size_t)at].P;
      if (e > 0) {
        Q.G = P.G;
        Q.cvec = P.cvec;
        Q.yy = P.yy;
      }
      l0_order(ds, ps, ng, l1 ? 0.0 : etas[e], T, need, Q);
      l0_profile_seed(W[(size_t)at], ps, K, big_M, l1 ? etas[e] : 0.0);
      bound[(size_t)at] = l1 && etas[e] > 0.0 ? l0_l1_lower_bound(Q.H.data(), Q.c.data(), ps, Q.yy, etas[e], Q.q_all) : Q.q_all;
    }
  }

  // ---- the block: one copy of the profile layout per problem; one upload, ONE launch, one read-back -------------------------------
  const L0BatchLayout B = l0_grid_layout(count, n_eta, ps, ng, eng->cus, 64, L0_PROFILE_WORDS, L0_PREFIX, L0_WAVES);
  const L0Layout& y = B.one;
  std::vector<unsigned long long> h(B.words, 0ull);
  for (int b = 0; b < problems; ++b) {
    const L0ProblemT<Mask>& P = W[(size_t)b].P;
    unsigned long long* hb = h.data() + B.at(b);
    l0_fill_image(y, P.H.data(), P.c.data(), ps, P.needo, P.gstart, hb);
    l0_profile_seed_image(W[(size_t)b], hb);
    memcpy(hb + L0_BATCH_QALL, &bound[(size_t)b], sizeof(double));
    if (l1) memcpy(hb + L0_BATCH_ETA, &etas[l0_grid_eta(b, n_eta)], sizeof(double));
  }
  L0Args k;
  memset(&k, 0, sizeof(k));
  k.p = ps; k.ng = ng; k.d = y.d; k.K = K;
  k.alpha = alpha_min; k.big_M = big_M;
  k.max_nodes = max_nodes > 0 ? max_nodes : kL0DefaultNodes;
  k.batch_stride = (long long)B.stride;
  k.batch_blocks = y.blocks;
  {
    unsigned long long* dev = nullptr;
    SLM_TRY(dalloc(&dev, B.words));
    L0DevGuard guard{dev, s};
    HIP_TRY(hipMemcpyAsync(dev, h.data(), sizeof(unsigned long long) * B.words, hipMemcpyHostToDevice, s));
    k.ctl = dev;
    k.best_val = reinterpret_cast<double*>(dev + y.off_bv);
    k.best_mask = dev + y.off_bm;
    k.H = reinterpret_cast<const double*>(dev + y.off_H);
    k.c = reinterpret_cast<const double*>(dev + y.off_c);
    k.need = dev + y.off_need;
    k.gstart = reinterpret_cast<const long long*>(dev + y.off_gs);
    const L0Kernel kernel = l1 ? l0_search_kernel<true, true, false, false, false, true> : l0_search_kernel<false, true, false, false, false, true>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)B.grid()), dim3(64 * L0_WAVES), 0, s, k);
    SLM_TRY(check_launch());
    // one read-back: the whole block (the results are most of every copy; H, c, need and the group starts come back as they went)
    HIP_TRY(hipMemcpyAsync(h.data(), dev, sizeof(unsigned long long) * B.words, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }

  // ---- per problem: the winners, the table, the record -------------------------------------------------------------------------------
  const size_t tab = (size_t)rows + 1;
  int unfinished = 0, first = -1;
  for (int b = 0; b < problems; ++b) {
    const unsigned long long* hb = h.data() + B.at(b);
    const int r = l0_grid_row_set(b, n_eta);
    const double eta_l1 = l1 ? etas[l0_grid_eta(b, n_eta)] : 0.0;
    const bool finished = hb[L0_ABORTED] == 0;
    if (!finished && unfinished++ == 0) first = b;
    double* beta_b = beta_out + (size_t)b * tab * ps;
    l0_profile_collect(W[(size_t)b], hb, y, ps, rows, K, alpha_min, big_M, finished, beta_b, support_out + (size_t)b * tab, value_out + (size_t)b * tab,
                       nodes_out ? nodes_out + b : nullptr, info ? info + b : nullptr, eta_l1);
    if (info && l1) {
      info[b].L = bound[(size_t)b];
      info[b].rejects = l0_count32(hb[L0_DESCENTS]);
    }
    for (size_t size = 0; size < tab && intercept_out; ++size) {
      double t = drop ? ymean[(size_t)r] : 0.0;
      for (int j = 0; j < ps && drop; ++j) t -= xmean[(size_t)r * ps + j] * beta_b[size * ps + j];
      intercept_out[(size_t)b * tab + size] = t;
    }
  }
  if (unfinished)
    return fail(SLM_ERR_NOT_CONVERGED, "the node budget (%lld per problem) ran out in %d of %d problems (the first: %d): their tables of "
                "incumbents are returned", k.max_nodes, unfinished, problems, first);
  return SLM_OK;
}

// slm_solve_l0_constrained (DESIGN 4d "Constrained mode").  H must be positive definite on all columns; the rows are scaled to unit
// norm and everything is put in search order; the seed, the bound F_lb on all columns and the winner come from l0_con_solve /
// l0_con_polish of l0_host.hpp, the very splitting the kernel runs.
int solve_l0_con_impl(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T, double big_M, const uint64_t* need,
                      int64_t max_nodes, const double* A, int32_t m, const double* lo, const double* hi, const double* box_lo,
                      const double* box_hi, int32_t max_qp_sweeps, double* beta_out, uint64_t* support_out, double* lower_bound_out,
                      int64_t* nodes_out, double* lambda_out, slm_point_info* info) {
  using Mask = unsigned long long;
  int p = 0, ng = 0;
  SLM_TRY(l0_check_args<Mask>(ds, beta_out, alpha, "alpha", eta, 0.0, big_M, T, need, &p, &ng));
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
  L0ProblemT<Mask> P;
  SLM_TRY(l0_prepare(ds, p, ng, eta, T, need, P));
  const double *H = P.H.data(), *c = P.c.data();
  const std::vector<int>&cols = P.cols, &gstart = P.gstart;
  if (!l0_con_pd(H, c, p))
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
  CP.H = H; CP.c = c; CP.p = p;
  CP.A = As.data(); CP.m = m; CP.lo = los.data(); CP.hi = his.data();
  CP.blo = blo.data(); CP.bhi = bhi.data();
  CP.rho = l0_con_rho(H, p, As.data(), m);
  CP.max_sweeps = L0_CON_SWEEPS;  // (the host's own solves -- seed, bound, winner -- always get the full cap: max_qp_sweeps starves the candidates on chip)

  // ---- F_lb, the subtree bound's proven lower bound on f(all columns); and what no feasible support's objective exceeds ------------
  L0ConPoint all;
  const double bound = l0_con_lower_bound(CP, P.q_all, &all);
  double cap = l0_con_value_cap(H, c, p, blo.data(), bhi.data());
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
    if (l0_better(v, mask, seed_val, seed_mask)) {
      seed_val = v;
      seed_mask = mask;
    }
  };
  l0_greedy(H, c, p, gstart, P.needo, K, value_of, offer);
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

  // ---- the search: one launch; A by columns, lo, hi and the box behind the group starts ---------------------------------------
  L0Plan plan = l0_plan(ds->eng, P, p, ng, K, 1, L0_CTL_WORDS, alpha, big_M, bound, max_nodes);
  plan.h[L0_INCUMBENT] = l0_key(std::min(seed_val, cap));
  plan.h[L0_UNSETTLED] = ~0ull;  // (lowered by a wave whose candidate ran out of sweeps)
  plan.append(&L0Args::A, At.data(), (size_t)m * p);
  plan.append(&L0Args::lo, los.data(), (size_t)m);
  plan.append(&L0Args::hi, his.data(), (size_t)m);
  plan.append(&L0Args::blo, blo.data(), (size_t)p);
  plan.append(&L0Args::bhi, bhi.data(), (size_t)p);
  plan.k.rows = m;
  plan.k.con_sweeps = max_qp_sweeps > 0 ? max_qp_sweeps : L0_CON_SWEEPS;
  plan.k.rho = CP.rho;
  SLM_TRY(l0_run(ds->eng, plan, l0_search_kernel<false, false, false, true>));
  const std::vector<unsigned long long>& h = plan.h;

  // ---- the winner -------------------------------------------------------------------------------------------------------------
  double win_val = seed_val;
  Mask win_mask = seed_mask;
  l0_winner(h.data(), plan.y.off_bv, plan.y.off_bm, plan.y.waves, 1, 0, win_val, win_mask);
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
  if (win_val < HUGE_VAL) {
    const int ms = l0_con_columns(gstart, win_mask, scols);
    L0ConPoint R = l0_con_solve(CP, scols, ms, HUGE_VAL);
    (void)l0_con_polish(CP, scols, ms, R);
    int n_active = 0;
    const Mask support = l0_caller_mask(win_mask, P.gorder, &n_active);
    objective = R.primal + alpha * (double)n_active;
    std::vector<double> beta_s((size_t)p, 0.0);
    for (int r = 0; r < ms; ++r) beta_s[(size_t)scols[r]] = R.beta[(size_t)r];
    l0_scatter(beta_s.data(), cols, beta_out);
    for (int i = 0; i < m && lambda_out; ++i) lambda_out[i] = R.y[(size_t)i] / rnorm[(size_t)i];
    if (support_out) *support_out = support;
  }
  const bool proven = finished && objective <= unsettled_bound && objective < HUGE_VAL;
  double lower = std::min(objective, unsettled_bound);
  if (!finished) lower = std::min(lower, bound);
  if (lower_bound_out) *lower_bound_out = lower;
  if (info) {
    l0_report(info, proven, l0_gram_loss(P.G.data(), P.cvec.data(), p, P.yy, beta_out), objective, seed_val, bound);
    info->rejects = l0_count32(h[L0_DESCENTS]);
    info->resid = (double)n_unsettled;
    info->beta_norm = unsettled_bound;
  }
  if (!finished) return l0_budget_ran_out(plan, "incumbent");
  if (!proven)
    return fail(SLM_ERR_NOT_CONVERGED, "%lld candidate(s) ran out of sweeps (%d each): the incumbent is above the bound %.17g on them",
                n_unsettled, plan.k.con_sweeps, unsettled_bound);
  return SLM_OK;
}

// Rows `rows` (ascending) of a device Gram [.][ld], their first `width` entries, to the host: out[k * width + j].  A few rows
// go one copy each; many go as one strided copy of the stretch that holds them.
int l0_fetch_rows(hipStream_t s, const double* G, size_t ld, int width, const std::vector<int>& rows, std::vector<double>& out) {
  out.assign(rows.size() * (size_t)width, 0.0);
  if (rows.empty()) return SLM_OK;
  if (rows.size() <= 64) {
    for (size_t k = 0; k < rows.size(); ++k)
      HIP_TRY(hipMemcpyAsync(out.data() + k * (size_t)width, G + (size_t)rows[k] * ld, sizeof(double) * (size_t)width, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SLM_OK;
  }
  const int lo = rows.front(), span = rows.back() - lo + 1;
  std::vector<double> all((size_t)span * (size_t)width);
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy2D(all.data(), sizeof(double) * (size_t)width, G + (size_t)lo * ld, sizeof(double) * ld, sizeof(double) * (size_t)width,
                      (size_t)span, hipMemcpyDeviceToHost));
  for (size_t k = 0; k < rows.size(); ++k)
    memcpy(out.data() + k * (size_t)width, all.data() + (size_t)(rows[k] - lo) * (size_t)width, sizeof(double) * (size_t)width);
  return SLM_OK;
}

// The Gram lookup of the local family (solve_l0_local_folds_impl, solve_l0_local_bound_impl): row set b -- its weights on the
// device wdev[b] (the dataset's own where the caller brings none), its divisor neff[b] -- is found in the dataset's store by
// fingerprint or built and filed here; held[b] gets a copy of the entry, which holds its blocks for the call.
int l0_local_hold_grams(slm_dataset* ds, int count, const double* const* row_weights, const int64_t* n_effs, const double* const* wdev,
                        const double* neff, slm_dataset::CovEntry* held) {
  std::vector<double> fp(2 * (size_t)count);
  SLM_TRY(cov_fingerprints(ds, wdev, count, fp.data()));
  for (int b = 0; b < count; ++b) {
    int entry = cov_find(ds, fp[2 * (size_t)b], fp[2 * (size_t)b + 1], neff[(size_t)b]);
    if (entry < 0) {  // not from the folds' call (or pushed out of the store by a later one): built here
      SLM_TRY(slm_dataset_covariance(ds, row_weights[b], row_weights[b] ? n_effs[b] : 0));
      entry = cov_find(ds, fp[2 * (size_t)b], fp[2 * (size_t)b + 1], neff[(size_t)b]);
    }
    if (entry < 0) return fail(SLM_ERR_HIP, "the Gram of row set %d was not filed", b);
    held[b] = ds->cov[(size_t)entry];
  }
  return SLM_OK;
}

// The l0 local search (DESIGN 4d "Local search", "Local search over folds", "Local subsets"): NOT a search over supports and
// not this unit's pipeline -- no order, no seed, no block image -- and ONE body, solve_l0_local_folds_impl, for its four entries:
//   slm_solve_l0_local_folds    `count` row sets of one dataset -- the training rows of a cross-validation's folds, then all rows
//   slm_solve_l0_local[_descent]  that call with ONE row set, the dataset's own rows (a NULL weight vector), no intercept and no
//                               intercept_out / stat_out; only the wording of two messages is its own (L0_LOCAL_ONE)
//   slm_solve_l0_local_subsets  that call with `sizes` in the place of `alphas`: the check is l0_lc_check, the launch
//                               l0_local_kernel<true> (the cardinality rule), the sizes travel as ints where the alphas did, the
//                               objective has no alpha term (Q after the polish), and stat_out holds six words per problem:
//                               grows and drops behind the four
//   slm_solve_l0_local_groups   the FOURTH kind (L0_LOCAL_GROUPS), the only one that goes on with groups: after the shared check
//                               l0_lg_check decides the group order and the need lists; gstart and the CLOSED lists (l0_lg_close) go up
//                               in a block of their own; the launch is l0_local_group_kernel; a winner is polished on every column of
//                               the groups in cl(S) (l0_ls_polish_on; l0_fetch_rows fetches those groups' rows only); the objective
//                               is quad + alpha |cl(S)| of the coefficients that go back; six status words (L0_LG_STATS); mode 9
//   slm_solve_l0_local_l1       the FIFTH kind (L0_LOCAL_L1): cells (alpha, l1, ridge); the check is l0_l1l_check; the l1 weights go up
//                               behind the eliminated c; the launch is l0_local_l1_kernel; a winner is polished by l0_l1l_polish on
//                               its support's rows; the objective holds lam ||beta||_1; four status words; mode 10
// check (l0_lsf_check -- at one row set l0_ls_check's refusals in l0_ls_check's order -- and the dataset's shape, before a device
// is touched); the Grams FILED, not fetched: as in solve_l0_profile_grid_impl (one slm_dataset_covariance_folds call when every
// row set brings its weights, else one by one; found again by fingerprint), each HELD for the call, so that a later build
// cannot push it out from under the kernel, which reads it in place with the dataset's leading dimension and puts 2 eta on the
// diagonal itself; with an intercept the ones column (last, alone in its group) is eliminated per row set: the vectors on the
// host (l0_eliminate_vectors, from the last row of each Gram), the matrices by one launch of l0_eliminate_kernel into a
// workspace of count * ps * ld doubles; ONE launch of l0_local_kernel over every (row set, cell, start) problem; per (row set,
// cell) the best start by (F, then the lowest index), polished (l0_ls_polish) on host copies of ONLY the rows of its Gram that
// the winners of that row set hold (l0_fetch_rows: the polish and the loss read nothing else; the whole Gram, 8 MB at 1024
// columns, never comes to the host); stat_out: the status words of EVERY problem; the record, per (row set, cell):
//
//   n_iter    rejects   resid                       mu                    kkt             L       mode
//   sweeps    swaps     the winner's status word    the objective before  the objective   -inf    8
//   of the    accepted  (1: a descent ran out of    the polish (the       after it        (no
//   winner    (winner)  sweeps, 2: the swap cap)    kernel's F)                           bound)
//
// status is SLM_OK where the winner reached its fixed point and SLM_ERR_NOT_CONVERGED where a cap ended it; beta_norm and
// loss as for solve_l0.  Nothing here is proven optimal, whatever the status.  Non-finite data is refused where it shows:
// X^T y before the launch, the winners' Gram rows after it.
static_assert(SLM_L0_LOCAL_PMAX == L0_LS_PMAX && SLM_L0_LOCAL_MAX_PROBLEMS == L0_LS_MAX_PROBLEMS, "the header and the host logic name one set of limits");
enum L0LocalKind { L0_LOCAL_ONE, L0_LOCAL_SETS, L0_LOCAL_SIZES, L0_LOCAL_GROUPS, L0_LOCAL_L1 };  // slm_solve_l0_local[_descent]; _folds; _subsets; _groups; _l1
struct L0LocalGroups {  // what only slm_solve_l0_local_groups brings: the direct need lists (CSR over the search groups) and cl(S) out
  const int32_t *need_ptr, *need_idx;
  int32_t* group_support_out;
};
int solve_l0_local_folds_impl(L0LocalKind kind, slm_dataset* ds, int32_t count, const double* const* row_weights, const int64_t* n_effs,
                              int32_t intercept, int32_t n_cells, const double* alphas, const int32_t* sizes, const double* etas, double big_M,
                              int32_t n_starts, const double* starts, int32_t swaps, double* beta_out, double* intercept_out,
                              double* objective_out, int32_t* start_out, int32_t* stat_out, slm_point_info* info,
                              const L0LocalGroups* lg = nullptr, const double* l1s = nullptr);

// slm_solve_l0_local, slm_solve_l0_local_descent: the body below on one row set, the dataset's own rows
int solve_l0_local_impl(int32_t swaps, slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas, double big_M,
                        int32_t n_starts, const double* starts, double* beta_out, double* objective_out, int32_t* start_out,
                        slm_point_info* info) {
  const double* const own_rows[1] = {nullptr};
  const int64_t n_eff[1] = {0};
  return solve_l0_local_folds_impl(L0_LOCAL_ONE, ds, 1, own_rows, n_eff, 0, n_cells, alphas, nullptr, etas, big_M, n_starts, starts, swaps,
                                   beta_out, nullptr, objective_out, start_out, nullptr, info);
}

int solve_l0_local_folds_impl(L0LocalKind kind, slm_dataset* ds, int32_t count, const double* const* row_weights, const int64_t* n_effs,
                              int32_t intercept, int32_t n_cells, const double* alphas, const int32_t* sizes, const double* etas, double big_M,
                              int32_t n_starts, const double* starts, int32_t swaps, double* beta_out, double* intercept_out,
                              double* objective_out, int32_t* start_out, int32_t* stat_out, slm_point_info* info,
                              const L0LocalGroups* lg, const double* l1s) {
  if (!ds || !beta_out || !objective_out) return fail(SLM_ERR_BAD_ARG, "NULL argument");
  const bool card = kind == L0_LOCAL_SIZES, one = kind == L0_LOCAL_ONE, grouped = kind == L0_LOCAL_GROUPS, l1 = kind == L0_LOCAL_L1;
  if (grouped && !lg) return fail(SLM_ERR_BAD_ARG, "NULL argument");
  const int drop = intercept != 0 ? 1 : 0;
  bool alone = ds->p >= 1;  // the ones column: last, alone in the last group
  if (drop && !ds->singleton) {
    const int G = ds->G;
    alone = alone && G >= 1;
    for (int64_t j = 0; j < ds->p && alone && !ds->h_gid.empty(); ++j) alone = (ds->h_gid[(size_t)j] == G - 1) == (j == ds->p - 1);
  }
  static_assert(sizeof(long long) == sizeof(int64_t), "n_effs goes to the host logic as it is");
  static_assert(sizeof(int) == sizeof(int32_t), "sizes goes to the host logic and to the kernel as it is");
  L0LsfRefusal R;
  if (card) {
    const L0LcRefusal C = l0_lc_check(count, row_weights, reinterpret_cast<const long long*>(n_effs), ds->n, drop != 0, alone, n_cells, sizes,
                                      etas, big_M, n_starts, starts, ds->p);
    switch (C.kind) {
      case L0_LC_OK: break;
      case L0_LC_NULL: return fail(SLM_ERR_BAD_ARG, "NULL argument");
      case L0_LC_SIZE: return fail(SLM_ERR_BAD_ARG, "sizes[%lld] must be >= 1 (got %d)", C.which, sizes[C.which]);
      case L0_LC_ETA: return fail(SLM_ERR_BAD_ARG, "etas[%lld] must be finite and >= 0", C.which);
      case L0_LC_LSF: break;
    }
    R = C.lsf;
  } else if (l1) {
    const L0L1lRefusal C = l0_l1l_check(count, row_weights, reinterpret_cast<const long long*>(n_effs), ds->n, drop != 0, alone, n_cells, alphas,
                                        l1s, etas, big_M, n_starts, starts, ds->p);
    switch (C.kind) {
      case L0_L1L_OK: break;
      case L0_L1L_NULL: return fail(SLM_ERR_BAD_ARG, "NULL argument");
      case L0_L1L_L1: return fail(SLM_ERR_BAD_ARG, "l1s[%lld] must be finite and >= 0", C.which);
      case L0_L1L_RIDGE: return fail(SLM_ERR_BAD_ARG, "ridges[%lld] must be finite and >= 0", C.which);
      case L0_L1L_LSF: break;
    }
    R = C.lsf;
  } else {
    R = l0_lsf_check(count, row_weights, reinterpret_cast<const long long*>(n_effs), ds->n, drop != 0, alone, n_cells, alphas, etas, big_M,
                     n_starts, starts, ds->p);
  }
  switch (R.kind) {
    case L0_LSF_OK: break;
    case L0_LSF_NULL: return fail(SLM_ERR_BAD_ARG, "NULL argument");
    case L0_LSF_COUNT: return fail(SLM_ERR_BAD_ARG, "count must be 1 .. %d, the Gram store's capacity (got %d)", L0_LS_ROW_SETS, count);
    case L0_LSF_PRODUCT:
      if (one) return fail(SLM_ERR_BAD_ARG, "n_cells * n_starts must be at most %d problems (got %d x %d)", L0_LS_MAX_PROBLEMS, n_cells, n_starts);
      return fail(SLM_ERR_BAD_ARG, "count * n_cells * n_starts must be at most %d problems (got %d x %d x %d)", L0_LS_MAX_PROBLEMS, count,
                  n_cells, n_starts);
    case L0_LSF_INTERCEPT: return fail(SLM_ERR_BAD_ARG, "intercept: the last column must be alone in the last group");
    case L0_LSF_WEIGHT: return fail(SLM_ERR_BAD_ARG, "row_weights[%d][%lld] must be finite and >= 0", R.row_set, R.which);
    case L0_LSF_LS:
      switch (R.ls) {
        case L0_LS_CELLS: return fail(SLM_ERR_BAD_ARG, "n_cells must be >= 1 (got %d)", n_cells);
        case L0_LS_STARTS: return fail(SLM_ERR_BAD_ARG, "n_starts must be >= 1 (got %d)", n_starts);
        case L0_LS_BIG_M: return fail(SLM_ERR_BAD_ARG, "big_M must be >= 0");
        case L0_LS_ALPHA: return fail(SLM_ERR_BAD_ARG, "alphas[%lld] must be finite and >= 0", R.which);
        case L0_LS_ETA: return fail(SLM_ERR_BAD_ARG, "etas[%lld] must be finite and >= 0", R.which);
        case L0_LS_WIDTH:
          return fail(SLM_ERR_UNSUPPORTED, "the l0 local search takes up to %d columns%s (got %lld)", L0_LS_PMAX,
                      drop ? " beside the intercept's" : "", (long long)ds->p - drop);
        case L0_LS_START_BOX:
          return fail(SLM_ERR_BAD_ARG, "starts[%lld] lies outside the box |beta_j| <= big_M = %g (or is not a number)", R.which, big_M);
        default: return fail(SLM_ERR_BAD_ARG, "NULL argument");
      }
  }
  if (!grouped && !ds->singleton)
    return fail(SLM_ERR_UNSUPPORTED, "the l0 local search is not built for groups: every column must be its own group");
  // (the grouped kind alone goes on with groups: l0_lg_check repeats the check above, which has passed, and decides the rest)
  int ngs = (int)ds->p - drop;  // the groups of the searched columns
  std::vector<int> gstart, cptr, cidx;
  if (grouped) {
    const int* gid = ds->singleton || ds->h_gid.empty() ? nullptr : ds->h_gid.data();
    const L0LgRefusal Q = l0_lg_check(count, row_weights, reinterpret_cast<const long long*>(n_effs), ds->n, drop != 0, alone, n_cells, alphas,
                                      etas, big_M, n_starts, starts, ds->p, gid, lg->need_ptr, lg->need_idx, row_sharded(ds), &ngs);
    switch (Q.kind) {
      case L0_LG_OK: break;
      case L0_LG_ORDER:
        return fail(SLM_ERR_UNSUPPORTED, "the grouped l0 local search takes groups that are contiguous and ascending in column order "
                    "(column %lld breaks it): the caller must order the columns by group", Q.which);
      case L0_LG_NEED_PTR: return fail(SLM_ERR_BAD_ARG, "need_ptr must start at 0 and never fall (entry %lld)", Q.which);
      case L0_LG_NEED_IDX: return fail(SLM_ERR_BAD_ARG, "need_idx[%lld] must name one of the %d search groups", Q.which, ngs);
      case L0_LG_SHARDED: break;  // (in the family's words, below)
      default: return fail(SLM_ERR_BAD_ARG, "NULL argument");
    }
  }
  if (row_sharded(ds)) return fail(SLM_ERR_UNSUPPORTED, "the l0 local search is not built for row-sharded datasets");
  if (grouped) {
    const int psearch = (int)ds->p - drop;
    gstart.assign((size_t)ngs + 1, psearch);
    for (int j = psearch - 1; j >= 0; --j) gstart[(size_t)(ds->singleton || ds->h_gid.empty() ? j : ds->h_gid[(size_t)j])] = j;
    l0_lg_close(ngs, lg->need_ptr, lg->need_idx, cptr, cidx);
  }
  const int p = (int)ds->p, ps = p - drop, per_set = n_cells * n_starts, problems = count * per_set;
  const std::vector<double> no_ridge(l1 && !etas ? (size_t)n_cells : 0, 0.0);  // (the l1 kind: ridges == NULL is no ridge)
  if (l1 && !etas) etas = no_ridge.data();
  const int64_t n = ds->n;
  const size_t ld = (size_t)ds->ld;
  slm_engine* eng = ds->eng;
  HIP_TRY(hipSetDevice(eng->device));
  hipStream_t s = eng->stream;

  // ---- the Grams: the folds' in one call when every row set brings its weights, else one by one; each held for the call ----------
  bool all_given = true, any_given = false;
  for (int b = 0; b < count; ++b) {
    all_given = all_given && row_weights[b] != nullptr;
    any_given = any_given || row_weights[b] != nullptr;
  }
  struct Weights {  // (the given weights on the device; nothing where no row set brings any)
    double* dev = nullptr;
    hipStream_t s;
    ~Weights() {
      if (!dev) return;
      (void)hipStreamSynchronize(s);
      dfree(dev);
    }
  } wts;
  wts.s = s;
  if (any_given) SLM_TRY(dalloc(&wts.dev, (size_t)count * (size_t)n));
  std::vector<const double*> wdev((size_t)count);
  std::vector<double> neff((size_t)count);
  for (int b = 0; b < count; ++b) {
    neff[(size_t)b] = row_weights[b] && n_effs[b] > 0 ? (double)n_effs[b] : (double)ds->n_global;
    wdev[(size_t)b] = ds->rw;
    if (!row_weights[b]) continue;
    wdev[(size_t)b] = wts.dev + (size_t)b * (size_t)n;
    HIP_TRY(hipMemcpyAsync(wts.dev + (size_t)b * (size_t)n, row_weights[b], sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
  }
  if (all_given) SLM_TRY(slm_dataset_covariance_folds(ds, row_weights, n_effs, count));
  std::vector<slm_dataset::CovEntry> held((size_t)count);  // (a copy holds the entry's blocks: the store may drop it, the memory stays)
  SLM_TRY(l0_local_hold_grams(ds, count, row_weights, n_effs, wdev.data(), neff.data(), held.data()));

  // ---- per row set: c on the host (the polish reads it); with an intercept the last row of G too, and the eliminated vectors ---------
  std::vector<double> ch((size_t)count * p), last((size_t)count * p), cs((size_t)count * ld, 0.0), xmean((size_t)count * ps, 0.0);
  std::vector<double> ymean((size_t)count, 0.0), yy((size_t)count, 0.0);
  for (int b = 0; b < count; ++b) {
    HIP_TRY(hipMemcpyAsync(ch.data() + (size_t)b * p, held[(size_t)b].c, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, s));
    if (drop)
      HIP_TRY(hipMemcpyAsync(last.data() + (size_t)b * p, held[(size_t)b].G + (size_t)ps * ld, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  for (double v : ch)
    if (!std::isfinite(v)) return fail(SLM_ERR_NON_FINITE, "X^T y holds a non-finite value (non-finite data)");
  for (int b = 0; b < count; ++b) {
    yy[(size_t)b] = held[(size_t)b].yy;
    if (!drop) continue;
    const double* g1 = last.data() + (size_t)b * p;
    for (int j = 0; j < p; ++j)
      if (!std::isfinite(g1[j])) return fail(SLM_ERR_NON_FINITE, "the Gram holds a non-finite value (non-finite data)");
    if (!l0_eliminate_vectors(g1, g1[ps], ch.data() + (size_t)b * p, ps, held[(size_t)b].yy, cs.data() + (size_t)b * ld, &yy[(size_t)b],
                              xmean.data() + (size_t)b * ps, &ymean[(size_t)b]))
      return fail(SLM_ERR_BAD_ARG, "intercept: row set %d gives the last column no weight", b);
  }
  // (what the kernel and the polish take for row set b's c: the eliminated vector, or the store's)
  auto c_host = [&](int b) { return drop ? cs.data() + (size_t)b * ld : ch.data() + (size_t)b * p; };

  // ---- one block: alphas | etas | starts | the eliminated c, then what comes back: F | the four status words | beta; the workspace --------
  // (the cardinality rule: the sizes, as ints, lie where the alphas did; six status words)
  const int nstat = card ? 6 : (grouped ? L0_LG_STATS : 4);
  const size_t n_start_words = starts ? (size_t)problems * ps : 0, n_c_words = drop ? (size_t)count * ld : 0;
  // (the l1 kind: its l1 weights last of what goes up, so that every other kind keeps its block)
  const size_t n_l1_words = l1 ? (size_t)n_cells : 0;
  const size_t off_eta = (size_t)n_cells, off_st = 2 * (size_t)n_cells, off_c = off_st + n_start_words, off_l1 = off_c + n_c_words,
               off_F = off_l1 + n_l1_words,
               off_stat = off_F + (size_t)problems, off_beta = off_stat + ((size_t)nstat * problems + 1) / 2, words = off_beta + (size_t)problems * ps;
  const size_t ws_stride = (size_t)ps * ld;
  std::vector<double> h(words, 0.0);
  if (card)
    memcpy(h.data(), sizes, sizeof(int32_t) * (size_t)n_cells);
  else
    memcpy(h.data(), alphas, sizeof(double) * (size_t)n_cells);
  memcpy(h.data() + off_eta, etas, sizeof(double) * (size_t)n_cells);
  if (starts) memcpy(h.data() + off_st, starts, sizeof(double) * n_start_words);
  if (drop) memcpy(h.data() + off_c, cs.data(), sizeof(double) * n_c_words);
  if (l1) memcpy(h.data() + off_l1, l1s, sizeof(double) * n_l1_words);
  unsigned long long *dev = nullptr, *ws = nullptr, *gtab = nullptr;
  L0DevGuard guard{dev, s}, ws_guard{ws, s}, gtab_guard{gtab, s};
  SLM_TRY(dalloc(&dev, words));
  if (drop) SLM_TRY(dalloc(&ws, (size_t)count * ws_stride));
  // (the grouped kind: gstart | the closed lists' cptr | cidx, as ints in a block of their own)
  std::vector<int> gh;
  if (grouped) {
    gh.insert(gh.end(), gstart.begin(), gstart.end());
    gh.insert(gh.end(), cptr.begin(), cptr.end());
    gh.insert(gh.end(), cidx.begin(), cidx.end());
    gh.push_back(0);  // (cidx is never an empty pointer)
    SLM_TRY(dalloc(&gtab, (gh.size() + 1) / 2));
    HIP_TRY(hipMemcpyAsync(gtab, gh.data(), sizeof(int) * gh.size(), hipMemcpyHostToDevice, s));
  }
  double *dd = reinterpret_cast<double*>(dev), *wd = reinterpret_cast<double*>(ws);
  std::vector<const double*> Gdev((size_t)count);
  {
    HIP_TRY(hipMemcpyAsync(dd, h.data(), sizeof(double) * off_F, hipMemcpyHostToDevice, s));
    L0LsArgs k;
    memset(&k, 0, sizeof(k));
    if (drop) {
      L0ElimArgs e;
      memset(&e, 0, sizeof(e));
      for (int b = 0; b < count; ++b) e.G[b] = held[(size_t)b].G;
      e.out = wd;
      e.ld = (long long)ld;
      e.stride = (long long)ws_stride;
      e.ps = ps;
      if (ps > 0) {
        const unsigned bx = (unsigned)std::min<size_t>(4, (ld + 255) / 256);
        hipLaunchKernelGGL(l0_eliminate_kernel, dim3(bx, (unsigned)ps, (unsigned)count), dim3(256), 0, s, e);
        SLM_TRY(check_launch());
      }
    }
    for (int b = 0; b < count; ++b) {
      Gdev[(size_t)b] = drop ? wd + (size_t)b * ws_stride : held[(size_t)b].G;
      k.G[b] = Gdev[(size_t)b];
      k.c[b] = drop ? dd + off_c + (size_t)b * ld : held[(size_t)b].c;
      k.yy[b] = yy[(size_t)b];
    }
    k.ld = (long long)ld;
    k.alphas = card ? nullptr : dd;
    k.sizes = card ? reinterpret_cast<const int*>(dd) : nullptr;
    k.stat_stride = nstat;
    k.etas = dd + off_eta;
    k.starts = starts ? dd + off_st : nullptr;
    k.F_out = dd + off_F;
    k.stat_out = reinterpret_cast<int*>(dd + off_stat);
    k.beta_out = dd + off_beta;
    k.p = ps; k.n_problems = problems; k.n_starts = n_starts; k.swaps = swaps ? 1 : 0; k.n_cells = n_cells;
    k.big_M = big_M;
    // (a problem is one wave.  The kernel's registers leave one workgroup of L0_WAVES waves resident per CU; twice that many are
    // launched so that a CU whose problems end early takes up another workgroup, and the problems beyond 2 cus workgroups are reached
    // by the kernel's grid-stride loop)
    const int blocks = std::min((problems + L0_WAVES - 1) / L0_WAVES, std::max(1, 2 * eng->cus));
    if (grouped) {
      L0LgArgs g;
      memset(&g, 0, sizeof(g));
      for (int b = 0; b < count; ++b) {
        g.G[b] = k.G[b];
        g.c[b] = k.c[b];
        g.yy[b] = k.yy[b];
      }
      g.alphas = k.alphas; g.etas = k.etas; g.starts = k.starts;
      g.gstart = reinterpret_cast<const int*>(gtab);
      g.cptr = g.gstart + (ngs + 1);
      g.cidx = g.cptr + (ngs + 1);
      g.beta_out = k.beta_out; g.F_out = k.F_out; g.stat_out = k.stat_out;
      g.ld = k.ld;
      g.p = ps; g.ng = ngs; g.n_problems = problems; g.n_starts = n_starts; g.swaps = k.swaps; g.n_cells = n_cells;
      g.big_M = big_M;
      hipLaunchKernelGGL(l0_local_group_kernel, dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, g);
    } else if (l1) {
      L0LsL1Args kl;
      memset(&kl, 0, sizeof(kl));
      static_cast<L0LsArgs&>(kl) = k;
      kl.l1s = dd + off_l1;
      hipLaunchKernelGGL(l0_local_l1_kernel, dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, kl);
    } else if (!card)
      hipLaunchKernelGGL(l0_local_kernel<false>, dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, k);
    else
      hipLaunchKernelGGL(l0_local_kernel<true>, dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, k);
    SLM_TRY(check_launch());
    HIP_TRY(hipMemcpyAsync(h.data() + off_F, dd + off_F, sizeof(double) * (words - off_F), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  const int* stat = reinterpret_cast<const int*>(h.data() + off_stat);
  if (stat_out) memcpy(stat_out, stat, sizeof(int32_t) * (size_t)nstat * (size_t)problems);

  // ---- per (row set, cell): the best start; per row set the rows its winners hold, and on them the polish and the record -----------
  int unconverged = 0, first_set = -1, first_cell = -1;
  std::vector<int> win((size_t)n_cells), rows, at((size_t)std::max(ps, 1));
  std::vector<double> Grows, Gc, cc, bc;
  std::vector<int> closed((size_t)std::max(ngs, 1), 0);  // (the grouped kind: cl(S) of a winner)
  for (int b = 0; b < count; ++b) {
    std::vector<char> used((size_t)std::max(ps, 1), 0);
    for (int cell = 0; cell < n_cells; ++cell) {
      const size_t q0 = (size_t)l0_lsf_index(b, cell, 0, n_cells, n_starts);
      int w = 0;
      for (int st = 1; st < n_starts; ++st)
        if (h[off_F + q0 + st] < h[off_F + q0 + w]) w = st;  // (ties: the lowest index)
      win[(size_t)cell] = w;
      const double* beta = h.data() + off_beta + (q0 + w) * ps;
      for (int j = 0; j < ps && !grouped; ++j) used[(size_t)j] = used[(size_t)j] || beta[j] != 0.0;
      if (grouped) {  // every column of the groups in cl(S): the polish may use them all
        l0_lg_closure(beta, ngs, gstart.data(), cptr.data(), cidx.data(), closed.data());
        for (int g = 0; g < ngs; ++g)
          for (int j = gstart[(size_t)g]; j < gstart[(size_t)g + 1] && closed[(size_t)g]; ++j) used[(size_t)j] = 1;
      }
    }
    rows.clear();
    for (int j = 0; j < ps; ++j)
      if (used[(size_t)j]) {
        at[(size_t)j] = (int)rows.size();
        rows.push_back(j);
      }
    const int m = (int)rows.size();
    SLM_TRY(l0_fetch_rows(s, Gdev[(size_t)b], ld, ps, rows, Grows));
    for (double v : Grows)
      if (!std::isfinite(v)) return fail(SLM_ERR_NON_FINITE, "the Gram holds a non-finite value (non-finite data)");
    // the Gram on those columns alone, in their order: the polish and the loss read entries between non-zeros only
    Gc.assign((size_t)m * m, 0.0);
    cc.assign((size_t)m, 0.0);
    bc.assign((size_t)m, 0.0);
    for (int a = 0; a < m; ++a) {
      cc[(size_t)a] = c_host(b)[rows[(size_t)a]];
      for (int k2 = 0; k2 < m; ++k2) Gc[(size_t)a * m + k2] = Grows[(size_t)a * ps + rows[(size_t)k2]];
    }
    for (int cell = 0; cell < n_cells; ++cell) {
      const size_t rc = (size_t)b * n_cells + cell, q = (size_t)l0_lsf_index(b, cell, win[(size_t)cell], n_cells, n_starts);
      double* beta = beta_out + rc * ps;
      memcpy(beta, h.data() + off_beta + q * ps, sizeof(double) * (size_t)ps);
      for (int a = 0; a < m; ++a) bc[(size_t)a] = beta[rows[(size_t)a]];
      double quad = 0.0;
      if (l1) {  // (quad holds the l1 term too: objective_out = quad + alpha nnz of the coefficients that go back, as below)
        quad = l0_l1l_polish(Gc.data(), (size_t)m, cc.data(), m, etas[cell], l1s[cell], big_M, bc.data());
      } else if (!grouped) {
        quad = l0_ls_polish(Gc.data(), (size_t)m, cc.data(), m, etas[cell], big_M, bc.data());
      } else {
        // on ALL columns of the groups in cl(S) -- a group that is only held is free to use -- but for those the rule leaves out
        l0_lg_closure(beta, ngs, gstart.data(), cptr.data(), cidx.data(), closed.data());
        double dmax = 0.0;
        for (int a = 0; a < m; ++a) dmax = std::max(dmax, Gc[(size_t)a * m + a] + 2.0 * etas[cell]);
        std::vector<int> on;
        int g = 0;
        for (int a = 0; a < m; ++a) {
          while (gstart[(size_t)g + 1] <= rows[(size_t)a]) ++g;
          if (closed[(size_t)g] && (bc[(size_t)a] != 0.0 || Gc[(size_t)a * m + a] + 2.0 * etas[cell] > L0_PIVOT * dmax)) on.push_back(a);
        }
        quad = l0_ls_polish_on(Gc.data(), (size_t)m, cc.data(), etas[cell], big_M, on, bc.data());
      }
      int nnz = 0;
      double bn = 0.0, dot = 0.0;
      for (int a = 0; a < m; ++a) beta[rows[(size_t)a]] = bc[(size_t)a];
      for (int j = 0; j < ps; ++j) {
        nnz += beta[j] != 0.0;
        bn += beta[j] * beta[j];
        if (drop) dot += xmean[(size_t)b * ps + j] * beta[j];
      }
      objective_out[rc] = card ? quad : quad + alphas[cell] * (double)nnz;
      if (grouped) {  // alpha |cl(S)| of the coefficients that go back
        const int ncl = l0_lg_closure(beta, ngs, gstart.data(), cptr.data(), cidx.data(), closed.data());
        objective_out[rc] = quad + alphas[cell] * (double)ncl;
        if (lg->group_support_out) memcpy(lg->group_support_out + rc * (size_t)ngs, closed.data(), sizeof(int32_t) * (size_t)ngs);
      }
      if (intercept_out) intercept_out[rc] = drop ? ymean[(size_t)b] - dot : 0.0;
      if (start_out) start_out[rc] = win[(size_t)cell];
      const bool done = stat[nstat * q + 2] == 0;
      if (!done && unconverged++ == 0) {
        first_set = b;
        first_cell = cell;
      }
      if (info) {
        l0_report(info + rc, done, l0_gram_loss(Gc.data(), cc.data(), m, yy[(size_t)b], bc.data()), objective_out[rc], h[off_F + q], -HUGE_VAL);
        info[rc].n_iter = stat[nstat * q + 0];
        info[rc].rejects = stat[nstat * q + 1];
        info[rc].resid = (double)stat[nstat * q + 2];
        info[rc].beta_norm = std::sqrt(bn);
        info[rc].mode = grouped ? 9 : (l1 ? 10 : 8);
      }
    }
  }
  if (unconverged && one)
    return fail(SLM_ERR_NOT_CONVERGED, "the local search reached a cap (%d sweeps per descent, %d swaps) in %d of %d cells (the first: %d): "
                "their last points are returned", L0_CD_SWEEPS, L0_LS_SWAPS, unconverged, n_cells, first_cell);
  if (unconverged)
    return fail(SLM_ERR_NOT_CONVERGED, "the local search reached a cap (%d sweeps per descent, %d swaps) in %d of %d (row set, cell) pairs "
                "(the first: row set %d, cell %d): their last points are returned", L0_CD_SWEEPS, L0_LS_SWAPS, unconverged, count * n_cells,
                first_set, first_cell);
  return SLM_OK;
}

// The local bound (DESIGN 4d "Local bound"; the mathematics: l0_host.hpp "local bound"): for every cell a PROVEN lower bound on the
// objective slm_solve_l0_local minimises, from one launch of l0_local_bound_kernel (csrc/l0_local_bound_kernels.hpp), one
// wavefront per cell.  The check (l0_bound_check, and the dataset's shape) comes before a device is touched; big_M = 0 leaves
// beta = 0 alone, whose objective 0 is the bound, and launches nothing.  The dataset's own rows, their Gram filed and held as
// for the local search (l0_local_hold_grams) and read in place; lam and tauc of every cell are the host's (l0_lb_cell) and go
// up beside the alphas and etas.  What comes back is a bound whatever the status: the status says only whether the relaxation
// was closed.  The record, per cell:
//
//   n_iter    resid                          mu        L           kkt    mode
//   sweeps    the status word (1: the        P(u)      the bound   P - L  11
//             sweeps ran out)
int solve_l0_local_bound_impl(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas, double big_M, const double* starts,
                              int32_t max_sweeps, double gap_tol, double* lower_out, double* primal_out, double* u_out, int32_t* stat_out,
                              slm_point_info* info) {
  if (!ds || !lower_out) return fail(SLM_ERR_BAD_ARG, "NULL argument");
  long long which = 0;
  switch (l0_bound_check(n_cells, alphas, etas, big_M, starts, ds->p, gap_tol, ds->singleton, row_sharded(ds), &which)) {
    case L0_LB_OK: break;
    case L0_LB_NULL: return fail(SLM_ERR_BAD_ARG, "NULL argument");
    case L0_LB_CELLS: return fail(SLM_ERR_BAD_ARG, "n_cells must be >= 1 (got %d)", n_cells);
    case L0_LB_PROBLEMS: return fail(SLM_ERR_BAD_ARG, "n_cells must be at most %d cells (got %d)", L0_LS_MAX_PROBLEMS, n_cells);
    case L0_LB_BIG_M: return fail(SLM_ERR_BAD_ARG, "big_M must be >= 0");
    case L0_LB_ALPHA: return fail(SLM_ERR_BAD_ARG, "alphas[%lld] must be finite and >= 0", which);
    case L0_LB_ETA: return fail(SLM_ERR_BAD_ARG, "etas[%lld] must be finite and >= 0", which);
    case L0_LB_GAP_TOL: return fail(SLM_ERR_BAD_ARG, "gap_tol must be >= 0");
    case L0_LB_WIDTH: return fail(SLM_ERR_UNSUPPORTED, "the l0 local bound takes up to %d columns (got %lld)", L0_LS_PMAX, (long long)ds->p);
    case L0_LB_START: return fail(SLM_ERR_BAD_ARG, "starts[%lld] is not a finite number", which);
    case L0_LB_GROUPS: return fail(SLM_ERR_UNSUPPORTED, "the l0 local bound is not built for groups: every column must be its own group");
    case L0_LB_SHARDED: return fail(SLM_ERR_UNSUPPORTED, "the l0 local bound is not built for row-sharded datasets");
  }
  const int p = (int)ds->p, sweeps_cap = max_sweeps > 0 ? max_sweeps : L0_LB_SWEEPS;
  auto record = [&](int e, double lower, double primal, int sweeps, int status) {
    lower_out[e] = lower;
    if (primal_out) primal_out[e] = primal;
    if (stat_out) {
      stat_out[2 * e] = sweeps;
      stat_out[2 * e + 1] = status;
    }
    if (!info) return;
    l0_report(info + e, status == 0, 0.0, primal - lower, primal, lower);
    info[e].n_iter = sweeps;
    info[e].resid = (double)status;
    info[e].mode = L0_LB_MODE;
  };
  if (big_M == 0.0) {  // the box holds beta = 0 alone: F = 0 is the optimum and the bound
    if (u_out) std::fill(u_out, u_out + (size_t)n_cells * p, 0.0);
    for (int e = 0; e < n_cells; ++e) record(e, 0.0, 0.0, 0, 0);
    return SLM_OK;
  }
  const size_t ld = (size_t)ds->ld;
  slm_engine* eng = ds->eng;
  HIP_TRY(hipSetDevice(eng->device));
  hipStream_t s = eng->stream;

  // ---- the Gram of the dataset's own rows: found or filed, held for the call ------------------------------------------------------
  const double* const own_rows[1] = {nullptr};
  const int64_t n_eff[1] = {0};
  const double* const wdev[1] = {ds->rw};
  const double neff[1] = {(double)ds->n_global};
  slm_dataset::CovEntry held;
  SLM_TRY(l0_local_hold_grams(ds, 1, own_rows, n_eff, wdev, neff, &held));
  std::vector<double> ch((size_t)p);
  HIP_TRY(hipMemcpyAsync(ch.data(), held.c, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (double v : ch)
    if (!std::isfinite(v)) return fail(SLM_ERR_NON_FINITE, "X^T y holds a non-finite value (non-finite data)");

  // ---- one block: alphas | etas | lams | taus | starts, then what comes back: lower | primal | the two status words | u -------------
  const size_t nc = (size_t)n_cells, n_start_words = starts ? nc * p : 0;
  const size_t off_eta = nc, off_lam = 2 * nc, off_tau = 3 * nc, off_st = 4 * nc, off_low = off_st + n_start_words, off_pri = off_low + nc,
               off_stat = off_pri + nc, off_u = off_stat + nc, words = off_u + nc * p;
  std::vector<double> h(words, 0.0);
  memcpy(h.data(), alphas, sizeof(double) * nc);
  memcpy(h.data() + off_eta, etas, sizeof(double) * nc);
  for (size_t e = 0; e < nc; ++e) {
    const L0LbCell cell = l0_lb_cell(alphas[e], etas[e], big_M);
    h[off_lam + e] = cell.lam;
    h[off_tau + e] = cell.tauc;
  }
  if (starts) memcpy(h.data() + off_st, starts, sizeof(double) * n_start_words);
  unsigned long long* dev = nullptr;
  L0DevGuard guard{dev, s};
  SLM_TRY(dalloc(&dev, words));
  double* dd = reinterpret_cast<double*>(dev);
  HIP_TRY(hipMemcpyAsync(dd, h.data(), sizeof(double) * off_low, hipMemcpyHostToDevice, s));
  L0LbArgs k;
  memset(&k, 0, sizeof(k));
  k.G = held.G;
  k.c = held.c;
  k.alphas = dd;
  k.etas = dd + off_eta;
  k.lams = dd + off_lam;
  k.taus = dd + off_tau;
  k.starts = starts ? dd + off_st : nullptr;
  k.lower_out = dd + off_low;
  k.primal_out = dd + off_pri;
  k.stat_out = reinterpret_cast<int*>(dd + off_stat);
  k.u_out = dd + off_u;
  k.ld = (long long)ld;
  k.p = p; k.n_cells = n_cells; k.max_sweeps = sweeps_cap;
  k.big_M = big_M; k.gap_tol = gap_tol;
  // (a cell is one wave; the grid as for the local search: up to two workgroups a CU, the cells beyond by the grid-stride loop)
  const int blocks = std::min((n_cells + L0_WAVES - 1) / L0_WAVES, std::max(1, 2 * eng->cus));
  hipLaunchKernelGGL(l0_local_bound_kernel, dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, k);
  SLM_TRY(check_launch());
  HIP_TRY(hipMemcpyAsync(h.data() + off_low, dd + off_low, sizeof(double) * (words - off_low), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const int* stat = reinterpret_cast<const int*>(h.data() + off_stat);
  if (u_out) memcpy(u_out, h.data() + off_u, sizeof(double) * nc * (size_t)p);
  int unclosed = 0, first = -1;
  for (int e = 0; e < n_cells; ++e) {
    record(e, h[off_low + (size_t)e], h[off_pri + (size_t)e], stat[2 * e], stat[2 * e + 1]);
    if (stat[2 * e + 1] != 0 && unclosed++ == 0) first = e;
  }
  if (unclosed)
    return fail(SLM_ERR_NOT_CONVERGED, "the local bound ran out of sweeps (%d) in %d of %d cells (the first: %d): the relaxation is not closed "
                "there, the values are bounds all the same", sweeps_cap, unclosed, n_cells, first);
  return SLM_OK;
}

// The local proof (DESIGN 4d "Local proof"; the mathematics, the twin and the tree: l0_host.hpp "local proof").  L0NodeRunner is
// what both entries share: the Gram of the dataset's own rows found or filed and held as solve_l0_local_bound_impl does it
// (l0_local_hold_grams), the cells' constants on the device once, and run(): ONE launch of l0_local_node_kernel
// (csrc/l0_local_node_kernels.hpp) for a batch of nodes -- the batch up in one copy, the results back in one.  The device block
// grows with the largest batch seen.
struct L0NodeRunner {
  slm_dataset* ds = nullptr;
  hipStream_t s = nullptr;
  slm_dataset::CovEntry held;
  int p = 0, n_cells = 0, max_sweeps = 0;
  double big_M = 0.0, gap_tol = 0.0;
  unsigned long long* cells_dev = nullptr;
  unsigned long long* dev = nullptr;
  size_t dev_words = 0;
  long long launches = 0, launched_nodes = 0;
  std::vector<double> h;
  int* groups_dev = nullptr;  // the grouped entries: gof [p] | gstart [ng + 1] | cptr [ng + 1] | cidx; NULL: the column kernel
  int ng = 0;
  size_t n_cidx = 0;
  ~L0NodeRunner() {
    if (s) (void)hipStreamSynchronize(s);
    dfree(dev);
    dfree(cells_dev);
    dfree(groups_dev);
  }
  // after open(): the nodes are GROUP nodes from here on, bounded by l0_local_group_node_kernel
  int set_groups(const L0GroupMap& gm) {
    ng = gm.ng;
    n_cidx = gm.cptr ? (size_t)gm.cptr[ng] : 0;
    std::vector<int> w((size_t)p + 2 * ((size_t)ng + 1) + n_cidx, 0);
    for (int g = 0; g < ng; ++g)
      for (int j = gm.gstart[g]; j < gm.gstart[g + 1]; ++j) w[(size_t)j] = g;
    memcpy(w.data() + p, gm.gstart, sizeof(int) * ((size_t)ng + 1));
    if (gm.cptr) memcpy(w.data() + p + ng + 1, gm.cptr, sizeof(int) * ((size_t)ng + 1));
    if (n_cidx) memcpy(w.data() + p + 2 * ((size_t)ng + 1), gm.cidx, sizeof(int) * n_cidx);
    SLM_TRY(dalloc(&groups_dev, w.size()));
    HIP_TRY(hipMemcpyAsync(groups_dev, w.data(), sizeof(int) * w.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // (w leaves scope)
    return SLM_OK;
  }
  int open(slm_dataset* ds_, const L0NodeCell* cells, int n_cells_, int max_sweeps_, double gap_tol_, std::vector<double>* c_host) {
    ds = ds_;
    p = (int)ds->p; n_cells = n_cells_; max_sweeps = max_sweeps_; gap_tol = gap_tol_; big_M = cells[0].big_M;
    slm_engine* eng = ds->eng;
    HIP_TRY(hipSetDevice(eng->device));
    s = eng->stream;
    const double* const own_rows[1] = {nullptr};
    const int64_t n_eff[1] = {0};
    const double* const wdev[1] = {ds->rw};
    const double neff[1] = {(double)ds->n_global};
    SLM_TRY(l0_local_hold_grams(ds, 1, own_rows, n_eff, wdev, neff, &held));
    std::vector<double> ch((size_t)p);
    HIP_TRY(hipMemcpyAsync(ch.data(), held.c, sizeof(double) * (size_t)p, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (double v : ch)
      if (!std::isfinite(v)) return fail(SLM_ERR_NON_FINITE, "X^T y holds a non-finite value (non-finite data)");
    const size_t nc = (size_t)n_cells;
    std::vector<double> cw(4 * nc);
    for (size_t e = 0; e < nc; ++e) {
      cw[e] = cells[e].alpha;
      cw[nc + e] = cells[e].eta;
      cw[2 * nc + e] = cells[e].lam;
      cw[3 * nc + e] = cells[e].tauc;
    }
    SLM_TRY(dalloc(&cells_dev, 4 * nc));
    HIP_TRY(hipMemcpyAsync(cells_dev, cw.data(), sizeof(double) * 4 * nc, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // (cw leaves scope)
    if (c_host) *c_host = ch;
    return SLM_OK;
  }
  // one block: cell | in | out | parent | starts, then what comes back: lower | primal | upper | the two status words | u
  int run(const L0NodeBatch& b) {
    const size_t n = (size_t)b.n, W = (size_t)L0_ND_WORDS;
    const size_t off_in = (n + 1) / 2, off_out = off_in + n * W, off_par = off_out + n * W, off_st = off_par + n, off_low = off_st + n * p,
                 off_pri = off_low + n, off_up = off_pri + n, off_stat = off_up + n, off_u = off_stat + n, words = off_u + n * p;
    if (words > dev_words) {
      HIP_TRY(hipStreamSynchronize(s));
      dfree(dev);
      dev_words = 0;
      SLM_TRY(dalloc(&dev, words + words / 2));
      dev_words = words + words / 2;
    }
    h.assign(words, 0.0);
    memcpy(h.data(), b.cell, sizeof(int) * n);
    memcpy(h.data() + off_in, b.in_mask, sizeof(unsigned long long) * n * W);
    memcpy(h.data() + off_out, b.out_mask, sizeof(unsigned long long) * n * W);
    if (b.parent_lower) memcpy(h.data() + off_par, b.parent_lower, sizeof(double) * n);
    if (b.starts) memcpy(h.data() + off_st, b.starts, sizeof(double) * n * p);
    double* dd = reinterpret_cast<double*>(dev);
    HIP_TRY(hipMemcpyAsync(dd, h.data(), sizeof(double) * off_low, hipMemcpyHostToDevice, s));
    const double* cd = reinterpret_cast<const double*>(cells_dev);
    L0NdArgs k;
    memset(&k, 0, sizeof(k));
    k.G = held.G;
    k.c = held.c;
    k.alphas = cd;
    k.etas = cd + n_cells;
    k.lams = cd + 2 * (size_t)n_cells;
    k.taus = cd + 3 * (size_t)n_cells;
    k.cell = reinterpret_cast<const int*>(dd);
    k.in_mask = dev + off_in;
    k.out_mask = dev + off_out;
    k.parent_lower = b.parent_lower ? dd + off_par : nullptr;
    k.starts = b.starts ? dd + off_st : nullptr;
    k.lower_out = dd + off_low;
    k.primal_out = dd + off_pri;
    k.upper_out = dd + off_up;
    k.stat_out = reinterpret_cast<int*>(dd + off_stat);
    k.u_out = dd + off_u;
    k.ld = (long long)ds->ld;
    k.p = p; k.n_nodes = b.n; k.max_sweeps = max_sweeps;
    k.big_M = big_M; k.gap_tol = gap_tol;
    // (a node is one wave; the grid as for the bound: up to two workgroups a CU, the nodes beyond by the grid-stride loop)
    const int blocks = std::min((b.n + L0_WAVES - 1) / L0_WAVES, std::max(1, 2 * ds->eng->cus));
    if (groups_dev) {
      L0GnArgs gk;
      memset(&gk, 0, sizeof(gk));
      gk.nd = k;
      gk.gof = groups_dev;
      gk.gstart = groups_dev + p;
      gk.cptr = groups_dev + p + ng + 1;
      gk.cidx = groups_dev + p + 2 * ((size_t)ng + 1);
      gk.ng = ng;
      hipLaunchKernelGGL(l0_local_group_node_kernel, dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, gk);
    } else {
      hipLaunchKernelGGL(l0_local_node_kernel, dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, k);
    }
    SLM_TRY(check_launch());
    HIP_TRY(hipMemcpyAsync(h.data() + off_low, dd + off_low, sizeof(double) * (words - off_low), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(b.lower, h.data() + off_low, sizeof(double) * n);
    memcpy(b.primal, h.data() + off_pri, sizeof(double) * n);
    memcpy(b.upper, h.data() + off_up, sizeof(double) * n);
    memcpy(b.stat, h.data() + off_stat, sizeof(int) * 2 * n);
    memcpy(b.u, h.data() + off_u, sizeof(double) * n * p);
    ++launches;
    launched_nodes += b.n;
    return SLM_OK;
  }
};

// One batch of nodes: the kernel's entry, and what the tests compare with the twin.  The record, per node:
//
//   n_iter    resid              mu          L           kkt       loss    mode
//   sweeps    the status word    P_node(u)   the bound   F(u)      0       12
int solve_l0_local_nodes_impl(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas, double big_M, int32_t n_nodes,
                              const int32_t* cell, const unsigned long long* in_mask, const unsigned long long* out_mask,
                              const double* parent_lower, const double* starts, int32_t max_sweeps, double gap_tol, double* lower_out,
                              double* primal_out, double* upper_out, double* u_out, int32_t* stat_out, slm_point_info* info,
                              const L0GroupMap* groups = nullptr) {
  // (groups: the grouped entry, whose own check has passed; the nodes are GROUP nodes, l0_local_group_node_kernel bounds them, mode 14)
  if (!ds || !lower_out) return fail(SLM_ERR_BAD_ARG, "NULL argument");
  long long which = 0;
  switch (l0_nodes_check(n_cells, alphas, etas, big_M, n_nodes, cell, in_mask, out_mask, parent_lower, starts, ds->p, gap_tol, ds->singleton || groups, row_sharded(ds),
                         &which)) {
    case L0_ND_OK: break;
    case L0_ND_NULL: return fail(SLM_ERR_BAD_ARG, "NULL argument");
    case L0_ND_CELLS: return fail(SLM_ERR_BAD_ARG, "n_cells must be >= 1 (got %d)", n_cells);
    case L0_ND_PROBLEMS: return fail(SLM_ERR_BAD_ARG, "n_cells must be at most %d cells (got %d)", L0_LS_MAX_PROBLEMS, n_cells);
    case L0_ND_NODES: return fail(SLM_ERR_BAD_ARG, "n_nodes must be >= 1 (got %d)", n_nodes);
    case L0_ND_BATCH: return fail(SLM_ERR_BAD_ARG, "n_nodes must be at most %d nodes (got %d)", L0_ND_MAX_BATCH, n_nodes);
    case L0_ND_BIG_M: return fail(SLM_ERR_BAD_ARG, "big_M must be >= 0");
    case L0_ND_ALPHA: return fail(SLM_ERR_BAD_ARG, "alphas[%lld] must be finite and >= 0", which);
    case L0_ND_ETA: return fail(SLM_ERR_BAD_ARG, "etas[%lld] must be finite and >= 0", which);
    case L0_ND_GAP_TOL: return fail(SLM_ERR_BAD_ARG, "gap_tol must be >= 0");
    case L0_ND_WIDTH: return fail(SLM_ERR_UNSUPPORTED, "the l0 local proof takes up to %d columns (got %lld)", L0_LS_PMAX, (long long)ds->p);
    case L0_ND_CELL: return fail(SLM_ERR_BAD_ARG, "cell[%lld] is not a cell of the call", which);
    case L0_ND_MASK: return fail(SLM_ERR_BAD_ARG, "node %lld holds a column that is both IN and OUT", which);
    case L0_ND_PARENT: return fail(SLM_ERR_BAD_ARG, "parent_lower[%lld] is neither a number nor -infinity", which);
    case L0_ND_START: return fail(SLM_ERR_BAD_ARG, "starts[%lld] is not a finite number", which);
    case L0_ND_GROUPS: return fail(SLM_ERR_UNSUPPORTED, "the l0 local proof is not built for groups: every column must be its own group");
    case L0_ND_SHARDED: return fail(SLM_ERR_UNSUPPORTED, "the l0 local proof is not built for row-sharded datasets");
  }
  const int p = (int)ds->p, sweeps_cap = max_sweeps > 0 ? max_sweeps : L0_LB_SWEEPS;
  const size_t n = (size_t)n_nodes;
  std::vector<double> lower(n, 0.0), primal(n, 0.0), upper(n, 0.0), u(n * (size_t)p, 0.0);
  std::vector<int> stat(2 * n, 0);
  if (big_M != 0.0) {  // (big_M = 0: the box holds beta = 0 alone, every value is 0 and nothing is launched)
    std::vector<L0NodeCell> cells((size_t)n_cells);
    for (int e = 0; e < n_cells; ++e) cells[(size_t)e] = l0_node_cell(alphas[e], etas[e], big_M);
    L0NodeRunner run;
    SLM_TRY(run.open(ds, cells.data(), n_cells, sweeps_cap, gap_tol, nullptr));
    if (groups) SLM_TRY(run.set_groups(*groups));
    const L0NodeBatch b{n_nodes, cell, in_mask, out_mask, parent_lower, starts, lower.data(), primal.data(), upper.data(), u.data(), stat.data()};
    SLM_TRY(run.run(b));
  }
  int unclosed = 0, first = -1;
  for (int i = 0; i < n_nodes; ++i) {
    lower_out[i] = lower[(size_t)i];
    if (primal_out) primal_out[i] = primal[(size_t)i];
    if (upper_out) upper_out[i] = upper[(size_t)i];
    if (stat_out) {
      stat_out[2 * i] = stat[2 * (size_t)i];
      stat_out[2 * i + 1] = stat[2 * (size_t)i + 1];
    }
    if (stat[2 * (size_t)i + 1] != 0 && unclosed++ == 0) first = i;
    if (!info) continue;
    l0_report(info + i, stat[2 * (size_t)i + 1] == 0, 0.0, upper[(size_t)i], primal[(size_t)i], lower[(size_t)i]);
    info[i].n_iter = stat[2 * (size_t)i];
    info[i].resid = (double)stat[2 * (size_t)i + 1];
    info[i].mode = groups ? L0_GN_MODE : L0_ND_MODE;
  }
  if (u_out) memcpy(u_out, u.data(), sizeof(double) * n * (size_t)p);
  if (unclosed)
    return fail(SLM_ERR_NOT_CONVERGED, "the node relaxation ran out of sweeps (%d) in %d of %d nodes (the first: %d): it is not closed there, the "
                "values are bounds all the same", sweeps_cap, unclosed, n_nodes, first);
  return SLM_OK;
}

// The whole tree for a grid of cells: l0_prove_tree (l0_host.hpp) with the launch as its callable, one launch a round for the
// children of every cell.  The Gram comes to the host once (the tree's branching rule and the incumbent's polish read it).
// The record, per cell:
//
//   n_iter    rejects   resid                           mu               L                 kkt             mode
//   rounds    nodes     the status (1: node limit)      the incumbent    the proven bound  the objective   13
int solve_l0_local_prove_impl(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas, double big_M, const double* incumbents,
                              double rel_gap, int32_t max_nodes, int32_t width, int32_t max_sweeps, int64_t leaf_capacity, double* beta_out,
                              double* objective_out, double* lower_out, int32_t* nodes_out, int32_t* rounds_out, int32_t* status_out,
                              int32_t* leaf_cell, unsigned long long* leaf_in, unsigned long long* leaf_out, double* leaf_u, double* leaf_lower,
                              int64_t* leaf_count, slm_point_info* info, const L0GroupMap* groups = nullptr) {
  // (groups: the grouped entry, whose own check has passed; group nodes, the closure at a branch, mode 15)
  if (!ds || !beta_out || !objective_out || !lower_out) return fail(SLM_ERR_BAD_ARG, "NULL argument");
  long long which = 0;
  switch (l0_prove_check(n_cells, alphas, etas, big_M, incumbents, ds->p, rel_gap, max_nodes, width, ds->singleton || groups, row_sharded(ds), &which)) {
    case L0_PV_OK: break;
    case L0_PV_NULL: return fail(SLM_ERR_BAD_ARG, "NULL argument");
    case L0_PV_CELLS: return fail(SLM_ERR_BAD_ARG, "n_cells must be >= 1 (got %d)", n_cells);
    case L0_PV_PROBLEMS: return fail(SLM_ERR_BAD_ARG, "n_cells must be at most %d cells (got %d)", L0_LS_MAX_PROBLEMS, n_cells);
    case L0_PV_BIG_M: return fail(SLM_ERR_BAD_ARG, "big_M must be >= 0");
    case L0_PV_ALPHA: return fail(SLM_ERR_BAD_ARG, "alphas[%lld] must be finite and >= 0", which);
    case L0_PV_ETA: return fail(SLM_ERR_BAD_ARG, "etas[%lld] must be finite and >= 0", which);
    case L0_PV_REL_GAP: return fail(SLM_ERR_BAD_ARG, "rel_gap must lie in [1e-10, 1]");
    case L0_PV_MAX_NODES: return fail(SLM_ERR_BAD_ARG, "max_nodes must be >= 1 (got %d)", max_nodes);
    case L0_PV_TREE_WIDTH: return fail(SLM_ERR_BAD_ARG, "width must be >= 1 (got %d)", width);
    case L0_PV_WIDTH: return fail(SLM_ERR_UNSUPPORTED, "the l0 local proof takes up to %d columns (got %lld)", L0_LS_PMAX, (long long)ds->p);
    case L0_PV_INCUMBENT: return fail(SLM_ERR_BAD_ARG, "incumbents[%lld] is outside the box [-big_M, big_M] or not a number", which);
    case L0_PV_GROUPS: return fail(SLM_ERR_UNSUPPORTED, "the l0 local proof is not built for groups: every column must be its own group");
    case L0_PV_SHARDED: return fail(SLM_ERR_UNSUPPORTED, "the l0 local proof is not built for row-sharded datasets");
  }
  const int p = (int)ds->p, sweeps_cap = max_sweeps > 0 ? max_sweeps : L0_LB_SWEEPS;
  const bool want_leaves = leaf_capacity > 0 && leaf_cell && leaf_in && leaf_out && leaf_u && leaf_lower;
  std::vector<int> nodes((size_t)n_cells, 0), rounds((size_t)n_cells, 0), status((size_t)n_cells, L0_PV_OPTIMAL);
  L0ProveLeaves leaves;
  if (big_M == 0.0) {  // the box holds beta = 0 alone: F = 0 is the optimum, proven without a launch
    std::fill(beta_out, beta_out + (size_t)n_cells * p, 0.0);
    std::fill(objective_out, objective_out + n_cells, 0.0);
    std::fill(lower_out, lower_out + n_cells, 0.0);
  } else {
    std::vector<L0NodeCell> cells((size_t)n_cells);
    for (int e = 0; e < n_cells; ++e) cells[(size_t)e] = l0_node_cell(alphas[e], etas[e], big_M);
    L0NodeRunner run;
    std::vector<double> ch;
    SLM_TRY(run.open(ds, cells.data(), n_cells, sweeps_cap, rel_gap / 100.0, &ch));
    if (groups) SLM_TRY(run.set_groups(*groups));
    const size_t ld = (size_t)ds->ld;
    std::vector<double> Gh((size_t)p * ld);
    HIP_TRY(hipMemcpyAsync(Gh.data(), run.held.G, sizeof(double) * (size_t)p * ld, hipMemcpyDeviceToHost, run.s));
    HIP_TRY(hipStreamSynchronize(run.s));
    if (want_leaves) {
      leaves.capacity = leaf_capacity;
      leaves.cell = leaf_cell; leaves.in_mask = leaf_in; leaves.out_mask = leaf_out; leaves.u = leaf_u; leaves.lower = leaf_lower;
    }
    SLM_TRY(l0_prove_tree(Gh.data(), ld, ch.data(), p, n_cells, cells.data(), incumbents, rel_gap, max_nodes, width,
                          [&](const L0NodeBatch& b) { return run.run(b); }, beta_out, objective_out, lower_out, nodes.data(), rounds.data(),
                          status.data(), want_leaves ? &leaves : nullptr, groups));
  }
  if (leaf_count) *leaf_count = leaves.count;
  int open_cells = 0, first = -1;
  for (int e = 0; e < n_cells; ++e) {
    if (nodes_out) nodes_out[e] = nodes[(size_t)e];
    if (rounds_out) rounds_out[e] = rounds[(size_t)e];
    if (status_out) status_out[e] = status[(size_t)e];
    if (status[(size_t)e] != L0_PV_OPTIMAL && open_cells++ == 0) first = e;
    if (!info) continue;
    l0_report(info + e, status[(size_t)e] == L0_PV_OPTIMAL, 0.0, objective_out[e], objective_out[e], lower_out[e]);
    info[e].n_iter = rounds[(size_t)e];
    info[e].rejects = nodes[(size_t)e];
    info[e].resid = (double)status[(size_t)e];
    info[e].mode = groups ? L0_GP_MODE : L0_PV_MODE;
  }
  if (open_cells)
    return fail(SLM_ERR_NOT_CONVERGED, "the node limit (%d) ran out in %d of %d cells (the first: %d): the incumbent and a proven lower bound are "
                "returned there", max_nodes, open_cells, n_cells, first);
  return SLM_OK;
}

// The local proof WITH GROUPS (DESIGN 4d "Local proof with groups"; l0_host.hpp "local proof with groups").  The dataset's groups
// (contiguous and ascending, as the grouped local search takes them) and the caller's direct need lists become the map both
// entries hand on: gstart, the closed lists and their reverse.
struct L0GroupMapOwner {
  std::vector<int> gstart, cptr, cidx, rptr, ridx;
  L0GroupMap map;
  void build(const slm_dataset* ds, int ng, const int32_t* need_ptr, const int32_t* need_idx) {
    const int p = (int)ds->p;
    const bool single = ds->singleton || ds->h_gid.empty();
    gstart.assign((size_t)ng + 1, p);
    for (int j = p - 1; j >= 0; --j) gstart[(size_t)(single ? j : ds->h_gid[(size_t)j])] = j;
    l0_lg_close(ng, need_ptr, need_idx, cptr, cidx);
    l0_gp_reverse(ng, cptr, cidx, rptr, ridx);
    map.ng = ng;
    map.gstart = gstart.data();
    map.cptr = cptr.data();
    map.cidx = cidx.data();
    map.rptr = rptr.data();
    map.ridx = ridx.data();
  }
};
// the refusals the two grouped entries share, in the words of the grouped local search
int l0_gp_refuse(const L0GpRefusal& Q, int ng) {
  switch (Q.kind) {
    case L0_GP_ORDER:
      return fail(SLM_ERR_UNSUPPORTED, "the grouped l0 local proof takes groups that are contiguous and ascending in column order "
                  "(column %lld breaks it): the caller must order the columns by group", Q.which);
    case L0_GP_NEED_PTR: return fail(SLM_ERR_BAD_ARG, "need_ptr must start at 0 and never fall (entry %lld)", Q.which);
    case L0_GP_NEED_IDX: return fail(SLM_ERR_BAD_ARG, "need_idx[%lld] must name one of the %d groups", Q.which, ng);
    case L0_GP_RANGE: return fail(SLM_ERR_BAD_ARG, "node %lld fixes a group beyond the %d groups of the dataset", Q.which, ng);
    case L0_GP_UNCLOSED:
      return fail(SLM_ERR_BAD_ARG, "node %lld is not closed under the hierarchy: an IN group brings every group it needs IN, an OUT group "
                  "takes every group that needs it OUT", Q.which);
    case L0_GP_SHARDED: return fail(SLM_ERR_UNSUPPORTED, "the l0 local proof is not built for row-sharded datasets");
    default: return SLM_OK;
  }
}

int solve_l0_local_group_nodes_impl(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas, double big_M, int32_t n_nodes,
                                    const int32_t* cell, const unsigned long long* in_mask, const unsigned long long* out_mask,
                                    const double* parent_lower, const double* starts, const int32_t* need_ptr, const int32_t* need_idx,
                                    int32_t max_sweeps, double gap_tol, double* lower_out, double* primal_out, double* upper_out, double* u_out,
                                    int32_t* stat_out, slm_point_info* info) {
  if (!ds || !lower_out) return fail(SLM_ERR_BAD_ARG, "NULL argument");
  const int* gid = ds->singleton || ds->h_gid.empty() ? nullptr : ds->h_gid.data();
  int ng = 0;
  const L0GpRefusal Q = l0_group_nodes_check(n_cells, alphas, etas, big_M, n_nodes, cell, in_mask, out_mask, parent_lower, starts, ds->p, gap_tol,
                                             gid, need_ptr, need_idx, row_sharded(ds), &ng);
  if (Q.kind == L0_GP_FIRST) {
    const long long which = Q.which;
    switch (Q.nd) {
      case L0_ND_NULL: return fail(SLM_ERR_BAD_ARG, "NULL argument");
      case L0_ND_CELLS: return fail(SLM_ERR_BAD_ARG, "n_cells must be >= 1 (got %d)", n_cells);
      case L0_ND_PROBLEMS: return fail(SLM_ERR_BAD_ARG, "n_cells must be at most %d cells (got %d)", L0_LS_MAX_PROBLEMS, n_cells);
      case L0_ND_NODES: return fail(SLM_ERR_BAD_ARG, "n_nodes must be >= 1 (got %d)", n_nodes);
      case L0_ND_BATCH: return fail(SLM_ERR_BAD_ARG, "n_nodes must be at most %d nodes (got %d)", L0_ND_MAX_BATCH, n_nodes);
      case L0_ND_BIG_M: return fail(SLM_ERR_BAD_ARG, "big_M must be >= 0");
      case L0_ND_ALPHA: return fail(SLM_ERR_BAD_ARG, "alphas[%lld] must be finite and >= 0", which);
      case L0_ND_ETA: return fail(SLM_ERR_BAD_ARG, "etas[%lld] must be finite and >= 0", which);
      case L0_ND_GAP_TOL: return fail(SLM_ERR_BAD_ARG, "gap_tol must be >= 0");
      case L0_ND_WIDTH: return fail(SLM_ERR_UNSUPPORTED, "the l0 local proof takes up to %d columns (got %lld)", L0_LS_PMAX, (long long)ds->p);
      case L0_ND_CELL: return fail(SLM_ERR_BAD_ARG, "cell[%lld] is not a cell of the call", which);
      case L0_ND_MASK: return fail(SLM_ERR_BAD_ARG, "node %lld holds a group that is both IN and OUT", which);
      case L0_ND_PARENT: return fail(SLM_ERR_BAD_ARG, "parent_lower[%lld] is neither a number nor -infinity", which);
      case L0_ND_START: return fail(SLM_ERR_BAD_ARG, "starts[%lld] is not a finite number", which);
      default: return fail(SLM_ERR_BAD_ARG, "NULL argument");
    }
  }
  if (Q.kind != L0_GP_OK) return l0_gp_refuse(Q, ng);
  L0GroupMapOwner own;
  own.build(ds, ng, need_ptr, need_idx);
  return solve_l0_local_nodes_impl(ds, n_cells, alphas, etas, big_M, n_nodes, cell, in_mask, out_mask, parent_lower, starts, max_sweeps, gap_tol,
                                   lower_out, primal_out, upper_out, u_out, stat_out, info, &own.map);
}

int solve_l0_local_group_prove_impl(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas, double big_M,
                                    const double* incumbents, const int32_t* need_ptr, const int32_t* need_idx, double rel_gap, int32_t max_nodes,
                                    int32_t width, int32_t max_sweeps, int64_t leaf_capacity, double* beta_out, double* objective_out,
                                    double* lower_out, int32_t* nodes_out, int32_t* rounds_out, int32_t* status_out, int32_t* group_support_out,
                                    int32_t* leaf_cell, unsigned long long* leaf_in, unsigned long long* leaf_out, double* leaf_u,
                                    double* leaf_lower, int64_t* leaf_count, slm_point_info* info) {
  if (!ds || !beta_out || !objective_out || !lower_out) return fail(SLM_ERR_BAD_ARG, "NULL argument");
  const int* gid = ds->singleton || ds->h_gid.empty() ? nullptr : ds->h_gid.data();
  int ng = 0;
  const L0GpRefusal Q = l0_group_prove_check(n_cells, alphas, etas, big_M, incumbents, ds->p, rel_gap, max_nodes, width, gid, need_ptr, need_idx,
                                             row_sharded(ds), &ng);
  if (Q.kind == L0_GP_FIRST) {
    const long long which = Q.which;
    switch (Q.pv) {
      case L0_PV_NULL: return fail(SLM_ERR_BAD_ARG, "NULL argument");
      case L0_PV_CELLS: return fail(SLM_ERR_BAD_ARG, "n_cells must be >= 1 (got %d)", n_cells);
      case L0_PV_PROBLEMS: return fail(SLM_ERR_BAD_ARG, "n_cells must be at most %d cells (got %d)", L0_LS_MAX_PROBLEMS, n_cells);
      case L0_PV_BIG_M: return fail(SLM_ERR_BAD_ARG, "big_M must be >= 0");
      case L0_PV_ALPHA: return fail(SLM_ERR_BAD_ARG, "alphas[%lld] must be finite and >= 0", which);
      case L0_PV_ETA: return fail(SLM_ERR_BAD_ARG, "etas[%lld] must be finite and >= 0", which);
      case L0_PV_REL_GAP: return fail(SLM_ERR_BAD_ARG, "rel_gap must lie in [1e-10, 1]");
      case L0_PV_MAX_NODES: return fail(SLM_ERR_BAD_ARG, "max_nodes must be >= 1 (got %d)", max_nodes);
      case L0_PV_TREE_WIDTH: return fail(SLM_ERR_BAD_ARG, "width must be >= 1 (got %d)", width);
      case L0_PV_WIDTH: return fail(SLM_ERR_UNSUPPORTED, "the l0 local proof takes up to %d columns (got %lld)", L0_LS_PMAX, (long long)ds->p);
      case L0_PV_INCUMBENT: return fail(SLM_ERR_BAD_ARG, "incumbents[%lld] is outside the box [-big_M, big_M] or not a number", which);
      default: return fail(SLM_ERR_BAD_ARG, "NULL argument");
    }
  }
  if (Q.kind != L0_GP_OK) return l0_gp_refuse(Q, ng);
  L0GroupMapOwner own;
  own.build(ds, ng, need_ptr, need_idx);
  const int rc = solve_l0_local_prove_impl(ds, n_cells, alphas, etas, big_M, incumbents, rel_gap, max_nodes, width, max_sweeps, leaf_capacity,
                                           beta_out, objective_out, lower_out, nodes_out, rounds_out, status_out, leaf_cell, leaf_in, leaf_out,
                                           leaf_u, leaf_lower, leaf_count, info, &own.map);
  if (group_support_out && (rc == SLM_OK || rc == SLM_ERR_NOT_CONVERGED))  // cl(S) of every cell's incumbent
    for (int e = 0; e < n_cells; ++e) l0_gp_closure(beta_out + (size_t)e * ds->p, own.map, group_support_out + (size_t)e * ng);
  return rc;
}

}  // namespace

// One batch of GROUP node relaxations of the local proof, from one launch of l0_local_group_node_kernel: one wavefront per node.
extern "C" int slm_solve_l0_local_group_nodes(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas, double big_M,
                                              int32_t n_nodes, const int32_t* cell, const uint64_t* in_mask, const uint64_t* out_mask,
                                              const double* parent_lower, const double* starts, const int32_t* need_ptr, const int32_t* need_idx,
                                              int32_t max_sweeps, double gap_tol, double* lower_out, double* primal_out, double* upper_out,
                                              double* u_out, int32_t* stat_out, slm_point_info* info) {
  return solve_l0_local_group_nodes_impl(ds, n_cells, alphas, etas, big_M, n_nodes, cell, reinterpret_cast<const unsigned long long*>(in_mask),
                                         reinterpret_cast<const unsigned long long*>(out_mask), parent_lower, starts, need_ptr, need_idx,
                                         max_sweeps, gap_tol, lower_out, primal_out, upper_out, u_out, stat_out, info);
}

// The local proof with groups and a hierarchy: branch and bound over GROUP nodes for every cell of a grid, one launch a round.
extern "C" int slm_solve_l0_local_group_prove(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas, double big_M,
                                              const double* incumbents, const int32_t* need_ptr, const int32_t* need_idx, double rel_gap,
                                              int32_t max_nodes, int32_t width, int32_t max_sweeps, int64_t leaf_capacity, double* beta_out,
                                              double* objective_out, double* lower_out, int32_t* nodes_out, int32_t* rounds_out,
                                              int32_t* status_out, int32_t* group_support_out, int32_t* leaf_cell, uint64_t* leaf_in,
                                              uint64_t* leaf_out, double* leaf_u, double* leaf_lower, int64_t* leaf_count, slm_point_info* info) {
  return solve_l0_local_group_prove_impl(ds, n_cells, alphas, etas, big_M, incumbents, need_ptr, need_idx, rel_gap, max_nodes, width, max_sweeps,
                                         leaf_capacity, beta_out, objective_out, lower_out, nodes_out, rounds_out, status_out, group_support_out,
                                         leaf_cell, reinterpret_cast<unsigned long long*>(leaf_in), reinterpret_cast<unsigned long long*>(leaf_out),
                                         leaf_u, leaf_lower, leaf_count, info);
}

// The l0 local search on up to 16 row sets of one dataset: every (row set, cell, start) problem from one launch.
extern "C" int slm_solve_l0_local_folds(slm_dataset* ds, int32_t count, const double* const* row_weights, const int64_t* n_effs,
                                        int32_t intercept, int32_t n_cells, const double* alphas, const double* etas, double big_M,
                                        int32_t n_starts, const double* starts, int32_t swaps, double* beta_out, double* intercept_out,
                                        double* objective_out, int32_t* start_out, int32_t* stat_out, slm_point_info* info) {
  return solve_l0_local_folds_impl(L0_LOCAL_SETS, ds, count, row_weights, n_effs, intercept, n_cells, alphas, nullptr, etas, big_M, n_starts,
                                   starts, swaps, beta_out, intercept_out, objective_out, start_out, stat_out, info);
}

// The cardinality form of the l0 local search: every (row set, (size, eta) cell, start) problem from one launch of
// l0_local_kernel<true>: at most sizes[e] non-zeros, nothing proven.
extern "C" int slm_solve_l0_local_subsets(slm_dataset* ds, int32_t count, const double* const* row_weights, const int64_t* n_effs,
                                          int32_t intercept, int32_t n_cells, const int32_t* sizes, const double* etas, double big_M,
                                          int32_t n_starts, const double* starts, int32_t swaps, double* beta_out, double* intercept_out,
                                          double* objective_out, int32_t* start_out, int32_t* stat_out, slm_point_info* info) {
  return solve_l0_local_folds_impl(L0_LOCAL_SIZES, ds, count, row_weights, n_effs, intercept, n_cells, nullptr, sizes, etas, big_M, n_starts,
                                   starts, swaps, beta_out, intercept_out, objective_out, start_out, stat_out, info);
}

// The l0 local search with groups and a hierarchy: every (row set, cell, start) problem from one launch of l0_local_group_kernel.
// The groups are the dataset's (slm_dataset_set_groups), contiguous and ascending; the need lists are closed on the host
// (l0_lg_close); the winner is polished on every column of the groups in cl(S); objective_out = quad + alpha |cl(S)|.
extern "C" int slm_solve_l0_local_groups(slm_dataset* ds, int32_t count, const double* const* row_weights, const int64_t* n_effs,
                                         int32_t intercept, int32_t n_cells, const double* alphas, const double* etas, double big_M,
                                         const int32_t* need_ptr, const int32_t* need_idx, int32_t n_starts, const double* starts,
                                         int32_t swaps, double* beta_out, double* intercept_out, double* objective_out,
                                         int32_t* start_out, int32_t* group_support_out, int32_t* stat_out, slm_point_info* info) {
  const L0LocalGroups lg{need_ptr, need_idx, group_support_out};
  return solve_l0_local_folds_impl(L0_LOCAL_GROUPS, ds, count, row_weights, n_effs, intercept, n_cells, alphas, nullptr, etas, big_M, n_starts,
                                   starts, swaps, beta_out, intercept_out, objective_out, start_out, stat_out, info, &lg);
}

// The l0 local search with an l1 term: every (row set, (alpha, l1, ridge) cell, start) problem from one launch of
// l0_local_l1_kernel; the winner is polished by the soft-threshold descent and the sign-face solve on its support (l0_l1l_polish).
extern "C" int slm_solve_l0_local_l1(slm_dataset* ds, int32_t count, const double* const* row_weights, const int64_t* n_effs,
                                     int32_t intercept, int32_t n_cells, const double* alphas, const double* l1s, const double* ridges,
                                     double big_M, int32_t n_starts, const double* starts, int32_t swaps, double* beta_out,
                                     double* intercept_out, double* objective_out, int32_t* start_out, int32_t* stat_out,
                                     slm_point_info* info) {
  return solve_l0_local_folds_impl(L0_LOCAL_L1, ds, count, row_weights, n_effs, intercept, n_cells, alphas, nullptr, ridges, big_M, n_starts,
                                   starts, swaps, beta_out, intercept_out, objective_out, start_out, stat_out, info, nullptr, l1s);
}

// The local bound: for every cell a proven lower bound on the objective of slm_solve_l0_local, from one launch of
// l0_local_bound_kernel -- a bound whatever the status, tight with a ridge or a real box, weak at eta = 0 under a loose big_M.
extern "C" int slm_solve_l0_local_bound(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas, double big_M,
                                        const double* starts, int32_t max_sweeps, double gap_tol, double* lower_out, double* primal_out,
                                        double* u_out, int32_t* stat_out, slm_point_info* info) {
  return solve_l0_local_bound_impl(ds, n_cells, alphas, etas, big_M, starts, max_sweeps, gap_tol, lower_out, primal_out, u_out, stat_out, info);
}

// One batch of node relaxations of the local proof, from one launch of l0_local_node_kernel: one wavefront per node.
extern "C" int slm_solve_l0_local_nodes(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas, double big_M, int32_t n_nodes,
                                        const int32_t* cell, const uint64_t* in_mask, const uint64_t* out_mask, const double* parent_lower,
                                        const double* starts, int32_t max_sweeps, double gap_tol, double* lower_out, double* primal_out,
                                        double* upper_out, double* u_out, int32_t* stat_out, slm_point_info* info) {
  return solve_l0_local_nodes_impl(ds, n_cells, alphas, etas, big_M, n_nodes, cell, reinterpret_cast<const unsigned long long*>(in_mask),
                                   reinterpret_cast<const unsigned long long*>(out_mask), parent_lower, starts, max_sweeps, gap_tol, lower_out,
                                   primal_out, upper_out, u_out, stat_out, info);
}

// The local proof: branch and bound on the local bound for every cell of a grid, one launch a round; `optimal` is proven.
extern "C" int slm_solve_l0_local_prove(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas, double big_M,
                                        const double* incumbents, double rel_gap, int32_t max_nodes, int32_t width, int32_t max_sweeps,
                                        int64_t leaf_capacity, double* beta_out, double* objective_out, double* lower_out, int32_t* nodes_out,
                                        int32_t* rounds_out, int32_t* status_out, int32_t* leaf_cell, uint64_t* leaf_in, uint64_t* leaf_out,
                                        double* leaf_u, double* leaf_lower, int64_t* leaf_count, slm_point_info* info) {
  return solve_l0_local_prove_impl(ds, n_cells, alphas, etas, big_M, incumbents, rel_gap, max_nodes, width, max_sweeps, leaf_capacity, beta_out,
                                   objective_out, lower_out, nodes_out, rounds_out, status_out, leaf_cell,
                                   reinterpret_cast<unsigned long long*>(leaf_in), reinterpret_cast<unsigned long long*>(leaf_out), leaf_u,
                                   leaf_lower, leaf_count, info);
}

// The l0 local search: every (cell, start) problem from one launch of l0_local_kernel, up to 1024 columns, nothing proven.
extern "C" int slm_solve_l0_local(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas, double big_M,
                                  int32_t n_starts, const double* starts, double* beta_out, double* objective_out, int32_t* start_out,
                                  slm_point_info* info) {
  return solve_l0_local_impl(1, ds, n_cells, alphas, etas, big_M, n_starts, starts, beta_out, objective_out, start_out, info);
}

// The same call without the swap scan: every problem ends at its descent's fixed point.
extern "C" int slm_solve_l0_local_descent(slm_dataset* ds, int32_t n_cells, const double* alphas, const double* etas, double big_M,
                                          int32_t n_starts, const double* starts, double* beta_out, double* objective_out,
                                          int32_t* start_out, slm_point_info* info) {
  return solve_l0_local_impl(0, ds, n_cells, alphas, etas, big_M, n_starts, starts, beta_out, objective_out, start_out, info);
}

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
  return solve_l0_profile_impl<false>(ds, alpha_min, max_groups, eta, T, 0.0, big_M, need, max_nodes, beta_out, support_out, value_out, nodes_out, info);
}

// The profile on the kernel's wide instantiation: masks of two words in need and support_out, max_groups up to 64.
extern "C" int slm_solve_l0_profile_wide(slm_dataset* ds, double alpha_min, int32_t max_groups, double eta, const double* T, double big_M,
                                         const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out,
                                         double* value_out, int64_t* nodes_out, slm_point_info* info) {
  return solve_l0_profile_impl<true>(ds, alpha_min, max_groups, eta, T, 0.0, big_M, need, max_nodes, beta_out, support_out, value_out, nodes_out, info);
}

// The l1 profile (the reference's L1L0 at every alpha from one search): the table F_k = min over supports of exactly k groups of the
// lasso value of the support; no ridge term, no T.  eta_l1 == 0 is slm_solve_l0_profile with eta = 0.
extern "C" int slm_solve_l0_l1_profile(slm_dataset* ds, double alpha_min, int32_t max_groups, double eta_l1, double big_M,
                                       const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out, double* value_out,
                                       int64_t* nodes_out, slm_point_info* info) {
  return solve_l0_profile_impl<false>(ds, alpha_min, max_groups, 0.0, nullptr, eta_l1, big_M, need, max_nodes, beta_out, support_out, value_out,
                                      nodes_out, info);
}

// The l1 profile on the kernel's wide instantiation: masks of two words, max_groups up to 64, every support within 64 columns.
extern "C" int slm_solve_l0_l1_profile_wide(slm_dataset* ds, double alpha_min, int32_t max_groups, double eta_l1, double big_M,
                                            const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out,
                                            double* value_out, int64_t* nodes_out, slm_point_info* info) {
  return solve_l0_profile_impl<true>(ds, alpha_min, max_groups, 0.0, nullptr, eta_l1, big_M, need, max_nodes, beta_out, support_out, value_out,
                                     nodes_out, info);
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

// The profiles of `count` row sets of one dataset (CV folds and all rows) from one launch of the kernel's batched instantiation.
extern "C" int slm_solve_l0_profile_batch(slm_dataset* ds, int32_t count, const double* const* row_weights, const int64_t* n_effs,
                                          int32_t intercept, double alpha_min, int32_t max_groups, double eta, const double* T, double big_M,
                                          const uint64_t* need, int64_t max_nodes, double* beta_out, double* intercept_out,
                                          uint64_t* support_out, double* value_out, int64_t* nodes_out, slm_point_info* info) {
  return solve_l0_profile_grid_impl(false, ds, count, row_weights, n_effs, intercept, 1, &eta, 0, alpha_min, max_groups, T, big_M, need, max_nodes,
                                    beta_out, intercept_out, support_out, value_out, nodes_out, info);
}

// The profiles of `count` row sets at n_eta weights each -- ridge (eta_kind 0) or l1 (eta_kind 1) -- from one launch: problem
// r * n_eta + e is row set r with etas[e].
extern "C" int slm_solve_l0_profile_grid(slm_dataset* ds, int32_t count, const double* const* row_weights, const int64_t* n_effs,
                                         int32_t intercept, int32_t n_eta, const double* etas, int32_t eta_kind, double alpha_min,
                                         int32_t max_groups, const double* T, double big_M, const uint64_t* need, int64_t max_nodes,
                                         double* beta_out, double* intercept_out, uint64_t* support_out, double* value_out,
                                         int64_t* nodes_out, slm_point_info* info) {
  return solve_l0_profile_grid_impl(true, ds, count, row_weights, n_effs, intercept, n_eta, etas, eta_kind, alpha_min, max_groups, T, big_M, need,
                                    max_nodes, beta_out, intercept_out, support_out, value_out, nodes_out, info);
}
