// Host side of the MI355X fit engine, sixth unit: the exact l0 estimators (csrc/l0_kernels.hpp) -- the reference's
// mixed-integer family (reference src/sparselm/model/_miqp/_best_subset.py, _regularized_l0.py), which it hands to
// Gurobi or SCIP through cvxpy.  Here: the dataset's own Gram (engine_cov.hip), the search order, the greedy seed and the
// unconstrained bound on the host (p <= 64: microseconds), ONE launch of the search, and the winner's coefficients
// recomputed in one place from the Gram on its support.
// slm_solve_l0_l1 (the reference's L1L0, _regularized_l0.py:258-410) is the same call in l1 mode: the kernel's L1 instantiation,
// the l0_l1_* functions of l0_host.hpp for seed, winner and the dual bound on all columns.
#include "engine_internal.hpp"
#include "l0_host.hpp"
#include "l0_kernels.hpp"

namespace {

constexpr long long kL0DefaultNodes = 1ll << 30;  // the budget of a call that names none: at the 6.2e8 nodes/s measured at 25 x 30
                                                  // (profiles/l0_search.txt) a call that exhausts it stays under two seconds

// Both entries.  eta_l1 > 0 is l1 mode (the kernel's L1 instantiation, the l0_l1_* functions of l0_host.hpp); eta_l1 == 0 is the
// search without an l1 term, instruction for instruction what it was before there was one.
int solve_l0_impl(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T, double eta_l1, double big_M,
                  const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out, double* lower_bound_out,
                  int64_t* nodes_out, slm_point_info* info) {
  if (!ds || !beta_out) return fail(SLM_ERR_BAD_ARG, "NULL argument");
  // the arguments are checked before anything touches the device
  if (!(alpha >= 0.0) || !std::isfinite(alpha)) return fail(SLM_ERR_BAD_ARG, "alpha must be finite and >= 0");
  if (!(eta >= 0.0) || !std::isfinite(eta)) return fail(SLM_ERR_BAD_ARG, "eta must be finite and >= 0");
  if (!(eta_l1 >= 0.0) || !std::isfinite(eta_l1)) return fail(SLM_ERR_BAD_ARG, "eta_l1 must be finite and >= 0");
  const bool l1 = eta_l1 > 0.0;
  if (!(big_M >= 0.0)) return fail(SLM_ERR_BAD_ARG, "big_M must be >= 0");
  const int64_t p64 = ds->p;
  const int ng = ds->singleton ? (int)std::min<int64_t>(p64, L0_PMAX + 1) : ds->G;
  if (need && ng <= L0_PMAX)
    for (int g = 0; g < ng; ++g)
      if (ng < 64 && (need[g] >> ng) != 0) return fail(SLM_ERR_BAD_ARG, "need[%d] names a group at or beyond n_groups = %d", g, ng);
  if (T)
    for (int64_t e = 0; e < p64 * p64 && p64 <= L0_PMAX; ++e)
      if (!std::isfinite(T[e])) return fail(SLM_ERR_BAD_ARG, "T contains a non-finite value");
  if (p64 > L0_PMAX || ng > L0_PMAX)
    return fail(SLM_ERR_UNSUPPORTED, "the exact l0 search takes up to %d columns and %d groups (got %lld, %d)", L0_PMAX, L0_PMAX,
                (long long)p64, ng);
  if (row_sharded(ds)) return fail(SLM_ERR_UNSUPPORTED, "the exact l0 search is not built for row-sharded datasets");
  const int p = (int)p64;
  const int K = max_groups < 0 ? 0 : std::min<int>(max_groups, ng);
  // the value (without alpha |S|) and coefficients of one support, as the kernel values a node
  auto value_of = [&](const std::vector<double>& H, const std::vector<double>& c, const std::vector<int>& gstart, unsigned long long mask,
                      bool polish, double* beta) {
    return l1 ? l0_l1_support(H.data(), c.data(), p, gstart, mask, eta_l1, big_M, polish, beta)
              : l0_support(H.data(), c.data(), p, gstart, mask, big_M, polish, beta);
  };
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
  std::vector<double> G((size_t)p * p), cvec((size_t)p);
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
  std::vector<int> gorder((size_t)ng), gpos((size_t)ng);
  std::iota(gorder.begin(), gorder.end(), 0);
  auto score = [&](int g) { return den[(size_t)g] > 0.0 ? num[(size_t)g] / den[(size_t)g] : 0.0; };
  std::stable_sort(gorder.begin(), gorder.end(), [&](int x, int y) { return score(x) > score(y); });
  for (int k = 0; k < ng; ++k) gpos[(size_t)gorder[(size_t)k]] = k;
  std::vector<int> cols;  // search position -> column of X
  std::vector<int> gstart((size_t)ng + 1, 0);
  for (int k = 0; k < ng; ++k) {
    for (int j = 0; j < p; ++j)
      if (gid[(size_t)j] == gorder[(size_t)k]) cols.push_back(j);
    gstart[(size_t)k + 1] = (int)cols.size();
  }
  std::vector<double> H((size_t)p * p), c((size_t)p);
  for (int i = 0; i < p; ++i) {
    c[(size_t)i] = cvec[(size_t)cols[(size_t)i]];
    for (int j = 0; j < p; ++j) {
      const int ci = cols[(size_t)i], cj = cols[(size_t)j];
      // (T symmetrised: only its symmetric part acts in beta^T T beta)
      const double t = T ? 0.5 * (T[(size_t)ci * p + cj] + T[(size_t)cj * p + ci]) : (ci == cj ? 1.0 : 0.0);
      H[(size_t)i * p + j] = G[(size_t)ci * p + cj] + 2.0 * eta * t;
    }
  }
  std::vector<unsigned long long> needo((size_t)ng, 0ull);
  if (need)
    for (int g = 0; g < ng; ++g)
      for (int h = 0; h < ng; ++h)
        if (h != g && ((need[g] >> h) & 1)) needo[(size_t)gpos[(size_t)g]] |= 1ull << gpos[(size_t)h];

  // ---- the unconstrained value on all columns, and the greedy seed of the incumbent -----------------------------------------
  std::vector<double> beta_s((size_t)p);
  double q_all;
  {
    L0Factor f(H.data(), c.data(), p);
    for (int j = 0; j < p; ++j) (void)f.push(j);
    q_all = -0.5 * f.ss;
  }
  // the subtree bound's lower bound on the value of all columns: in l1 mode the lasso dual value where it is above q_all
  const double bound = l1 ? l0_l1_lower_bound(H.data(), c.data(), p, ds->cov[(size_t)entry].yy, eta_l1, q_all) : q_all;
  const unsigned long long all_mask = ng == 64 ? ~0ull : ((1ull << ng) - 1);
  double seed_val = 0.0;  // the empty support
  unsigned long long seed_mask = 0;
  {
    L0Factor f(H.data(), c.data(), p);
    unsigned long long cur = 0;
    for (int step = 0; step < K; ++step) {
      int pick = -1;
      double pick_ss = f.ss;
      const int m0 = f.m;
      for (int g = 0; g < ng; ++g) {
        if (((cur >> g) & 1) || (needo[(size_t)g] & ~cur)) continue;
        for (int j = gstart[(size_t)g]; j < gstart[(size_t)g + 1]; ++j) (void)f.push(j);  // (dependent columns are skipped, as in the kernel)
        if (f.ss > pick_ss) {
          pick_ss = f.ss;
          pick = g;
        }
        f.pop_to(m0);
      }
      if (pick < 0) break;
      cur |= 1ull << pick;
      // (the factor keeps search order inside the kernel; the seed's value is taken the same way)
      const double v = value_of(H, c, gstart, cur, false, beta_s.data()) + alpha * (double)(step + 1);
      if (v < seed_val) {
        seed_val = v;
        seed_mask = cur;
      }
      for (int j = gstart[(size_t)pick]; j < gstart[(size_t)pick + 1]; ++j) (void)f.push(j);
    }
    if (K >= ng && ng > 0) {  // every group: the one support whose value can meet the bound exactly
      const double v = value_of(H, c, gstart, all_mask, false, beta_s.data()) + alpha * (double)ng;
      if (v < seed_val) {
        seed_val = v;
        seed_mask = all_mask;
      }
    }
  }

  // ---- the search: one launch --------------------------------------------------------------------------------------------
  const int d = std::min(ng, L0_PREFIX);
  const long long n_tickets = 1ll << d;
  const int blocks = (int)std::max<long long>(1, std::min<long long>(2ll * eng->cus, (n_tickets + L0_WAVES - 1) / L0_WAVES));
  const int waves = blocks * L0_WAVES;
  // one block of 8-byte words: control | best values | best supports | H | c | need | group starts
  const size_t off_bv = L0_CTL_WORDS, off_bm = off_bv + (size_t)waves, off_H = off_bm + (size_t)waves, off_c = off_H + (size_t)p * p,
               off_need = off_c + (size_t)p, off_gs = off_need + (size_t)ng, words = off_gs + (size_t)ng + 1;
  std::vector<unsigned long long> h(words, 0ull);
  h[L0_INCUMBENT] = l0_key(seed_val);
  memcpy(&h[off_H], H.data(), sizeof(double) * (size_t)p * p);
  memcpy(&h[off_c], c.data(), sizeof(double) * (size_t)p);
  for (int g = 0; g < ng; ++g) h[off_need + (size_t)g] = needo[(size_t)g];
  for (int g = 0; g <= ng; ++g) h[off_gs + (size_t)g] = (unsigned long long)gstart[(size_t)g];
  unsigned long long* dev = nullptr;
  SLM_TRY(dalloc(&dev, words));
  struct Guard {
    unsigned long long*& p;
    hipStream_t s;
    ~Guard() {
      (void)hipStreamSynchronize(s);
      dfree(p);
    }
  } guard{dev, s};
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
  if (l1)
    hipLaunchKernelGGL(l0_search_kernel<true>, dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, k);
  else
    hipLaunchKernelGGL(l0_search_kernel<false>, dim3((unsigned)blocks), dim3(64 * L0_WAVES), 0, s, k);
  SLM_TRY(check_launch());
  HIP_TRY(hipMemcpyAsync(h.data(), dev, sizeof(unsigned long long) * off_H, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));

  // ---- the winner: the waves' bests and the seed in a fixed order, the lower support on a bitwise tie -------------------------
  double win_val = seed_val;
  unsigned long long win_mask = seed_mask;
  for (int wv = 0; wv < waves; ++wv) {
    double v;
    memcpy(&v, &h[off_bv + (size_t)wv], 8);
    const unsigned long long mk = h[off_bm + (size_t)wv];
    if (v < win_val || (v == win_val && mk < win_mask)) {
      win_val = v;
      win_mask = mk;
    }
  }
  const bool finished = h[L0_ABORTED] == 0;
  // its coefficients, recomputed here whichever wave found it
  const double quad = value_of(H, c, gstart, win_mask, true, beta_s.data());
  int n_active = 0;
  unsigned long long support = 0;
  for (int g = 0; g < ng; ++g)
    if ((win_mask >> g) & 1) {
      ++n_active;
      support |= 1ull << gorder[(size_t)g];
    }
  const double objective = quad + alpha * (double)n_active;
  for (int i = 0; i < p; ++i) beta_out[cols[(size_t)i]] = beta_s[(size_t)i];
  if (support_out) *support_out = support;
  if (lower_bound_out) *lower_bound_out = finished ? objective : std::min(objective, bound);
  if (nodes_out) *nodes_out = (int64_t)h[L0_NODES];
  if (info) {
    // 1/(2n)||X beta - y||_W^2 = 1/2 beta^T G beta - c^T beta + 1/2 y^T W y / n from the Gram already on the host: no second launch
    double loss = 0.5 * ds->cov[(size_t)entry].yy;
    for (int i = 0; i < p; ++i) {
      if (beta_out[i] == 0.0) continue;
      double t = 0.0;
      for (int j = 0; j < p; ++j) t += G[(size_t)i * p + j] * beta_out[j];
      loss += beta_out[i] * (0.5 * t - cvec[(size_t)i]);
    }
    memset(info, 0, sizeof(*info));
    info->n_iter = 1;
    info->status = finished ? SLM_OK : SLM_ERR_NOT_CONVERGED;
    info->loss = loss;
    info->mode = 4;
    info->kkt = objective;
    info->mu = seed_val;
    info->L = bound;
    info->rejects = (int32_t)std::min<unsigned long long>(h[L0_DESCENTS], 0x7fffffffull);  // (l1 mode: descents run)
    double bn = 0.0;
    for (int j = 0; j < p; ++j) bn += beta_out[j] * beta_out[j];
    info->beta_norm = std::sqrt(bn);
  }
  if (!finished) return fail(SLM_ERR_NOT_CONVERGED, "the node budget (%lld) ran out before the search finished: the incumbent is returned",
                             (long long)k.max_nodes);
  return SLM_OK;
}

}  // namespace

extern "C" int slm_solve_l0(slm_dataset* ds, double alpha, int32_t max_groups, double eta, const double* T, double big_M,
                            const uint64_t* need, int64_t max_nodes, double* beta_out, uint64_t* support_out,
                            double* lower_bound_out, int64_t* nodes_out, slm_point_info* info) {
  return solve_l0_impl(ds, alpha, max_groups, eta, T, 0.0, big_M, need, max_nodes, beta_out, support_out, lower_bound_out, nodes_out, info);
}

// The reference's L1L0 (_regularized_l0.py:258-410): no cardinality bound, no ridge term, eta_l1 ||beta||_1.
extern "C" int slm_solve_l0_l1(slm_dataset* ds, double alpha, double eta_l1, double big_M, const uint64_t* need, int64_t max_nodes,
                               double* beta_out, uint64_t* support_out, double* lower_bound_out, int64_t* nodes_out,
                               slm_point_info* info) {
  return solve_l0_impl(ds, alpha, L0_PMAX, 0.0, nullptr, eta_l1, big_M, need, max_nodes, beta_out, support_out, lower_bound_out, nodes_out,
                       info);
}
