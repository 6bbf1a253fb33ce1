// Host side of the exact l0 search (l0_kernels.hpp, engine_l0.hip): the limits and tolerances the kernel and the host share,
// the factor of H on a growing list of columns as the kernel keeps it, the boxed descent candidates are compared by, and the
// value and coefficients of one support, the same for l1 mode (a lasso per support: the descent, its polish, the dual
// bound on all columns), and for profile mode the pruning rule and the two questions its table answers.  Like host_logic.hpp and tail_logic.hpp it is free of HIP types so that g++
// compiles it alone: tests/host_logic_test.cpp, tests/l1l0_host_test.cpp, tests/l0_profile_host_test.cpp and tests/l1l0_profile_host_test.cpp run these functions on the CPU under the sanitizers, and slm_solve_l0 / slm_solve_l0_l1 / slm_solve_l0_profile call
// THESE functions for the seed, the bound q_all and the winner's coefficients -- what is tested is what runs.  The l1 profile
// (slm_solve_l0_l1_profile, slm_solve_l0_l1_profile_wide) values the seed and the winner of every size by l0_l1_support_of, the
// lasso of a support for a mask of either width, and cuts with l0_l1_lower_bound on up to 128 columns.  The wide mode
// (slm_solve_l0_wide, slm_solve_l0_profile_wide; tests/l0_wide_host_test.cpp) adds masks of two words, a factor with a capacity
// parameter and the capacity rule.  The constrained mode (slm_solve_l0_constrained; tests/l0_con_host_test.cpp) adds the splitting
// that values a support under linear constraints, the dual value host and device share, its face polish, the positive-definite
// check and the lower bound on all columns.  The exclusion bound (slm_solve_l0_xb, slm_solve_l0_xb_wide;
// tests/l0_bound_host_test.cpp) adds P = H^-1, P c, the margin delta and the guarded bound host and device share.  The end of
// the file holds what every entry's launch shares (tests/l0_launch_host_test.cpp): the layout of the device block, the
// winner among the waves' results, the way back to the caller's groups and columns, and the loss from the Gram.  The batched
// profile (slm_solve_l0_profile_batch; tests/l0_batch_host_test.cpp) adds the layout of several problems in one block and the
// elimination of an intercept column from a Gram.  The profile grid (slm_solve_l0_profile_grid; tests/l0_grid_host_test.cpp) adds
// the problem index over (row set, eta), its argument checks and the layout at up to L0_GRID_MAX problems.  The local search
// (slm_solve_l0_local; tests/l0_local_host_test.cpp) adds, at the very end, the two decisions host and device share, the rule
// itself without a device (l0_local_solve: ONE twin of the one kernel, all of its rules), the polish of its winner and its
// argument checks; it uses nothing of the exact search but l0_boxed and the dense Cholesky.
#pragma once
#include <stddef.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <memory>
#include <type_traits>
#include <vector>

namespace slm {

constexpr int L0_PMAX = 64;        // columns, and groups; in wide mode the rows of the factor (independent columns of a support)
constexpr int L0_WIDE_PMAX = 128;  // columns, and groups, of the wide mode (slm_solve_l0_wide, slm_solve_l0_profile_wide)
constexpr int L0_CD_SWEEPS = 10000;
constexpr double L0_CD_TOL = 1e-12;
constexpr double L0_PIVOT = 1e-12;

// ---- supports as masks over the groups ----------------------------------------------------------------------------------------
//
// One 64-bit word up to 64 groups; the wide mode's two words, bit g of the 128-bit integer hi:lo.  One set of functions for
// both (and for host and device: constexpr), so that the search, the seed and the winner are written once.  The order of
// l0m_less is that of the 128-bit integer -- the high word first, then the low one: "the lower support wins a bitwise tie".
struct L0Mask128 {
  unsigned long long lo, hi;
};
constexpr unsigned long long l0m_low_word(int g) { return g <= 0 ? 0ull : (g >= 64 ? ~0ull : (~0ull >> (64 - g))); }
template <class M> constexpr M l0m_none();
template <> constexpr unsigned long long l0m_none<unsigned long long>() { return 0ull; }
template <> constexpr L0Mask128 l0m_none<L0Mask128>() { return L0Mask128{0ull, 0ull}; }
template <class M> constexpr M l0m_ones();
template <> constexpr unsigned long long l0m_ones<unsigned long long>() { return ~0ull; }
template <> constexpr L0Mask128 l0m_ones<L0Mask128>() { return L0Mask128{~0ull, ~0ull}; }
template <class M> constexpr M l0m_below(int g);  // the bits 0 .. g - 1
template <> constexpr unsigned long long l0m_below<unsigned long long>(int g) { return g == 0 ? 0ull : (~0ull >> (64 - g)); }
template <> constexpr L0Mask128 l0m_below<L0Mask128>(int g) { return L0Mask128{l0m_low_word(g), l0m_low_word(g - 64)}; }
constexpr bool l0m_test(unsigned long long a, int g) { return ((a >> g) & 1) != 0; }
constexpr bool l0m_test(L0Mask128 a, int g) { return g < 64 ? ((a.lo >> g) & 1) != 0 : ((a.hi >> (g - 64)) & 1) != 0; }
constexpr void l0m_set(unsigned long long& a, int g) { a |= 1ull << g; }
constexpr void l0m_set(L0Mask128& a, int g) {
  if (g < 64) a.lo |= 1ull << g;
  else a.hi |= 1ull << (g - 64);
}
constexpr void l0m_clear(unsigned long long& a, int g) { a &= ~(1ull << g); }
constexpr void l0m_clear(L0Mask128& a, int g) {
  if (g < 64) a.lo &= ~(1ull << g);
  else a.hi &= ~(1ull << (g - 64));
}
constexpr void l0m_or(unsigned long long& a, unsigned long long b) { a |= b; }
constexpr void l0m_or(L0Mask128& a, L0Mask128 b) {
  a.lo |= b.lo;
  a.hi |= b.hi;
}
constexpr unsigned long long l0m_and(unsigned long long a, unsigned long long b) { return a & b; }
constexpr L0Mask128 l0m_and(L0Mask128 a, L0Mask128 b) { return L0Mask128{a.lo & b.lo, a.hi & b.hi}; }
constexpr bool l0m_any_outside(unsigned long long a, unsigned long long b) { return (a & ~b) != 0; }  // a holds a bit that b lacks
constexpr bool l0m_any_outside(L0Mask128 a, L0Mask128 b) { return ((a.lo & ~b.lo) | (a.hi & ~b.hi)) != 0; }
constexpr bool l0m_less(unsigned long long a, unsigned long long b) { return a < b; }
constexpr bool l0m_less(L0Mask128 a, L0Mask128 b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

// The factor of H on a growing list of columns, as the kernel keeps it: L row by row, w = L^-1 c, value = -1/2 ||w||^2.
// CAP rows.  An INDEPENDENT column that arrives when all CAP rows are taken is refused like a dependent one and sets
// `overflow` (the wide mode's capacity rule; at p <= CAP it cannot happen).
template <int CAP>
struct L0FactorT {
  const double* H;
  const double* c;
  int p;
  double L[CAP][CAP];
  double w[CAP];
  int col[CAP];
  int m = 0;
  double ss = 0.0;
  bool overflow = false;
  L0FactorT(const double* H_, const double* c_, int p_) : H(H_), c(c_), p(p_) {}
  bool push(int j) {  // false: the column depends on the included ones (the kernel's pivot rule)
    double x[CAP];
    double s2 = 0.0, sw = 0.0;
    for (int k = 0; k < m; ++k) {
      double b = H[(size_t)j * p + col[k]];
      for (int i = 0; i < k; ++i) b -= L[k][i] * x[i];
      x[k] = b / L[k][k];
      s2 += x[k] * x[k];
      sw += x[k] * w[k];
    }
    const double hjj = H[(size_t)j * p + j], piv = hjj - s2;
    if (!(piv > L0_PIVOT * hjj)) return false;
    if (m == CAP) {
      overflow = true;
      return false;
    }
    for (int k = 0; k < m; ++k) L[m][k] = x[k];
    L[m][m] = std::sqrt(piv);
    w[m] = (c[j] - sw) / L[m][m];
    col[m] = j;
    ss += w[m] * w[m];
    ++m;
    return true;
  }
  void pop_to(int m0) {
    m = m0;
    overflow = false;
    ss = 0.0;
    for (int k = 0; k < m; ++k) ss += w[k] * w[k];
  }
  void solve(double* beta /* [m] */) const {  // beta = L^-T w
    for (int k = m - 1; k >= 0; --k) {
      double t = w[k];
      for (int r = k + 1; r < m; ++r) t -= L[r][k] * beta[r];
      beta[k] = t / L[k][k];
    }
  }
};
using L0Factor = L0FactorT<L0_PMAX>;

// min 1/2 b^T H_S b - c_S^T b over |b_j| <= big_M on the columns `cols` (independent: they passed the pivot rule).
// Cyclic coordinate descent with clipping, the kernel's own (same stopping rule): what candidates are COMPARED by, on both
// sides.  polish: the free coordinates are then solved exactly with the bound ones fixed, and that point is taken when it
// stays inside the box (it is then the minimiser to rounding) -- the reported coefficients.  Returns the value.
inline double l0_boxed(const double* H, const double* c, int p, const int* cols, int m, double big_M, bool polish, double* b /* in: start, out */) {
  std::vector<double> g((size_t)m);
  for (int r = 0; r < m; ++r) {
    b[r] = std::min(std::max(b[r], -big_M), big_M);
  }
  for (int r = 0; r < m; ++r) {
    double t = -c[cols[r]];
    for (int k = 0; k < m; ++k) t += H[(size_t)cols[r] * p + cols[k]] * b[k];
    g[(size_t)r] = t;
  }
  for (int sweep = 0; sweep < L0_CD_SWEEPS; ++sweep) {
    double maxd = 0.0, maxb = 0.0;
    for (int k = 0; k < m; ++k) {
      const double nb = std::min(std::max(b[k] - g[(size_t)k] / H[(size_t)cols[k] * p + cols[k]], -big_M), big_M);
      const double dk = nb - b[k];
      if (dk != 0.0) {
        for (int r = 0; r < m; ++r) g[(size_t)r] += H[(size_t)cols[r] * p + cols[k]] * dk;
        b[k] = nb;
      }
      maxd = std::max(maxd, std::fabs(dk));
      maxb = std::max(maxb, std::fabs(nb));
    }
    if (maxd <= L0_CD_TOL * maxb || maxd == 0.0) break;
  }
  // polish: the free coordinates exactly, the bound ones where they are
  std::vector<int> fr;
  for (int k = 0; k < m; ++k)
    if (std::fabs(b[k]) < big_M) fr.push_back(k);
  if (polish && !fr.empty() && (int)fr.size() < m) {
    const int f = (int)fr.size();
    std::vector<double> A((size_t)f * f), rhs((size_t)f);
    for (int i = 0; i < f; ++i) {
      double t = c[cols[fr[(size_t)i]]];
      for (int k = 0; k < m; ++k)
        if (std::fabs(b[k]) >= big_M) t -= H[(size_t)cols[fr[(size_t)i]] * p + cols[k]] * b[k];
      rhs[(size_t)i] = t;
      for (int j = 0; j < f; ++j) A[(size_t)i * f + j] = H[(size_t)cols[fr[(size_t)i]] * p + cols[fr[(size_t)j]]];
    }
    bool ok = true;  // Cholesky of the free block, in place
    for (int i = 0; i < f && ok; ++i) {
      for (int j = 0; j <= i; ++j) {
        double t = A[(size_t)i * f + j];
        for (int k = 0; k < j; ++k) t -= A[(size_t)i * f + k] * A[(size_t)j * f + k];
        if (i == j) {
          if (!(t > 0.0)) { ok = false; break; }
          A[(size_t)i * f + i] = std::sqrt(t);
        } else {
          A[(size_t)i * f + j] = t / A[(size_t)j * f + j];
        }
      }
    }
    if (ok) {
      for (int i = 0; i < f; ++i) {
        double t = rhs[(size_t)i];
        for (int k = 0; k < i; ++k) t -= A[(size_t)i * f + k] * rhs[(size_t)k];
        rhs[(size_t)i] = t / A[(size_t)i * f + i];
      }
      for (int i = f - 1; i >= 0; --i) {
        double t = rhs[(size_t)i];
        for (int k = i + 1; k < f; ++k) t -= A[(size_t)k * f + i] * rhs[(size_t)k];
        rhs[(size_t)i] = t / A[(size_t)i * f + i];
      }
      bool inside = true;
      for (int i = 0; i < f; ++i) inside = inside && std::fabs(rhs[(size_t)i]) <= big_M;
      if (inside)
        for (int i = 0; i < f; ++i) b[fr[(size_t)i]] = rhs[(size_t)i];
    }
  }
  double val = 0.0;
  for (int r = 0; r < m; ++r) {
    double t = 0.0;
    for (int k = 0; k < m; ++k) t += H[(size_t)cols[r] * p + cols[k]] * b[k];
    val += b[r] * (0.5 * t - c[cols[r]]);
  }
  return val;
}

// The quadratic value and coefficients of the support `mask` (groups in search order), inside the box.  Columns that depend
// on earlier ones of the support stay at zero.  beta: [p] in search order.
// (A template over the mask: the wide mode's supports draw their at most L0_PMAX independent columns from up to
// L0_WIDE_PMAX; *overflow, when asked for, says that the support holds more independent columns than the factor has rows.)
template <class Mask>
inline double l0_support_of(const double* H, const double* c, int p, const std::vector<int>& gstart, Mask mask, double big_M, bool polish,
                            double* beta, bool* overflow = nullptr) {
  L0Factor f(H, c, p);
  const int ng = (int)gstart.size() - 1;
  bool over = false;
  for (int g = 0; g < ng; ++g)
    if (l0m_test(mask, g))
      for (int j = gstart[(size_t)g]; j < gstart[(size_t)g + 1]; ++j) {
        (void)f.push(j);
        over = over || f.overflow;
      }
  if (overflow) *overflow = over;
  for (int j = 0; j < p; ++j) beta[j] = 0.0;
  double b[L0_PMAX];
  f.solve(b);
  double val = -0.5 * f.ss;
  bool outside = false;
  for (int k = 0; k < f.m; ++k) outside = outside || std::fabs(b[k]) > big_M;
  if (outside) val = l0_boxed(H, c, p, f.col, f.m, big_M, polish, b);
  for (int k = 0; k < f.m; ++k) beta[f.col[k]] = b[k];
  return val;
}
inline double l0_support(const double* H, const double* c, int p, const std::vector<int>& gstart, unsigned long long mask, double big_M,
                  bool polish, double* beta) {
  return l0_support_of(H, c, p, gstart, mask, big_M, polish, beta);
}

// The unconstrained value on ALL columns, q_all of the subtree bound: a factor of up to L0_WIDE_PMAX rows, dependent columns
// skipped by the pivot rule.  (On the heap: 128 KiB of factor.)
inline double l0_q_all(const double* H, const double* c, int p) {
  if (p <= L0_PMAX) {
    L0Factor f(H, c, p);
    for (int j = 0; j < p; ++j) (void)f.push(j);
    return -0.5 * f.ss;
  }
  auto f = std::make_unique<L0FactorT<L0_WIDE_PMAX>>(H, c, p);
  for (int j = 0; j < p; ++j) (void)f->push(j);
  return -0.5 * f->ss;
}

// The wide mode's capacity rule (section "Capacity" of DESIGN 4d).  cut = c_min + 1, c_min the smallest number of groups
// held where an include was refused because the factor was full; 0: none was.  Every support below such a refusal has at
// least c_min + 1 groups and a quadratic value of at least q_all, so nothing unsearched is below q_all + alpha cut.
constexpr double l0_capacity_bound(double q_all, double alpha, int cut) { return q_all + alpha * (double)cut; }
constexpr bool l0_capacity_proven(double objective, double q_all, double alpha, int cut) {
  return cut == 0 || objective <= l0_capacity_bound(q_all, alpha, cut);
}

// ---- exclusion bound (slm_solve_l0_xb, slm_solve_l0_xb_wide; DESIGN 4d "Exclusion bound") ------------------------------------
//
// With P = H^-1 and bhat = P c (q_all = -1/2 c^T bhat), every support S that avoids the excluded columns E has
//     q(S) >= q(all \ E) = q_all + 1/2 bhat_E^T (P_EE)^-1 bhat_E = q_all + 1/2 ||w'||^2,   w' = L'^-1 bhat_E,  L' L'^T = P_EE
// (q is monotone in the support; the block inverse of H).  Along a depth-first path E grows in the order of the decisions, so
// L' grows by the append of L0FactorT on (P, bhat) instead of (H, c) -- the kernel keeps it in a second register row of
// L0_XCAP entries per lane.  ANY sub-collection of E gives a valid, weaker bound: a column whose pivot fails the pivot rule
// and every column that arrives when the factor holds L0_XCAP rows are left out of it.
// The increment comes from a P that is itself a rounded inverse, so it is trusted only up to the relative margin
//     delta = L0_XB_C kappa_1 2^-53,   kappa_1 = ||H||_1 ||P||_1;
// L0_XB_C is 16 times the worst overshoot of the unguarded fp64 increment over a long-double Cholesky of H on all \ E that
// tests/l0_bound_host_test.cpp measures (12.2 units of kappa_1 2^-53 1/2 ssx).  delta >= 1/2, or
// an H that is not positive definite on all columns under the pivot rule, runs the search with the plain bound q_all.
constexpr int L0_XCAP = 64;          // rows of the exclusion factor (columns of E the bound can use along one path)
constexpr double L0_XB_C = 256.0;     // >= 16 x 12.2, the worst overshoot measured
// what the kernel compares: the guarded q(all \ E).  One function for host and device (constexpr, as l0_l1_step is).
constexpr double l0_excl_bound(double q_all, double ssx, double delta) {
  return q_all + 0.5 * ssx * (1.0 - delta) - 1e-10 * ((q_all < 0.0 ? -q_all : q_all) + 0.5 * ssx);
}
struct L0ExclPlan {
  int reason = 0;  // 0: the exclusion bound runs; 1: H is not positive definite on all columns; 2: delta >= 1/2
  double kappa1 = 0.0, delta = 0.0;
  std::vector<double> P, bhat;  // [p][p], [p]: search order
};
inline double l0_excl_delta(double kappa1) { return L0_XB_C * kappa1 * 0x1p-53; }
// P, bhat, kappa_1 and delta from the factor of H on all columns in search order
inline L0ExclPlan l0_excl_plan(const double* H, const double* c, int p) {
  L0ExclPlan R;
  auto f = std::make_unique<L0FactorT<L0_WIDE_PMAX>>(H, c, p);
  for (int j = 0; j < p; ++j)
    if (!f->push(j)) {
      R.reason = 1;
      return R;
    }
  // X = L^-1 (lower triangle, column by column), P = X^T X
  std::vector<double> X((size_t)p * p, 0.0);
  for (int j = 0; j < p; ++j)
    for (int i = j; i < p; ++i) {
      double t = i == j ? 1.0 : 0.0;
      for (int k = j; k < i; ++k) t -= f->L[i][k] * X[(size_t)k * p + j];
      X[(size_t)i * p + j] = t / f->L[i][i];
    }
  R.P.assign((size_t)p * p, 0.0);
  for (int i = 0; i < p; ++i)
    for (int j = 0; j <= i; ++j) {
      double t = 0.0;
      for (int k = i; k < p; ++k) t += X[(size_t)k * p + i] * X[(size_t)k * p + j];
      R.P[(size_t)i * p + j] = R.P[(size_t)j * p + i] = t;
    }
  R.bhat.assign((size_t)p, 0.0);
  if (p > 0) f->solve(R.bhat.data());
  double h1 = 0.0, p1 = 0.0;
  for (int j = 0; j < p; ++j) {
    double sh = 0.0, sp = 0.0;
    for (int i = 0; i < p; ++i) {
      sh += std::fabs(H[(size_t)i * p + j]);
      sp += std::fabs(R.P[(size_t)i * p + j]);
    }
    h1 = std::max(h1, sh);
    p1 = std::max(p1, sp);
  }
  R.kappa1 = h1 * p1;
  R.delta = l0_excl_delta(R.kappa1);
  if (!(R.delta < 0.5)) R.reason = 2;
  return R;
}
// The exclusion factor as the kernel keeps it: L0FactorT on (P, bhat) with L0_XCAP rows; push() refuses a column the pivot
// rule skips and every column once the rows are full, and ss is ssx = ||w'||^2.
using L0ExclFactor = L0FactorT<L0_XCAP>;

// Greedy forward selection over the groups (H, c, gstart and the hierarchy needo in search order), up to K of them: one
// admissible support per size, handed to visit(size, support, value) with the value value_of(support) gives it (the kernel's
// own valuation, no alpha term); and, when K reaches the group count, the support of every group -- the one whose value can
// meet the bound q_all exactly.
// Wide mode: a group whose columns would not fit in the factor's L0_PMAX rows is no candidate, and the support of every group
// is visited only when it fits.
template <class Mask, class ValueOf, class Visit>
void l0_greedy(const double* H, const double* c, int p, const std::vector<int>& gstart, const std::vector<Mask>& needo, int K,
               ValueOf value_of, Visit visit) {
  const int ng = (int)gstart.size() - 1;
  L0Factor f(H, c, p);
  Mask cur = l0m_none<Mask>();
  for (int step = 0; step < K; ++step) {
    int pick = -1;
    double pick_ss = f.ss;
    const int m0 = f.m;
    for (int g = 0; g < ng; ++g) {
      if (l0m_test(cur, g) || l0m_any_outside(needo[(size_t)g], cur)) continue;
      bool fits = true;
      for (int j = gstart[(size_t)g]; j < gstart[(size_t)g + 1]; ++j) {  // (dependent columns are skipped, as in the kernel)
        (void)f.push(j);
        fits = fits && !f.overflow;
      }
      if (fits && f.ss > pick_ss) {
        pick_ss = f.ss;
        pick = g;
      }
      f.pop_to(m0);
    }
    if (pick < 0) break;
    l0m_set(cur, pick);
    // (the factor keeps search order inside the kernel; the seed's value is taken the same way)
    visit(step + 1, cur, value_of(cur));
    for (int j = gstart[(size_t)pick]; j < gstart[(size_t)pick + 1]; ++j) (void)f.push(j);
  }
  if (K >= ng && ng > 0) {
    const Mask all_mask = l0m_below<Mask>(ng);
    f.pop_to(0);
    bool fits = true;
    for (int j = 0; j < p; ++j) {
      (void)f.push(j);
      fits = fits && !f.overflow;
    }
    if (fits) visit(ng, all_mask, value_of(all_mask));
  }
}

// ---- profile mode (slm_solve_l0_profile): the best support of every size from one search ------------------------------------
//
// values[k], k = 0 .. K: the best quadratic value over admissible supports of exactly k groups (values[0] = 0, +inf where no
// support of that size was held).  The two questions the table answers; ties go to the smaller k, and an all-+inf range
// answers 0 (the empty support is always there).
inline int l0_profile_best_subset(const double* values, int K_prime) {  // argmin_{k <= K'} values[k]
  int best = 0;
  for (int k = 1; k <= K_prime; ++k)
    if (values[k] < values[best]) best = k;
  return best;
}
inline int l0_profile_regularized(const double* values, int K, double alpha) {  // argmin_k values[k] + alpha k
  int best = 0;
  for (int k = 1; k <= K; ++k)
    if (values[k] + alpha * (double)k < values[best] + alpha * (double)best) best = k;
  return best;
}

// The pruning rule of the profile search, one set of functions for host and device (constexpr, as l0_l1_step is):
//     E(c) = min(0, min_{1 <= k <= c} q_k + alpha_min k),      cut below a node of cnt groups when q_all + alpha_min (cnt + 1) >= E(cnt).
// The kernel folds l0_profile_term with l0_profile_join across the lanes (a prefix-min); l0_profile_envelope is the same
// fold in a loop.  q: the incumbents of the sizes 1 .. c (q[k - 1] for size k).
constexpr double l0_profile_term(double qk, int k, double alpha_min) { return qk + alpha_min * (double)k; }
constexpr double l0_profile_join(double a, double b) { return b < a ? b : a; }
constexpr double l0_profile_envelope(const double* q, int c, double alpha_min) {
  double e = 0.0;
  for (int k = 1; k <= c; ++k) e = l0_profile_join(e, l0_profile_term(q[k - 1], k, alpha_min));
  return e;
}
constexpr bool l0_profile_cut(double q_all, double alpha_min, int cnt, double e_cnt) { return !(q_all + alpha_min * (double)(cnt + 1) < e_cnt); }

// ---- l1 mode (slm_solve_l0_l1, the reference's L1L0): eta ||beta||_1 joins the objective ------------------------------------
//
// One coordinate step of the descent, the kernel's own: clip(soft(b - g / h, eta / h), +-big_M).  A column of zeros (h = 0)
// keeps a zero coefficient.  (constexpr: the device code calls this very function.)
constexpr double l0_l1_step(double b, double g, double h, double eta, double big_M) {
  if (!(h > 0.0)) return 0.0;
  const double u = b - g / h, th = eta / h;
  const double s = u > th ? u - th : (u < -th ? u + th : 0.0);
  return s < -big_M ? -big_M : (s > big_M ? big_M : s);
}

// 1/2 b^T H_S b - c_S^T b + eta ||b||_1 on the columns `cols`
inline double l0_l1_value(const double* H, const double* c, int p, const int* cols, int m, double eta, const double* b) {
  double val = 0.0;
  for (int r = 0; r < m; ++r) {
    double t = 0.0;
    for (int k = 0; k < m; ++k) t += H[(size_t)cols[r] * p + cols[k]] * b[k];
    val += b[r] * (0.5 * t - c[cols[r]]) + eta * std::fabs(b[r]);
  }
  return val;
}

// min 1/2 b^T H_S b - c_S^T b + eta ||b||_1 over |b_j| <= big_M on the columns `cols` -- ANY columns of a support, dependent
// ones included (with an l1 term a dependent column can lower the value).  The kernel's descent with the kernel's stopping
// rule; b: in the start, out the point reached.  Returns the value the kernel computes, 1/2 sum b_r (g_r - c_r) + eta ||b||_1.
inline double l0_l1_descent(const double* H, const double* c, int p, const int* cols, int m, double eta, double big_M, double* b) {
  std::vector<double> g((size_t)m);
  for (int r = 0; r < m; ++r) b[r] = std::min(std::max(b[r], -big_M), big_M);
  for (int r = 0; r < m; ++r) {
    double t = -c[cols[r]];
    for (int k = 0; k < m; ++k) t += H[(size_t)cols[r] * p + cols[k]] * b[k];
    g[(size_t)r] = t;
  }
  for (int sweep = 0; sweep < L0_CD_SWEEPS; ++sweep) {
    double maxd = 0.0, maxb = 0.0;
    for (int k = 0; k < m; ++k) {
      const double nb = l0_l1_step(b[k], g[(size_t)k], H[(size_t)cols[k] * p + cols[k]], eta, big_M);
      const double dk = nb - b[k];
      if (dk != 0.0) {
        for (int r = 0; r < m; ++r) g[(size_t)r] += H[(size_t)cols[r] * p + cols[k]] * dk;
        b[k] = nb;
      }
      maxd = std::max(maxd, std::fabs(dk));
      maxb = std::max(maxb, std::fabs(nb));
    }
    if (maxd <= L0_CD_TOL * maxb || maxd == 0.0) break;
  }
  double val = 0.0;
  for (int r = 0; r < m; ++r) val += 0.5 * b[r] * (g[(size_t)r] - c[cols[r]]) + eta * std::fabs(b[r]);
  return val;
}

// Polish of a descent's point: the free, non-zero coordinates are solved exactly on their sign pattern,
//     H_FF x = c_F - eta sign(b_F) - H_FB b_B,
// with the bound ones (B) where they are and the zero ones at zero.  x is taken only when every sign and the box hold: it is
// then the minimiser over the face the descent's point lies in, so its value is not above that point's (to rounding).
// Returns the value of the point kept, computed from that point.
inline double l0_l1_polish(const double* H, const double* c, int p, const int* cols, int m, double eta, double big_M, double* b) {
  const double v0 = l0_l1_value(H, c, p, cols, m, eta, b);  // (what is returned whenever the point stays as it is)
  std::vector<int> fr;
  for (int k = 0; k < m; ++k)
    if (b[k] != 0.0 && std::fabs(b[k]) < big_M) fr.push_back(k);
  const int f = (int)fr.size();
  if (f == 0) return v0;
  std::vector<double> A((size_t)f * f), x((size_t)f);
  for (int i = 0; i < f; ++i) {
    const int ci = cols[fr[(size_t)i]];
    double t = c[ci] - (b[fr[(size_t)i]] > 0.0 ? eta : -eta);
    for (int k = 0; k < m; ++k)
      if (b[k] != 0.0 && std::fabs(b[k]) >= big_M) t -= H[(size_t)ci * p + cols[k]] * b[k];
    x[(size_t)i] = t;
    for (int j = 0; j < f; ++j) A[(size_t)i * f + j] = H[(size_t)ci * p + cols[fr[(size_t)j]]];
  }
  for (int i = 0; i < f; ++i)  // Cholesky of the free block, in place; a block that is not definite keeps the descent's point
    for (int j = 0; j <= i; ++j) {
      double t = A[(size_t)i * f + j];
      for (int k = 0; k < j; ++k) t -= A[(size_t)i * f + k] * A[(size_t)j * f + k];
      if (i == j) {
        if (!(t > L0_PIVOT * A[(size_t)i * f + i])) return v0;
        A[(size_t)i * f + i] = std::sqrt(t);
      } else {
        A[(size_t)i * f + j] = t / A[(size_t)j * f + j];
      }
    }
  for (int i = 0; i < f; ++i) {
    double t = x[(size_t)i];
    for (int k = 0; k < i; ++k) t -= A[(size_t)i * f + k] * x[(size_t)k];
    x[(size_t)i] = t / A[(size_t)i * f + i];
  }
  for (int i = f - 1; i >= 0; --i) {
    double t = x[(size_t)i];
    for (int k = i + 1; k < f; ++k) t -= A[(size_t)k * f + i] * x[(size_t)k];
    x[(size_t)i] = t / A[(size_t)i * f + i];
  }
  std::vector<double> nb(b, b + m);
  for (int i = 0; i < f; ++i) {
    const double xi = x[(size_t)i], bi = b[fr[(size_t)i]];
    if (!((bi > 0.0 ? xi > 0.0 : xi < 0.0) && std::fabs(xi) <= big_M)) return v0;
    nb[(size_t)fr[(size_t)i]] = xi;
  }
  for (int k = 0; k < m; ++k) b[k] = nb[(size_t)k];
  return l0_l1_value(H, c, p, cols, m, eta, b);
}

// f(S) of the support `mask` (groups in search order) in l1 mode, and its coefficients: the descent over ALL its columns from
// the back-substituted beta of the independent ones (clipped; zero on the columns the pivot rule skipped), as the kernel
// values a node.  beta: [p] in search order.
inline double l0_l1_support(const double* H, const double* c, int p, const std::vector<int>& gstart, unsigned long long mask, double eta,
                            double big_M, bool polish, double* beta) {
  L0Factor f(H, c, p);
  const int ng = (int)gstart.size() - 1;
  int cols[L0_PMAX];
  int na = 0;
  for (int g = 0; g < ng; ++g)
    if ((mask >> g) & 1)
      for (int j = gstart[(size_t)g]; j < gstart[(size_t)g + 1]; ++j) {
        (void)f.push(j);
        cols[na++] = j;
      }
  for (int j = 0; j < p; ++j) beta[j] = 0.0;
  double bs[L0_PMAX], b[L0_PMAX];
  f.solve(bs);
  for (int r = 0; r < na; ++r) {
    b[r] = 0.0;
    for (int k = 0; k < f.m; ++k)
      if (f.col[k] == cols[r]) b[r] = bs[k];
  }
  double val = l0_l1_descent(H, c, p, cols, na, eta, big_M, b);
  if (polish) val = l0_l1_polish(H, c, p, cols, na, eta, big_M, b);
  for (int r = 0; r < na; ++r) beta[cols[r]] = b[r];
  return val;
}

// The same for a mask of either width (slm_solve_l0_l1_profile, _profile_wide): the support's at most L0_PMAX columns are drawn
// from up to L0_WIDE_PMAX.  A column that arrives when the list holds L0_PMAX is left out and sets *overflow (the entries refuse
// such a call before anything runs; at p <= L0_PMAX it cannot happen, and the result is the narrow function's bit for bit).
template <class Mask>
inline double l0_l1_support_of(const double* H, const double* c, int p, const std::vector<int>& gstart, Mask mask, double eta, double big_M,
                               bool polish, double* beta, bool* overflow = nullptr) {
  L0Factor f(H, c, p);
  const int ng = (int)gstart.size() - 1;
  int cols[L0_PMAX];
  int na = 0;
  bool over = false;
  for (int g = 0; g < ng; ++g)
    if (l0m_test(mask, g))
      for (int j = gstart[(size_t)g]; j < gstart[(size_t)g + 1]; ++j) {
        if (na == L0_PMAX) {
          over = true;
          continue;
        }
        (void)f.push(j);
        cols[na++] = j;
      }
  if (overflow) *overflow = over;
  for (int j = 0; j < p; ++j) beta[j] = 0.0;
  double bs[L0_PMAX], b[L0_PMAX];
  f.solve(bs);
  for (int r = 0; r < na; ++r) {
    b[r] = 0.0;
    for (int k = 0; k < f.m; ++k)
      if (f.col[k] == cols[r]) b[r] = bs[k];
  }
  double val = l0_l1_descent(H, c, p, cols, na, eta, big_M, b);
  if (polish) val = l0_l1_polish(H, c, p, cols, na, eta, big_M, b);
  for (int r = 0; r < na; ++r) beta[cols[r]] = b[r];
  return val;
}

// A proven lower bound on f(all columns) = min_b 1/2 b^T G b - c^T b + eta ||b||_1 (the box can only raise it): the larger of
// q_all and the lasso dual value at a feasible point.  With the primal 1/(2n)||y - X b||^2 + eta ||b||_1 = f + yy / 2
// (yy = y^T W y / n), the dual is  max D(nu) = yy/2 - n/2 ||nu - y/n||^2  over ||X^T nu||_inf <= eta.  For any b,
// nu = s (y - X b) / n has X^T nu = -s (G b - c), feasible for s = min(1, eta / ||G b - c||_inf), and
//     D(nu) - yy/2 = -1/2 s^2 rr + s ry - 1/2 yy,    rr = yy - 2 c^T b + b^T G b,  ry = yy - c^T b
// (at eta -> 0, s = 1 and b the least-squares solution this is -1/2 c^T b = q_all).  b comes from the descent on all
// columns without the box; only its quality, never its validity, depends on how far that descent got.  The value is
// lowered by a margin that covers the rounding of the sums and of a Gram that is itself a rounded product.  Up to
// L0_WIDE_PMAX columns (the wide l1 profile).
inline double l0_l1_lower_bound(const double* G, const double* c, int p, double yy, double eta, double q_all) {
  if (p <= 0 || p > L0_WIDE_PMAX || !(eta > 0.0)) return q_all;
  int cols[L0_WIDE_PMAX];
  double b[L0_WIDE_PMAX];
  for (int j = 0; j < p; ++j) {
    cols[j] = j;
    b[j] = 0.0;
  }
  (void)l0_l1_descent(G, c, p, cols, p, eta, HUGE_VAL, b);
  double cb = 0.0, bGb = 0.0, ginf = 0.0, scale = std::fabs(yy);
  for (int i = 0; i < p; ++i) {
    double t = 0.0, ta = 0.0;
    for (int j = 0; j < p; ++j) {
      t += G[(size_t)i * p + j] * b[j];
      ta += std::fabs(G[(size_t)i * p + j] * b[j]);
    }
    ginf = std::max(ginf, std::fabs(t - c[i]));
    cb += c[i] * b[i];
    bGb += b[i] * t;
    scale += 2.0 * std::fabs(c[i] * b[i]) + std::fabs(b[i]) * ta;
  }
  const double s = ginf > eta ? eta / ginf : 1.0;
  const double rr = yy - 2.0 * cb + bGb, ry = yy - cb;
  const double dual = -0.5 * s * s * rr + s * ry - 0.5 * yy - 1e-10 * scale;
  return dual > q_all && std::isfinite(dual) ? dual : q_all;
}

// ---- constrained mode (slm_solve_l0_constrained): linear constraints on the coefficients -------------------------------------
//
//     f(S) = min 1/2 b^T H_S b - c_S^T b   over   blo_j <= b_j <= bhi_j  (a box that contains 0),   lo <= A_S b <= hi  (m rows)
//
// and +inf when no b on S is feasible.  H is positive definite on ALL columns (l0_con_pd: the call is refused otherwise), so
// no column is ever skipped.  q(S) = -1/2 ||w||^2 <= f(S) stays the kernel's filter; a node that passes it is valued by the
// splitting below (the augmented Lagrangian of the rows, one clipped coordinate sweep per multiplier step), the same on the
// host (l0_con_solve: the seed, the bound on all columns, the winner) and in the kernel.  Every sweep ends with the dual value
//     D_S(y, mu) = -1/2 ||L_S^-1 (c_S - A_S^T y - mu)||^2 - sum_i (hi_i y_i^+ - lo_i y_i^-) - sum_j (bhi_j mu_j^+ - blo_j mu_j^-)  <=  f(S)
// at y = rho u (signs admissible by construction) and mu = the multipliers of the clipped coordinates: weak duality, for ANY
// admissible (y, mu), so how far the sweeps got decides only how tight it is.  A candidate ends VALUED (rows within
// L0_CON_TOL of their scale, primal value within L0_CON_TOL of D), REJECTED (D - margin above what it has to beat) or
// UNSETTLED (the sweep cap ran out: D - margin is a lower bound on that one support).
constexpr int L0_CON_MMAX = 64;        // rows of A
constexpr double L0_CON_TOL = 1e-9;    // feasibility and duality gap of a valued candidate, relative
constexpr int L0_CON_SWEEPS = 20000;   // sweep cap of one candidate (max_qp_sweeps <= 0)

// The pieces host and device share (constexpr, as l0_l1_step is: the device code calls these very functions).
constexpr double l0_con_abs(double v) { return v < 0.0 ? -v : v; }
constexpr double l0_con_clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }
// one row's term of the support function, hi y^+ - lo y^-; +inf for a multiplier whose sign the row does not admit
constexpr double l0_con_sigma(double y, double lo, double hi) {
  return y > 0.0 ? (hi < __builtin_inf() ? hi * y : __builtin_inf()) : (y < 0.0 ? (lo > -__builtin_inf() ? lo * y : __builtin_inf()) : 0.0);
}
// the multiplier of a clipped coordinate: gl = (H b - c + A^T y)_j, taken where the bound and the sign agree
constexpr double l0_con_box_mu(double b, double gl, double blo, double bhi) {
  return (b >= bhi && gl < 0.0) || (b <= blo && gl > 0.0) ? -gl : 0.0;
}
// a coordinate step on the augmented Lagrangian: g the entry of H b - c plus rho A_k^T (A b - s + u), curv = H_kk + rho ||A_k||^2
constexpr double l0_con_step(double b, double g, double curv, double blo, double bhi) { return l0_con_clip(b - g / curv, blo, bhi); }
// a row's violation relative to its scale (the rows of A have unit norm; maxb = the larger of ||b||_inf and the unconstrained minimiser's)
constexpr double l0_con_violation(double t, double lo, double hi, double maxb) {
  const double v = lo - t > t - hi ? lo - t : t - hi;
  if (!(v > 0.0)) return 0.0;
  double sc = maxb;
  if (lo > -__builtin_inf() && l0_con_abs(lo) > sc) sc = l0_con_abs(lo);
  if (hi < __builtin_inf() && l0_con_abs(hi) > sc) sc = l0_con_abs(hi);
  return sc > 0.0 ? v / sc : __builtin_inf();
}
// The dual value from zz = ||L^-1 (c - A^T y - mu)||^2, sigma = the sum of the support-function terms and asum = the sum of
// their magnitudes: raw, and lowered by the rounding margin (1e-10 of the sum of its terms' magnitudes, as
// l0_l1_lower_bound does it) -- `bound` is what is compared.
struct L0ConDual {
  double raw, bound, mag;
};
constexpr L0ConDual l0_con_dual(double zz, double sigma, double asum) {
  const double mag = 0.5 * zz + asum;
  return L0ConDual{-0.5 * zz - sigma, -0.5 * zz - sigma - 1e-10 * mag, mag};
}
// valued: the rows within L0_CON_TOL of their scale, the gap (either way: a point that undercuts D is not feasible enough) within L0_CON_TOL of the dual's terms and of qmag = 1/2 ||w||^2, the
// size of the support's unconstrained value (a support whose optimum is b = 0 has no other scale)
constexpr bool l0_con_valued(double primal, const L0ConDual& d, double viol, double qmag) {
  return viol <= L0_CON_TOL && l0_con_abs(primal - d.raw) <= L0_CON_TOL * (d.mag + qmag);
}

struct L0ConProblem {
  const double* H;  // [p][p], search order
  const double* c;  // [p]
  int p;
  const double* A;  // [m][p] row-major, search order, every non-zero row scaled to unit norm
  int m;
  const double *lo, *hi;    // [m] (scaled with their rows)
  const double *blo, *bhi;  // [p]: blo_j <= 0 <= bhi_j
  double rho;
  int max_sweeps;  // <= 0: L0_CON_SWEEPS
};
struct L0ConPoint {
  int outcome = 2;  // 0 valued, 1 rejected (infeasible supports included), 2 unsettled
  double primal = HUGE_VAL, bound = -HUGE_VAL;  // the point's value; D - margin at exit, a lower bound on f(S) however it ended
  int sweeps = 0;
  bool polished = false;
  std::vector<double> beta, mu, y;  // [ms], [ms], [m]
};

// H positive definite on all columns, under the kernel's pivot rule in search order (fact 4 of DESIGN 4d "Constrained mode")
inline bool l0_con_pd(const double* H, const double* c, int p) {
  auto f = std::make_unique<L0Factor>(H, c, p);
  for (int j = 0; j < p; ++j)
    if (!f->push(j)) return false;
  return true;
}
// the augmented Lagrangian's weight: rho ||A||_F^2 = tr H
inline double l0_con_rho(const double* H, int p, const double* A, int m) {
  double trH = 0.0, trK = 0.0;
  for (int j = 0; j < p; ++j) trH += H[(size_t)j * p + j];
  for (size_t e = 0; e < (size_t)m * p; ++e) trK += A[e] * A[e];
  return trH > 0.0 && trK > 0.0 ? trH / trK : 1.0;
}
// no feasible b has a larger value: sum |c_j| B_j + 1/2 sum |H_ij| B_i B_j, B_j = max(-blo_j, bhi_j) (+inf with an open box)
inline double l0_con_value_cap(const double* H, const double* c, int p, const double* blo, const double* bhi) {
  double v = 0.0;
  for (int i = 0; i < p; ++i) {
    const double Bi = std::max(-blo[i], bhi[i]);
    if (Bi == 0.0) continue;
    v += std::fabs(c[i]) * Bi;
    for (int j = 0; j < p; ++j) {
      const double Bj = std::max(-blo[j], bhi[j]);
      if (Bj != 0.0) v += 0.5 * std::fabs(H[(size_t)i * p + j]) * Bi * Bj;
    }
  }
  return v;
}

// f(S) on the columns `cols` by the splitting, as the kernel values a node.  reject_above: the solve stops as REJECTED once
// D - margin is above it (+inf: never).
inline L0ConPoint l0_con_solve(const L0ConProblem& P, const int* cols, int ms, double reject_above) {
  L0ConPoint R;
  const int m = P.m, p = P.p;
  R.beta.assign((size_t)ms, 0.0);
  R.mu.assign((size_t)ms, 0.0);
  R.y.assign((size_t)m, 0.0);
  for (int i = 0; i < m; ++i) {  // a row that is zero on the support and excludes 0: infeasible without a solve
    bool zero = true;
    for (int r = 0; r < ms; ++r) zero = zero && P.A[(size_t)i * p + cols[r]] == 0.0;
    if (zero && (P.lo[i] > 0.0 || P.hi[i] < 0.0)) {
      R.outcome = 1;
      R.bound = HUGE_VAL;
      return R;
    }
  }
  auto f = std::make_unique<L0Factor>(P.H, P.c, p);
  for (int r = 0; r < ms; ++r)
    if (!f->push(cols[r])) return R;  // (cannot happen once l0_con_pd passed)
  std::vector<double> b((size_t)ms), g((size_t)ms), curv((size_t)ms), t((size_t)m, 0.0), s((size_t)m), u((size_t)m, 0.0), z((size_t)ms);
  if (ms > 0) f->solve(b.data());
  double bref = 0.0;  // the size of the unconstrained minimiser: the scale of a row that binds at b = 0
  for (int r = 0; r < ms; ++r) bref = std::max(bref, std::fabs(b[(size_t)r]));
  for (int r = 0; r < ms; ++r) b[(size_t)r] = l0_con_clip(b[(size_t)r], P.blo[cols[r]], P.bhi[cols[r]]);
  for (int r = 0; r < ms; ++r) {
    double tt = -P.c[cols[r]], a2 = 0.0;
    for (int k = 0; k < ms; ++k) tt += P.H[(size_t)cols[r] * p + cols[k]] * b[(size_t)k];
    for (int i = 0; i < m; ++i) a2 += P.A[(size_t)i * p + cols[r]] * P.A[(size_t)i * p + cols[r]];
    g[(size_t)r] = tt;
    curv[(size_t)r] = P.H[(size_t)cols[r] * p + cols[r]] + P.rho * a2;
  }
  for (int i = 0; i < m; ++i) {
    for (int k = 0; k < ms; ++k) t[(size_t)i] += P.A[(size_t)i * p + cols[k]] * b[(size_t)k];
    s[(size_t)i] = l0_con_clip(t[(size_t)i], P.lo[i], P.hi[i]);
  }
  const int cap = P.max_sweeps > 0 ? P.max_sweeps : L0_CON_SWEEPS;
  for (int sweep = 1; sweep <= cap; ++sweep) {
    R.sweeps = sweep;
    double maxb = bref;
    for (int k = 0; k < ms; ++k) {
      double pen = 0.0;
      for (int i = 0; i < m; ++i) pen += P.A[(size_t)i * p + cols[k]] * (t[(size_t)i] - s[(size_t)i] + u[(size_t)i]);
      const double nb = l0_con_step(b[(size_t)k], g[(size_t)k] + P.rho * pen, curv[(size_t)k], P.blo[cols[k]], P.bhi[cols[k]]);
      const double dk = nb - b[(size_t)k];
      if (dk != 0.0) {
        for (int r = 0; r < ms; ++r) g[(size_t)r] += P.H[(size_t)cols[r] * p + cols[k]] * dk;
        for (int i = 0; i < m; ++i) t[(size_t)i] += P.A[(size_t)i * p + cols[k]] * dk;
        b[(size_t)k] = nb;
      }
      maxb = std::max(maxb, std::fabs(nb));
    }
    double sigma = 0.0, asum = 0.0, viol = 0.0;
    for (int i = 0; i < m; ++i) {  // the multiplier step: s <- clip(A b + u), u <- A b + u - s, y = rho u
      const double v = t[(size_t)i] + u[(size_t)i];
      s[(size_t)i] = l0_con_clip(v, P.lo[i], P.hi[i]);
      u[(size_t)i] = v - s[(size_t)i];
      R.y[(size_t)i] = P.rho * u[(size_t)i];
      const double st = l0_con_sigma(R.y[(size_t)i], P.lo[i], P.hi[i]);
      sigma += st;
      asum += std::fabs(st);
      viol = std::max(viol, l0_con_violation(t[(size_t)i], P.lo[i], P.hi[i], maxb));
    }
    double primal = 0.0, zz = 0.0;
    for (int r = 0; r < ms; ++r) {  // z = L^-1 (c - A^T y - mu), row by row
      double aty = 0.0;
      for (int i = 0; i < m; ++i) aty += P.A[(size_t)i * p + cols[r]] * R.y[(size_t)i];
      R.mu[(size_t)r] = l0_con_box_mu(b[(size_t)r], g[(size_t)r] + aty, P.blo[cols[r]], P.bhi[cols[r]]);
      const double st = l0_con_sigma(R.mu[(size_t)r], P.blo[cols[r]], P.bhi[cols[r]]);
      sigma += st;
      asum += std::fabs(st);
      double v = P.c[cols[r]] - aty - R.mu[(size_t)r];
      for (int k = 0; k < r; ++k) v -= f->L[r][k] * z[(size_t)k];
      z[(size_t)r] = v / f->L[r][r];
      zz += z[(size_t)r] * z[(size_t)r];
      primal += 0.5 * b[(size_t)r] * (g[(size_t)r] - P.c[cols[r]]);
    }
    const L0ConDual d = l0_con_dual(zz, sigma, asum);
    R.bound = d.bound;
    R.primal = primal;
    if (d.bound > reject_above) {
      R.outcome = 1;
      break;
    }
    if (l0_con_valued(primal, d, viol, 0.5 * f->ss)) {
      R.outcome = 0;
      break;
    }
  }
  R.beta = b;
  return R;
}

// D_S(y, mu) at ANY multipliers (the kernel and l0_con_solve evaluate it at their own): -inf where a sign is not admissible
inline L0ConDual l0_con_dual_at(const L0ConProblem& P, const int* cols, int ms, const double* y /* [m] */, const double* mu /* [ms] */) {
  auto f = std::make_unique<L0Factor>(P.H, P.c, P.p);
  for (int r = 0; r < ms; ++r) (void)f->push(cols[r]);
  double sigma = 0.0, asum = 0.0, zz = 0.0;
  for (int i = 0; i < P.m; ++i) {
    const double st = l0_con_sigma(y[i], P.lo[i], P.hi[i]);
    sigma += st;
    asum += std::fabs(st);
  }
  std::vector<double> z((size_t)ms);
  for (int r = 0; r < ms && r < f->m; ++r) {
    const double st = l0_con_sigma(mu[r], P.blo[cols[r]], P.bhi[cols[r]]);
    sigma += st;
    asum += std::fabs(st);
    double v = P.c[cols[r]] - mu[r];
    for (int i = 0; i < P.m; ++i) v -= P.A[(size_t)i * P.p + cols[r]] * y[i];
    for (int k = 0; k < r; ++k) v -= f->L[r][k] * z[(size_t)k];
    z[(size_t)r] = v / f->L[r][r];
    zz += z[(size_t)r] * z[(size_t)r];
  }
  return l0_con_dual(zz, sigma, asum);
}

// Cholesky of a dense n x n matrix in place (lower triangle), pivots under the rule L0_PIVOT; and the two substitutions
inline bool l0_dense_chol(std::vector<double>& M, int n) {
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double t = M[(size_t)i * n + j];
      for (int k = 0; k < j; ++k) t -= M[(size_t)i * n + k] * M[(size_t)j * n + k];
      if (i == j) {
        if (!(t > L0_PIVOT * M[(size_t)i * n + i])) return false;
        M[(size_t)i * n + i] = std::sqrt(t);
      } else {
        M[(size_t)i * n + j] = t / M[(size_t)j * n + j];
      }
    }
  return true;
}
inline void l0_dense_fwd(const std::vector<double>& M, int n, double* x) {  // x <- L^-1 x
  for (int i = 0; i < n; ++i) {
    double t = x[i];
    for (int k = 0; k < i; ++k) t -= M[(size_t)i * n + k] * x[k];
    x[i] = t / M[(size_t)i * n + i];
  }
}
inline void l0_dense_bwd(const std::vector<double>& M, int n, double* x) {  // x <- L^-T x
  for (int i = n - 1; i >= 0; --i) {
    double t = x[i];
    for (int k = i + 1; k < n; ++k) t -= M[(size_t)k * n + i] * x[k];
    x[i] = t / M[(size_t)i * n + i];
  }
}

// Polish of a valued point (the pattern of l0_l1_polish): the face it lies in -- the rows with a non-zero multiplier and the
// equality rows held at their bound, the clipped coordinates where they are -- is solved exactly,
//     [H_FF  A_WF^T] [b_F   ]   [c_F - H_FB b_B ]
//     [A_WF  0     ] [lambda] = [d_W - A_WB b_B ],
// and that point is taken only when every row and the box hold and every multiplier has the sign of its side.  It is then
// the minimiser on S (the KKT conditions hold to rounding), whatever the splitting's last digits were.  Returns whether
// the point was taken; R.beta, R.y (the rows' multipliers) and R.mu (the box multipliers) then describe it.
inline bool l0_con_polish(const L0ConProblem& P, const int* cols, int ms, L0ConPoint& R) {
  const int m = P.m, p = P.p;
  std::vector<int> W, F, B;
  std::vector<double> d;
  for (int i = 0; i < m; ++i) {
    if (P.lo[i] == P.hi[i]) {
      bool zero = true;
      for (int r = 0; r < ms; ++r) zero = zero && P.A[(size_t)i * p + cols[r]] == 0.0;
      if (zero) continue;
      W.push_back(i);
      d.push_back(P.lo[i]);
    } else if (R.y[(size_t)i] != 0.0) {
      W.push_back(i);
      d.push_back(R.y[(size_t)i] > 0.0 ? P.hi[i] : P.lo[i]);
    }
  }
  for (int r = 0; r < ms; ++r) (R.beta[(size_t)r] <= P.blo[cols[r]] || R.beta[(size_t)r] >= P.bhi[cols[r]] ? B : F).push_back(r);
  const int nf = (int)F.size(), nw = (int)W.size();
  std::vector<double> b(R.beta), lam((size_t)nw, 0.0);
  if (nf > 0) {
    std::vector<double> HF((size_t)nf * nf), rhs((size_t)nf);
    for (int i = 0; i < nf; ++i) {
      const int ci = cols[F[(size_t)i]];
      double t = P.c[ci];
      for (int r : B) t -= P.H[(size_t)ci * p + cols[r]] * b[(size_t)r];
      rhs[(size_t)i] = t;
      for (int j = 0; j < nf; ++j) HF[(size_t)i * nf + j] = P.H[(size_t)ci * p + cols[F[(size_t)j]]];
    }
    if (!l0_dense_chol(HF, nf)) return false;
    l0_dense_fwd(HF, nf, rhs.data());  // w0 = L^-1 rhs
    if (nw > 0) {
      if (nw > nf) return false;
      std::vector<double> Y((size_t)nw * nf), S((size_t)nw * nw);  // Y row i = L^-1 A_{W_i, F}^T
      for (int i = 0; i < nw; ++i) {
        for (int j = 0; j < nf; ++j) Y[(size_t)i * nf + j] = P.A[(size_t)W[(size_t)i] * p + cols[F[(size_t)j]]];
        l0_dense_fwd(HF, nf, &Y[(size_t)i * nf]);
        double t = d[(size_t)i];
        for (int r : B) t -= P.A[(size_t)W[(size_t)i] * p + cols[r]] * b[(size_t)r];
        double yw = 0.0;
        for (int j = 0; j < nf; ++j) yw += Y[(size_t)i * nf + j] * rhs[(size_t)j];
        lam[(size_t)i] = yw - t;
      }
      for (int i = 0; i < nw; ++i)
        for (int j = 0; j < nw; ++j) {
          double t = 0.0;
          for (int k = 0; k < nf; ++k) t += Y[(size_t)i * nf + k] * Y[(size_t)j * nf + k];
          S[(size_t)i * nw + j] = t;
        }
      if (!l0_dense_chol(S, nw)) return false;
      l0_dense_fwd(S, nw, lam.data());
      l0_dense_bwd(S, nw, lam.data());
      for (int i = 0; i < nw; ++i)
        for (int j = 0; j < nf; ++j) rhs[(size_t)j] -= Y[(size_t)i * nf + j] * lam[(size_t)i];
    }
    l0_dense_bwd(HF, nf, rhs.data());
    for (int i = 0; i < nf; ++i) b[(size_t)F[(size_t)i]] = rhs[(size_t)i];
  } else if (nw > 0) {
    return false;  // (every coordinate clipped and rows active: the multipliers of the splitting stay)
  }
  // the conditions that make the face point the minimiser
  double maxb = 0.0;
  for (int r = 0; r < ms; ++r) maxb = std::max(maxb, std::fabs(b[(size_t)r]));
  for (int i : F)
    if (!(b[(size_t)i] >= P.blo[cols[i]] && b[(size_t)i] <= P.bhi[cols[i]])) return false;
  for (int i = 0; i < m; ++i) {
    double t = 0.0;
    for (int r = 0; r < ms; ++r) t += P.A[(size_t)i * p + cols[r]] * b[(size_t)r];
    if (l0_con_violation(t, P.lo[i], P.hi[i], maxb) > 1e-12) return false;
  }
  std::vector<double> y((size_t)m, 0.0), mu((size_t)ms, 0.0);
  for (int i = 0; i < nw; ++i) {
    const int row = W[(size_t)i];
    if (P.lo[row] != P.hi[row] && (R.y[(size_t)row] > 0.0 ? lam[(size_t)i] < 0.0 : lam[(size_t)i] > 0.0)) return false;
    y[(size_t)row] = lam[(size_t)i];
  }
  for (int r : B) {
    double gl = -P.c[cols[r]];
    for (int k = 0; k < ms; ++k) gl += P.H[(size_t)cols[r] * p + cols[k]] * b[(size_t)k];
    for (int i = 0; i < m; ++i) gl += P.A[(size_t)i * p + cols[r]] * y[(size_t)i];
    const bool at_lo = b[(size_t)r] <= P.blo[cols[r]], at_hi = b[(size_t)r] >= P.bhi[cols[r]];
    if ((at_hi && !at_lo && gl > 0.0) || (at_lo && !at_hi && gl < 0.0)) return false;
    mu[(size_t)r] = -gl;
  }
  double val = 0.0;
  for (int r = 0; r < ms; ++r) {
    double t = 0.0;
    for (int k = 0; k < ms; ++k) t += P.H[(size_t)cols[r] * p + cols[k]] * b[(size_t)k];
    val += b[(size_t)r] * (0.5 * t - P.c[cols[r]]);
  }
  R.beta = b;
  R.y = y;
  R.mu = mu;
  R.primal = val;
  R.polished = true;
  return true;
}

// The columns of the support `mask` (groups in search order), in search order
inline int l0_con_columns(const std::vector<int>& gstart, unsigned long long mask, int* cols) {
  int ms = 0;
  for (int g = 0; g + 1 < (int)gstart.size(); ++g)
    if ((mask >> g) & 1)
      for (int j = gstart[(size_t)g]; j < gstart[(size_t)g + 1]; ++j) cols[ms++] = j;
  return ms;
}

// A proven lower bound on f(all columns), the subtree bound's F_lb: the larger of q_all and the dual value at the multipliers
// of a solve on all columns (whose quality decides how tight it is, never whether it holds; +inf when all columns together
// are infeasible -- every support then is).  all: that solve, for the seed's repair.
inline double l0_con_lower_bound(const L0ConProblem& P, double q_all, L0ConPoint* all = nullptr) {
  int cols[L0_PMAX];
  for (int j = 0; j < P.p; ++j) cols[j] = j;
  L0ConPoint R = l0_con_solve(P, cols, P.p, HUGE_VAL);
  const double lb = R.bound > q_all ? R.bound : q_all;  // (a NaN bound keeps q_all)
  if (all) *all = std::move(R);
  return lb;
}

// ---- the launch plan and what is read back (every entry of engine_l0.hip; tests/l0_launch_host_test.cpp) ---------------------
//
// The search's one block of 8-byte words, in this order:
//     control | best values | best supports | H | c | need | group starts | what a mode appends
// A wave owns `slots` results (1; profile mode 64, entry k - 1 for size k); a mask is `mask_words` words, the low one first.
// The host reads back the part before H.  The kernel's constants (control words, ticket prefix, waves per workgroup) are
// arguments: this header knows nothing of l0_kernels.hpp.
struct L0Layout {
  int d = 0, blocks = 0, waves = 0, slots = 1, mask_words = 1;
  size_t off_bv = 0, off_bm = 0, off_H = 0, off_c = 0, off_need = 0, off_gs = 0, words = 0;
  size_t append(size_t n) { return (words += n) - n; }  // a section of n words behind what is there; its offset
};
// (max_blocks: the most workgroups one problem may have -- two per CU for a problem that has the device to itself)
inline L0Layout l0_layout_capped(int p, int ng, long long max_blocks, int mask_words, int slots, int ctl_words, int prefix, int block_waves) {
  L0Layout y;
  y.d = std::min(ng, prefix);  // 2^d tickets, one per wave while they last: at least one workgroup, at most two per CU
  y.blocks = (int)std::max<long long>(1, std::min<long long>(max_blocks, ((1ll << y.d) + block_waves - 1) / block_waves));
  y.waves = y.blocks * block_waves;
  y.slots = slots;
  y.mask_words = mask_words;
  (void)y.append((size_t)ctl_words);
  y.off_bv = y.append((size_t)y.waves * slots);
  y.off_bm = y.append((size_t)mask_words * y.waves * slots);
  y.off_H = y.append((size_t)p * p);
  y.off_c = y.append((size_t)p);
  y.off_need = y.append((size_t)mask_words * ng);
  y.off_gs = y.append((size_t)ng + 1);
  return y;
}
inline L0Layout l0_layout(int p, int ng, int cus, int mask_words, int slots, int ctl_words, int prefix, int block_waves) {
  return l0_layout_capped(p, ng, 2ll * cus, mask_words, slots, ctl_words, prefix, block_waves);
}
// The batched profile (slm_solve_l0_profile_batch): `count` problems of one shape in one block, each a whole copy of the
// layout above, back to back.  `one` is a single problem's layout with its offsets relative to the copy; problem b's copy
// starts at word at(b) = b * stride.  The problems share the device: blocks_b = clamp(ceil(2^d / block_waves), 1,
// max(1, floor(2 cus / count))) workgroups each (one.blocks), so that the grid of count * blocks_b workgroups is resident
// at once like a single problem's.  count = 1 is l0_layout.
struct L0BatchLayout {
  L0Layout one;
  int count = 1;
  size_t stride = 0, words = 0;
  size_t at(int b) const { return (size_t)b * stride; }
  int grid() const { return count * one.blocks; }
};
inline L0BatchLayout l0_batch_layout(int count, int p, int ng, int cus, int mask_words, int slots, int ctl_words, int prefix, int block_waves) {
  L0BatchLayout B;
  B.count = count;
  B.one = l0_layout_capped(p, ng, 2ll * cus / count, mask_words, slots, ctl_words, prefix, block_waves);
  B.stride = B.one.words;
  B.words = B.stride * (size_t)count;
  return B;
}

// The profile grid (slm_solve_l0_profile_grid): one problem per (row set, eta), problem b = r * n_eta + e the row set r with
// etas[e] -- the row sets outermost, so that a row set's problems (one Gram, n_eta orders and seeds) lie side by side and every
// output's leading dimension is count * n_eta in that order.  At most L0_GRID_MAX problems: l0_batch_layout gives each
// max(1, 2 cus / problems) workgroups, so on a device of at least 64 CUs the whole grid is resident at once; below that every
// problem keeps its one workgroup, the grid exceeds 2 cus and runs in waves -- nothing in the kernel waits on another workgroup.
constexpr int L0_GRID_MAX = 128;      // problems of one grid launch
constexpr int L0_GRID_ROW_SETS = 16;  // row sets of one call: what the dataset's Gram store holds
constexpr int l0_grid_index(int r, int e, int n_eta) { return r * n_eta + e; }
constexpr int l0_grid_row_set(int b, int n_eta) { return b / n_eta; }
constexpr int l0_grid_eta(int b, int n_eta) { return b % n_eta; }
// What the grid entry refuses on top of the entries it generalises, in this order (0: nothing); *which: the offending eta.
enum L0GridRefusal { L0_GRID_OK = 0, L0_GRID_COUNT, L0_GRID_N_ETA, L0_GRID_NULL, L0_GRID_KIND, L0_GRID_T_WITH_L1, L0_GRID_ETA, L0_GRID_PROBLEMS };
inline L0GridRefusal l0_grid_check(long long count, long long n_eta, const double* etas, int eta_kind, bool has_T, int* which = nullptr) {
  if (count < 1 || count > L0_GRID_ROW_SETS) return L0_GRID_COUNT;
  if (n_eta < 1) return L0_GRID_N_ETA;
  if (!etas) return L0_GRID_NULL;
  if (eta_kind != 0 && eta_kind != 1) return L0_GRID_KIND;
  if (eta_kind == 1 && has_T) return L0_GRID_T_WITH_L1;
  if (count * n_eta > L0_GRID_MAX) return L0_GRID_PROBLEMS;  // (before etas is read: n_eta is then within bounds the caller meant)
  for (long long e = 0; e < n_eta; ++e)
    if (!(etas[e] >= 0.0) || !std::isfinite(etas[e])) {
      if (which) *which = (int)e;
      return L0_GRID_ETA;
    }
  return L0_GRID_OK;
}
inline L0BatchLayout l0_grid_layout(int count, int n_eta, int p, int ng, int cus, int slots, int ctl_words, int prefix, int block_waves) {
  return l0_batch_layout(count * n_eta, p, ng, cus, 1, slots, ctl_words, prefix, block_waves);
}

// Elimination of an intercept column from the Gram of [X | 1] on one row set (weights w, sum w = n_eff):
//     G <- G - g1 g1^T / G11,   c <- c - g1 c1 / G11,   yy <- yy - c1^2 / G11,      g1 = G[:, last], c1 = c[last], G11 = G[last][last]
// -- the Schur complement of the ones column, which is exactly weighted centring of X and y by that row set's own weighted
// means xmean = g1 / G11 and ymean = c1 / G11, so one Gram build per row set gives the centred problem of each.  The
// intercept that goes with coefficients beta is ymean - xmean^T beta.
// Cancellation: G_ij holds mean_i mean_j + cov_ij and the subtraction removes the first term, so the centred entry keeps a
// relative error of about 2^-53 (1 + mean_i mean_j / cov_ij): a column whose |mean| is 1e4 times its spread loses eight to
// nine of sixteen digits (tests/l0_batch_host_test.cpp measures 3.8e-7; centring X before the product does not).  Data far
// from the origin should be shifted by the caller.
// In: G [p][p], c [p] with the ones column LAST.  Out: Gs [(p - 1)][(p - 1)], cs, xmean [p - 1].  false: G11 is not positive.
inline bool l0_eliminate_last(const double* G, const double* c, int p, double yy, double* Gs, double* cs, double* yys, double* xmean,
                              double* ymean) {
  const int q = p - 1;
  const double g11 = G[(size_t)q * p + q], c1 = c[q];
  if (!(g11 > 0.0) || !std::isfinite(g11)) return false;
  for (int i = 0; i < q; ++i) {
    const double gi = G[(size_t)i * p + q];
    xmean[i] = gi / g11;
    cs[i] = c[i] - gi * c1 / g11;
    for (int j = 0; j < q; ++j) Gs[(size_t)i * q + j] = G[(size_t)i * p + j] - gi * G[(size_t)j * p + q] / g11;  // (symmetric when G is)
  }
  *ymean = c1 / g11;
  *yys = yy - c1 * c1 / g11;
  return true;
}
// the common sections of the host image h[y.words] (control, results and whatever is appended stay as they are)
template <class Mask>
inline void l0_fill_image(const L0Layout& y, const double* H, const double* c, int p, const std::vector<Mask>& needo,
                          const std::vector<int>& gstart, unsigned long long* h) {
  static_assert(sizeof(Mask) % sizeof(unsigned long long) == 0, "a mask is whole words, the low one first");
  memcpy(h + y.off_H, H, sizeof(double) * (size_t)p * p);
  memcpy(h + y.off_c, c, sizeof(double) * (size_t)p);
  if (!needo.empty()) memcpy(h + y.off_need, needo.data(), sizeof(Mask) * needo.size());
  for (size_t g = 0; g < gstart.size(); ++g) h[y.off_gs + g] = (unsigned long long)gstart[g];
}

// The tie rule of every comparison of two candidates: the lower value, then the lower support.  Two candidates at +inf are
// no tie: +inf says "nothing held" (a wave that found nothing stores +inf with an all-ones mask, the seed of an infeasible
// empty support is +inf with all ones), and whoever holds +inf keeps the mask it has -- which nobody reads.
template <class Mask>
inline bool l0_better(double v, Mask mk, double than_v, Mask than_mk) {
  return v < than_v || (v == than_v && v < HUGE_VAL && l0m_less(mk, than_mk));
}
// The winner among the seed (in val, mask) and result `slot` of every wave's `stride`, in a fixed order; h: the block as read back.
template <class Mask>
inline void l0_winner(const unsigned long long* h, size_t off_bv, size_t off_bm, int waves, int stride, int slot, double& val, Mask& mask) {
  for (int wv = 0; wv < waves; ++wv) {
    const size_t at = (size_t)wv * stride + slot;
    double v;
    Mask mk;
    memcpy(&v, h + off_bv + at, sizeof(double));
    memcpy(&mk, h + off_bm + at * (sizeof(Mask) / sizeof(unsigned long long)), sizeof(Mask));
    if (l0_better(v, mk, val, mask)) {
      val = v;
      mask = mk;
    }
  }
}

// A support in search order as the caller sees it: group gorder[k] for bit k.  count: the groups it holds.
template <class Mask>
inline Mask l0_caller_mask(Mask mask, const std::vector<int>& gorder, int* count = nullptr) {
  Mask out = l0m_none<Mask>();
  int n = 0;
  for (int k = 0; k < (int)gorder.size(); ++k)
    if (l0m_test(mask, k)) {
      ++n;
      l0m_set(out, gorder[(size_t)k]);
    }
  if (count) *count = n;
  return out;
}
// coefficients in search order to the caller's columns: cols[i] is the column at search position i
inline void l0_scatter(const double* beta_s, const std::vector<int>& cols, double* beta) {
  for (size_t i = 0; i < cols.size(); ++i) beta[cols[i]] = beta_s[i];
}
// 1/(2n)||X beta - y||_W^2 = 1/2 beta^T G beta - c^T beta + 1/2 yy (yy = y^T W y / n) from the Gram: no pass over X
inline double l0_gram_loss(const double* G, const double* c, int p, double yy, const double* beta) {
  double loss = 0.5 * yy;
  for (int i = 0; i < p; ++i) {
    if (beta[i] == 0.0) continue;
    double t = 0.0;
    for (int j = 0; j < p; ++j) t += G[(size_t)i * p + j] * beta[j];
    loss += beta[i] * (0.5 * t - c[i]);
  }
  return loss;
}

// ---- local search (slm_solve_l0_local; csrc/l0_local_kernels.hpp; tests/l0_local_host_test.cpp) ------------------------------
//
// The one part of the family that proves nothing: for a cell (alpha, eta), H = G + 2 eta I,
//     F(beta) = 1/2 beta^T H beta - c^T beta + alpha ||beta||_0   over |beta_j| <= big_M,
// cyclic coordinate descent with hard thresholding, then one-for-one swaps until none helps (DESIGN 4d "Local search").  The
// state is beta, r = c - H beta and d_j = H_jj.  l0_ls_coord and l0_ls_swap_better are the two decisions, shared with the
// kernel; l0_local_solve<false> is the whole rule without a device (the kernel's twin: the same sequence of changes, the same
// arithmetic up to the order of the final sums and the contraction of a multiply-add), l0_ls_polish the exact re-solve of a
// support inside the box that the entry runs on the winner.
constexpr int L0_LS_PMAX = 1024;             // columns: 16 slots of 64 lanes
constexpr int L0_LS_SLOTS = L0_LS_PMAX / 64;
constexpr int L0_LS_SWAPS = 10000;           // accepted swaps of one problem; reaching it marks the problem unconverged
constexpr double L0_LS_SWAP_TOL = 1e-10;     // a swap must gain this much, relative to max(|g_i|, alpha)
constexpr int L0_LS_MAX_PROBLEMS = 8192;     // (cell, start) problems of one call
constexpr int L0_LS_SWEEPS_OUT = 1, L0_LS_SWAPS_OUT = 2;  // bits of a problem's status word: which cap it reached
constexpr int L0_LS_ROW_SETS = 16;           // row sets of one slm_solve_l0_local_folds call: what the dataset's Gram store holds

// coordinate j given the others: u = r_j + d_j beta_j, b = clip(u / d_j), gain = u b - 1/2 d_j b^2 (what F without the alpha
// term falls by when beta_j goes from 0 to b)
struct L0LsCoord {
  double b, gain;
};
constexpr L0LsCoord l0_ls_coord(double u, double d, double big_M) {
  double b = u / d;
  b = b < -big_M ? -big_M : (b > big_M ? big_M : b);
  return L0LsCoord{b, u * b - 0.5 * d * b * b};
}
// the same coordinate with an l1 term lam |beta_j| in F ("local search with an l1 term", below; l0_local_solve<false, true>):
// s = sign(u) max(|u| - lam, 0), b = clip(s / d_j), gain = u b - 1/2 d_j b^2 - lam |b|.  lam = 0 gives l0_ls_coord's b and gain.
constexpr L0LsCoord l0_ls_coord_l1(double u, double d, double big_M, double lam) {
  const double au = u < 0.0 ? -u : u;
  const double s = au > lam ? (u < 0.0 ? lam - au : au - lam) : 0.0;
  double b = s / d;
  b = b < -big_M ? -big_M : (b > big_M ? big_M : b);
  return L0LsCoord{b, u * b - 0.5 * d * b * b - lam * (b < 0.0 ? -b : b)};
}
// the descent's rule: the new value of a coordinate
constexpr double l0_ls_threshold(const L0LsCoord& co, double alpha) { return co.gain > alpha ? co.b : 0.0; }
// the swap rule: column j (gain gj with i removed) replaces column i (gain gi with i removed)
constexpr bool l0_ls_swap_better(double gj, double gi, double alpha) {
  const double a = gi < 0.0 ? -gi : gi;
  return gj > gi + L0_LS_SWAP_TOL * (a > alpha ? a : alpha);
}

struct L0LsResult {
  double F = 0.0;  // the objective at the returned beta (the cardinality rule: Q, which has no alpha term)
  int sweeps = 0, swaps = 0, status = 0, nnz = 0;
  int grows = 0, drops = 0;  // the cardinality rule's: columns that entered in its grow step, that left in its shrink or descent
  long long changes = 0;     // columns of H applied to r after the start (one per coordinate change, two per swap): what the time goes to
};

// The rule on one problem: the kernel's twin, l0_local_kernel<CARD> without a device, laid out as the kernel is.  CARD false is
// the penalised rule of this section and `cell` the cell's alpha; CARD true the cardinality rule of "local subsets" below and
// `cell` its size k (k >= p is legal).  G: [p][ld] the Gram (symmetric; row j is read for column j), c: [p]; 2 eta goes on the
// diagonal here.  start: [p] inside the box, or NULL for zero.  beta: [p] out.  A column whose d_j <= L0_PIVOT max d stays zero.
// L1 (the penalised rule alone): lam ||beta||_1 joins F and every coordinate is l0_ls_coord_l1's -- nothing else changes.
template <bool CARD, bool L1 = false>
inline L0LsResult l0_local_solve(const double* G, size_t ld, const double* c, int p, std::conditional_t<CARD, int, double> cell, double eta,
                                 double big_M, double yy, bool swaps, const double* start, double* beta, double lam = 0.0) {
  static_assert(!(CARD && L1), "best subset with an l1 term is no estimator of the reference");
  L0LsResult R;
  auto coord = [&](double u, double dj) {
    if constexpr (L1)
      return l0_ls_coord_l1(u, dj, big_M, lam);
    else
      return l0_ls_coord(u, dj, big_M);
  };
  std::vector<double> r(c, c + p), d((size_t)p);
  const double alpha = CARD ? 0.0 : (double)cell, eta2 = 2.0 * eta;
  const int kmax = CARD ? (int)cell : 0;
  double dmax = 0.0;
  for (int j = 0; j < p; ++j) {
    d[(size_t)j] = G[(size_t)j * ld + j] + eta2;
    dmax = std::max(dmax, d[(size_t)j]);
  }
  for (int j = 0; j < p; ++j) {
    if (!(d[(size_t)j] > L0_PIVOT * dmax)) d[(size_t)j] = 0.0;  // (0 marks a column that stays out)
    beta[j] = start && d[(size_t)j] > 0.0 ? start[j] : 0.0;
  }
  auto axpy = [&](int j, double w) {  // r += w H[:, j]
    const double* row = G + (size_t)j * ld;
    for (int k = 0; k < p; ++k) r[(size_t)k] += w * (k == j ? row[k] + eta2 : row[k]);
    ++R.changes;
  };
  int nact = 0;  // (the cardinality rule's: the support's size)
  for (int j = 0; j < p; ++j)
    if (beta[j] != 0.0) {
      axpy(j, -beta[j]);
      ++nact;
    }
  R.changes = 0;  // (the start is not counted)
  const double tol = L0_CD_TOL * std::sqrt(yy);
  if (CARD) {
    // ---- shrink: while the support is larger than k its weakest column leaves (only a start can be: nothing below adds beyond k)
    while (nact > kmax) {
      double gb = HUGE_VAL;
      int ib = -1;
      for (int i = 0; i < p; ++i) {
        if (beta[i] == 0.0) continue;
        const double g = coord(r[(size_t)i] + d[(size_t)i] * beta[i], d[(size_t)i]).gain;
        if (g < gb) {  // (ties: the lowest i)
          gb = g;
          ib = i;
        }
      }
      if (ib < 0) break;
      const double bi = beta[ib];
      beta[ib] = 0.0;
      axpy(ib, bi);
      --nact;
      ++R.drops;
    }
  }
  for (;;) {
    // ---- 1. the descent to its fixed point (the cardinality rule: on the support alone, no threshold, b == 0 leaves) ---------
    for (int sw = 0;; ++sw) {
      if (sw == L0_CD_SWEEPS) {
        R.status |= L0_LS_SWEEPS_OUT;
        break;
      }
      bool moved = false;
      double maxd = 0.0;
      for (int j = 0; j < p; ++j) {
        const double dj = d[(size_t)j];
        if (CARD ? beta[j] == 0.0 : !(dj > 0.0)) continue;
        const L0LsCoord co = coord(r[(size_t)j] + dj * beta[j], dj);
        const double nb = CARD ? co.b : l0_ls_threshold(co, alpha);
        if (nb == beta[j]) continue;
        const double delta = nb - beta[j];
        moved = moved || ((nb != 0.0) != (beta[j] != 0.0));  // (on the support alone: only a column that leaves)
        if (CARD && nb == 0.0) {
          --nact;
          ++R.drops;
        }
        maxd = std::max(maxd, std::fabs(delta) * std::sqrt(dj));
        beta[j] = nb;
        axpy(j, -delta);
      }
      ++R.sweeps;
      if (!moved && maxd <= tol) break;
    }
    if (CARD) {
      // ---- grow: below k, the outside column with the largest gain enters -- if it would move by more than the descent's own
      // stopping tolerance -- and the descent runs again
      if (R.status) break;
      if (nact < kmax) {
        double gb = -1.0, bb = 0.0;
        int jb = -1;
        for (int j = 0; j < p; ++j) {
          if (beta[j] != 0.0 || !(d[(size_t)j] > 0.0)) continue;
          const L0LsCoord co = coord(r[(size_t)j], d[(size_t)j]);
          if (co.gain > gb) {  // (ties: the lowest j)
            gb = co.gain;
            bb = co.b;
            jb = j;
          }
        }
        if (jb >= 0 && std::fabs(bb) * std::sqrt(d[(size_t)jb]) > tol) {
          beta[jb] = bb;
          axpy(jb, -bb);
          ++nact;
          ++R.grows;
          continue;
        }
      }
    }
    if (!swaps || R.status) break;
    // ---- 2. the swap scan: the first i of the support that a column outside replaces with a gain (the cardinality rule: alpha = 0)
    bool swapped = false;
    for (int i = 0; i < p && !swapped; ++i) {
      const double bi = beta[i];
      if (bi == 0.0) continue;
      const double* row = G + (size_t)i * ld;
      const double gi = coord(r[(size_t)i] + d[(size_t)i] * bi, d[(size_t)i]).gain;
      double gb = -1.0, bb = 0.0;
      int jb = -1;
      for (int j = 0; j < p; ++j) {
        if (beta[j] != 0.0 || !(d[(size_t)j] > 0.0)) continue;
        const L0LsCoord co = coord(r[(size_t)j] + row[j] * bi, d[(size_t)j]);
        if (co.gain > gb) {  // (ties: the lowest j)
          gb = co.gain;
          bb = co.b;
          jb = j;
        }
      }
      if (jb < 0 || !l0_ls_swap_better(gb, gi, alpha)) continue;
      beta[i] = 0.0;
      axpy(i, bi);
      beta[jb] = bb;
      axpy(jb, -bb);
      ++R.swaps;
      swapped = true;
    }
    if (!swapped) break;
    if (R.swaps == L0_LS_SWAPS) {
      R.status |= L0_LS_SWAPS_OUT;
      break;
    }
  }
  // F = 1/2 beta^T H beta - c^T beta + alpha nnz with H beta = c - r (the cardinality rule: no alpha term is added)
  double acc = 0.0;
  for (int j = 0; j < p; ++j) {
    acc += beta[j] * (c[j] + r[(size_t)j]);
    R.nnz += beta[j] != 0.0;
  }
  R.F = CARD ? -0.5 * acc : -0.5 * acc + alpha * (double)R.nnz;
  if constexpr (L1) {  // + lam ||beta||_1
    double l1 = 0.0;
    for (int j = 0; j < p; ++j) l1 += std::fabs(beta[j]);
    R.F = -0.5 * acc + lam * l1 + alpha * (double)R.nnz;
  }
  return R;
}

// The winner's support re-solved exactly inside the box (what l0_boxed(..., polish = true) does for the exact search): the
// descent of l0_boxed from beta, its face solve where the box binds, and where it does not the Cholesky solve of the whole
// support, taken when the factor exists under the pivot rule and the point is inside the box.  beta: [p] in, out (the support
// is kept: zeros stay zero).  Returns 1/2 beta^T H beta - c^T beta, without the alpha term.
// (l0_ls_polish_on: the same on a given column list, whose zeros are free to move -- the grouped search polishes on every column
// of the groups in cl(S), "local groups" below)
inline double l0_ls_polish_on(const double* G, size_t ld, const double* c, double eta, double big_M, const std::vector<int>& cols, double* beta);
inline double l0_ls_polish(const double* G, size_t ld, const double* c, int p, double eta, double big_M, double* beta) {
  std::vector<int> cols;
  for (int j = 0; j < p; ++j)
    if (beta[j] != 0.0) cols.push_back(j);
  return l0_ls_polish_on(G, ld, c, eta, big_M, cols, beta);
}
inline double l0_ls_polish_on(const double* G, size_t ld, const double* c, double eta, double big_M, const std::vector<int>& cols, double* beta) {
  const int m = (int)cols.size();
  if (m == 0) return 0.0;
  std::vector<double> Hs((size_t)m * m), cs((size_t)m), b((size_t)m);
  std::vector<int> id((size_t)m);
  for (int a = 0; a < m; ++a) {
    id[(size_t)a] = a;
    cs[(size_t)a] = c[cols[(size_t)a]];
    b[(size_t)a] = beta[cols[(size_t)a]];
    for (int k = 0; k < m; ++k) Hs[(size_t)a * m + k] = G[(size_t)cols[(size_t)a] * ld + cols[(size_t)k]] + (a == k ? 2.0 * eta : 0.0);
  }
  double val = l0_boxed(Hs.data(), cs.data(), m, id.data(), m, big_M, true, b.data());
  bool all_free = true;
  for (int a = 0; a < m; ++a) all_free = all_free && std::fabs(b[(size_t)a]) < big_M;
  if (all_free) {
    std::vector<double> M = Hs, x = cs;
    if (l0_dense_chol(M, m)) {
      l0_dense_fwd(M, m, x.data());
      l0_dense_bwd(M, m, x.data());
      bool inside = true;
      for (int a = 0; a < m; ++a) inside = inside && std::fabs(x[(size_t)a]) <= big_M && x[(size_t)a] != 0.0;
      if (inside) {
        b = x;
        val = 0.0;
        for (int a = 0; a < m; ++a) {
          double t = 0.0;
          for (int k = 0; k < m; ++k) t += Hs[(size_t)a * m + k] * b[(size_t)k];
          val += b[(size_t)a] * (0.5 * t - cs[(size_t)a]);
        }
      }
    }
  }
  for (int a = 0; a < m; ++a) beta[cols[(size_t)a]] = b[(size_t)a];
  return val;
}

// What slm_solve_l0_local refuses before anything is launched, in this order (0: nothing); *which: the offending index.
enum L0LsRefusal { L0_LS_OK = 0, L0_LS_NULL, L0_LS_CELLS, L0_LS_STARTS, L0_LS_PROBLEMS, L0_LS_BIG_M, L0_LS_ALPHA, L0_LS_ETA, L0_LS_WIDTH,
                   L0_LS_START_BOX };
inline L0LsRefusal l0_ls_check(long long n_cells, const double* alphas, const double* etas, double big_M, long long n_starts,
                               const double* starts, long long p, long long* which = nullptr) {
  if (!alphas || !etas) return L0_LS_NULL;
  if (n_cells < 1) return L0_LS_CELLS;
  if (n_starts < 1) return L0_LS_STARTS;
  if (n_cells > L0_LS_MAX_PROBLEMS || n_starts > L0_LS_MAX_PROBLEMS || n_cells * n_starts > L0_LS_MAX_PROBLEMS) return L0_LS_PROBLEMS;
  if (!(big_M >= 0.0)) return L0_LS_BIG_M;
  for (long long e = 0; e < n_cells; ++e) {
    if (which) *which = e;
    if (!(alphas[e] >= 0.0) || !std::isfinite(alphas[e])) return L0_LS_ALPHA;
    if (!(etas[e] >= 0.0) || !std::isfinite(etas[e])) return L0_LS_ETA;
  }
  if (p > L0_LS_PMAX) return L0_LS_WIDTH;
  for (long long e = 0; starts && e < n_cells * n_starts * p; ++e)
    if (!(std::fabs(starts[e]) <= big_M)) {  // (a NaN fails too)
      if (which) *which = e;
      return L0_LS_START_BOX;
    }
  return L0_LS_OK;
}

// ---- local search over row sets (slm_solve_l0_local_folds; tests/l0_local_folds_host_test.cpp) ---------------------------------
//
// The same problems on `count` row sets of one dataset -- a cross-validation's training rows, then all rows -- in one launch.
// Problem q = (r * n_cells + e) * n_starts + s is row set r, cell e, start s; l0_lsf_split is the inverse.
constexpr int l0_lsf_index(int r, int e, int s, int n_cells, int n_starts) { return (r * n_cells + e) * n_starts + s; }
struct L0LsfProblem {
  int r, e, s;
};
constexpr L0LsfProblem l0_lsf_split(int q, int n_cells, int n_starts) {
  return L0LsfProblem{q / n_starts / n_cells, q / n_starts % n_cells, q % n_starts};
}

// What slm_solve_l0_local_folds refuses before a device is touched, in this order.  L0_LSF_LS: what slm_solve_l0_local
// refuses too -- `ls` says which; its limit on the problems is reported as L0_LSF_PRODUCT, the cap on all three factors.
// which: the offending index (a cell, a row of row set `row_set`, an entry of starts).
enum L0LsfKind { L0_LSF_OK = 0, L0_LSF_COUNT, L0_LSF_NULL, L0_LSF_LS, L0_LSF_PRODUCT, L0_LSF_INTERCEPT, L0_LSF_WEIGHT };
struct L0LsfRefusal {
  L0LsfKind kind = L0_LSF_OK;
  L0LsRefusal ls = L0_LS_OK;
  long long which = 0;
  int row_set = 0;
};
// p: the dataset's columns, the ones column included when `intercept`; last_alone: that column is last and alone in its group;
// n: the rows (the length of every given row_weights[r]).
inline L0LsfRefusal l0_lsf_check(long long count, const double* const* row_weights, const long long* n_effs, long long n, bool intercept,
                                 bool last_alone, long long n_cells, const double* alphas, const double* etas, double big_M,
                                 long long n_starts, const double* starts, long long p) {
  L0LsfRefusal R;
  auto refuse = [&](L0LsfKind kind, L0LsRefusal ls = L0_LS_OK) {
    R.kind = kind;
    R.ls = ls;
    return R;
  };
  if (count < 1 || count > L0_LS_ROW_SETS) return refuse(L0_LSF_COUNT);  // (first, as in the batch entry: no row set, no table of them)
  if (!row_weights || !n_effs || !alphas || !etas) return refuse(L0_LSF_NULL);
  const long long ps = p - (intercept ? 1 : 0);
  // (the product where l0_ls_check has its own of two factors: behind n_cells and n_starts, before big_M and the cells)
  if (n_cells >= 1 && n_starts >= 1 &&
      (n_cells > L0_LS_MAX_PROBLEMS || n_starts > L0_LS_MAX_PROBLEMS || count * n_cells * n_starts > L0_LS_MAX_PROBLEMS))
    return refuse(L0_LSF_PRODUCT);
  const L0LsRefusal ls = l0_ls_check(n_cells, alphas, etas, big_M, n_starts, nullptr, 0, &R.which);  // (the width and the box: below)
  if (ls != L0_LS_OK) return refuse(L0_LSF_LS, ls);
  R.which = 0;
  if (ps > L0_LS_PMAX) return refuse(L0_LSF_LS, L0_LS_WIDTH);
  if (intercept && (p < 1 || !last_alone)) return refuse(L0_LSF_INTERCEPT);
  for (int r = 0; r < (int)count; ++r)
    for (long long i = 0; i < n && row_weights[r]; ++i)
      if (!(row_weights[r][i] >= 0.0) || !std::isfinite(row_weights[r][i])) {
        R.row_set = r;
        R.which = i;
        return refuse(L0_LSF_WEIGHT);
      }
  for (long long e = 0; starts && e < count * n_cells * n_starts * ps; ++e)
    if (!(std::fabs(starts[e]) <= big_M)) {  // (a NaN fails too)
      R.which = e;
      return refuse(L0_LSF_LS, L0_LS_START_BOX);
    }
  return R;
}

// ---- local subsets: the cardinality form (slm_solve_l0_local_subsets; tests/l0_local_subsets_host_test.cpp) -------------------
//
// For a cell (k, eta), H = G + 2 eta I:   minimise Q(beta) = 1/2 beta^T H beta - c^T beta   over |beta_j| <= big_M, ||beta||_0 <= k
// (DESIGN 4d "Local subsets").  The state and the two decisions are the local search's; the rule, from a start of ANY support
// size inside the box:
//   1. Shrink: while nnz > k the support column with the smallest g_i = l0_ls_coord(r_i + d_i beta_i, d_i).gain leaves (ties:
//      the lowest index).
//   2. Descent on the support: j over the support cyclically, beta_j <- b, no threshold, no column enters; b == 0 leaves.  It
//      ends as the local search's descent does.
//   3. Grow: if nnz < k the outside column with the largest l0_ls_coord(r_j, d_j).gain (ties: the lowest j) enters at b_j when
//      |b_j| sqrt(d_j) > tol; then 2.
//   4. Swap scan, once 3 adds nothing: the local search's with alpha = 0; a swap goes to 2, none ends the problem.
// `drops` counts the columns that left in 1 or 2, `grows` those that entered in 3.  The rule without a device is
// l0_local_solve<true>, above: the penalised twin's body, with 1 before its loop and 3 between its descent and its swap scan,
// where the kernel has them.

// What slm_solve_l0_local_subsets refuses before a device is touched, in this order: a NULL sizes or etas; the first size < 1;
// the first eta that is negative or not finite; then everything l0_lsf_check refuses that is not about a cell's values (`lsf`:
// the row sets, the problem counts, big_M, the width, the intercept, the weights, the box of the starts).  which: the cell.
enum L0LcKind { L0_LC_OK = 0, L0_LC_NULL, L0_LC_SIZE, L0_LC_ETA, L0_LC_LSF };
struct L0LcRefusal {
  L0LcKind kind = L0_LC_OK;
  L0LsfRefusal lsf;
  long long which = 0;
};
inline L0LcRefusal l0_lc_check(long long count, const double* const* row_weights, const long long* n_effs, long long n, bool intercept,
                               bool last_alone, long long n_cells, const int* sizes, const double* etas, double big_M, long long n_starts,
                               const double* starts, long long p) {
  L0LcRefusal R;
  if (!sizes || !etas) {
    R.kind = L0_LC_NULL;
    return R;
  }
  for (long long e = 0; e < n_cells; ++e)
    if (sizes[e] < 1) {
      R.kind = L0_LC_SIZE;
      R.which = e;
      return R;
    }
  for (long long e = 0; e < n_cells; ++e)
    if (!(etas[e] >= 0.0) || !std::isfinite(etas[e])) {
      R.kind = L0_LC_ETA;
      R.which = e;
      return R;
    }
  // (the etas stand in for the alphas: they have just passed the test both get)
  R.lsf = l0_lsf_check(count, row_weights, n_effs, n, intercept, last_alone, n_cells, etas, etas, big_M, n_starts, starts, p);
  if (R.lsf.kind != L0_LSF_OK) R.kind = L0_LC_LSF;
  return R;
}

// ---- local search with an l1 term (slm_solve_l0_local_l1; l0_local_l1_kernel; tests/l1l0_local_host_test.cpp) -------------------
//
// A cell is (alpha, lam, eta); with H = G + 2 eta I,
//     F(beta) = 1/2 beta^T H beta - c^T beta + lam ||beta||_1 + alpha ||beta||_0   over |beta_j| <= big_M
// (eta = 0: the reference's L1L0 objective over 2n, singleton groups; DESIGN 4d "Local search with an l1 term").  The rule is the
// local search's with ONE change, the coordinate (l0_ls_coord_l1, above): the descent keeps b iff gain > alpha, the swap scan
// compares the same gains with l0_ls_swap_better, F gains lam ||beta||_1.  lam = 0 takes the decisions of the local search.  The
// rule without a device is l0_local_solve<false, true>.  Nothing is proven.

// What slm_solve_l0_local_l1 refuses before a device is touched, in this order: a NULL alphas or l1s; the first l1s[e] that is
// negative or not finite; the first ridges[e] that is (ridges may be NULL: no ridge); then everything l0_lsf_check refuses, in
// its order (`lsf`).  which: the cell.
enum L0L1lKind { L0_L1L_OK = 0, L0_L1L_NULL, L0_L1L_L1, L0_L1L_RIDGE, L0_L1L_LSF };
struct L0L1lRefusal {
  L0L1lKind kind = L0_L1L_OK;
  L0LsfRefusal lsf;
  long long which = 0;
};
inline L0L1lRefusal l0_l1l_check(long long count, const double* const* row_weights, const long long* n_effs, long long n, bool intercept,
                                 bool last_alone, long long n_cells, const double* alphas, const double* l1s, const double* ridges,
                                 double big_M, long long n_starts, const double* starts, long long p) {
  L0L1lRefusal R;
  if (!alphas || !l1s) {
    R.kind = L0_L1L_NULL;
    return R;
  }
  for (long long e = 0; e < n_cells; ++e)
    if (!(l1s[e] >= 0.0) || !std::isfinite(l1s[e])) {
      R.kind = L0_L1L_L1;
      R.which = e;
      return R;
    }
  for (long long e = 0; ridges && e < n_cells; ++e)
    if (!(ridges[e] >= 0.0) || !std::isfinite(ridges[e])) {
      R.kind = L0_L1L_RIDGE;
      R.which = e;
      return R;
    }
  // (no ridges: l0_lsf_check gets the zeros they stand for -- as many as it reads, which is none beyond the problem cap)
  const std::vector<double> none(ridges || n_cells < 1 || n_cells > L0_LS_MAX_PROBLEMS ? 1 : (size_t)n_cells, 0.0);
  R.lsf = l0_lsf_check(count, row_weights, n_effs, n, intercept, last_alone, n_cells, alphas, ridges ? ridges : none.data(), big_M, n_starts,
                       starts, p);
  if (R.lsf.kind != L0_LSF_OK) R.kind = L0_L1L_LSF;
  return R;
}

// The polish of a winner, on the rows of its support alone (as l0_ls_polish): the soft-threshold descent on the support to its
// last digit (l0_l1_descent), then the exact sign-face solve of l0_l1_polish -- H_FF x = c_F - lam sign(b_F) - H_FB b_B, taken
// only when every sign and the box hold.  A coefficient that comes to zero goes back as zero.  The point is kept only when its
// value is not above the incoming point's, so the polish never raises F (the non-zeros can only get fewer).  beta: [p] in, out.
// Returns 1/2 beta^T H beta - c^T beta + lam ||beta||_1 of what goes back, without the alpha term.
inline double l0_l1l_polish(const double* G, size_t ld, const double* c, int p, double eta, double lam, double big_M, double* beta) {
  std::vector<int> cols;
  for (int j = 0; j < p; ++j)
    if (beta[j] != 0.0) cols.push_back(j);
  const int m = (int)cols.size();
  if (m == 0) return 0.0;
  std::vector<double> Hs((size_t)m * m), cs((size_t)m), b((size_t)m), b0((size_t)m);
  std::vector<int> id((size_t)m);
  for (int a = 0; a < m; ++a) {
    id[(size_t)a] = a;
    cs[(size_t)a] = c[cols[(size_t)a]];
    b0[(size_t)a] = b[(size_t)a] = beta[cols[(size_t)a]];
    for (int k = 0; k < m; ++k) Hs[(size_t)a * m + k] = G[(size_t)cols[(size_t)a] * ld + cols[(size_t)k]] + (a == k ? 2.0 * eta : 0.0);
  }
  const double v0 = l0_l1_value(Hs.data(), cs.data(), m, id.data(), m, lam, b0.data());
  l0_l1_descent(Hs.data(), cs.data(), m, id.data(), m, lam, big_M, b.data());
  double val = l0_l1_polish(Hs.data(), cs.data(), m, id.data(), m, lam, big_M, b.data());
  if (!(val <= v0)) {
    b = b0;
    val = v0;
  }
  for (int a = 0; a < m; ++a) beta[cols[(size_t)a]] = b[(size_t)a];
  return val;
}

// l0_eliminate_last at a leading dimension, in two parts (the note on cancellation above it applies unchanged).
// The vectors and scalars, from the ones column g1 [ps] (row or column `last` of G: symmetric), G11 and c [ps + 1]:
//     c' = c - g1 c1 / G11,  yy' = yy - c1^2 / G11,  xmean = g1 / G11,  ymean = c1 / G11.     false: G11 is not positive.
inline bool l0_eliminate_vectors(const double* g1, double g11, const double* c, int ps, double yy, double* cs, double* yys, double* xmean,
                                 double* ymean) {
  const double c1 = c[ps];
  if (!(g11 > 0.0) || !std::isfinite(g11)) return false;
  for (int i = 0; i < ps; ++i) {
    xmean[i] = g1[i] / g11;
    cs[i] = c[i] - g1[i] * c1 / g11;
  }
  *ymean = c1 / g11;
  *yys = yy - c1 * c1 / g11;
  return true;
}
// In: G [p][ld] with the ones column LAST, c [p].  Out: Gs [(p - 1)][lds] (the padding of a row is left alone), cs, xmean
// [p - 1].  The device's l0_eliminate_kernel writes the same Gs.
inline bool l0_eliminate_last_ld(const double* G, size_t ld, const double* c, int p, double yy, double* Gs, size_t lds, double* cs,
                                 double* yys, double* xmean, double* ymean) {
  const int q = p - 1;
  std::vector<double> g1((size_t)q);
  for (int i = 0; i < q; ++i) g1[(size_t)i] = G[(size_t)i * ld + q];
  const double g11 = G[(size_t)q * ld + q];
  if (!l0_eliminate_vectors(g1.data(), g11, c, q, yy, cs, yys, xmean, ymean)) return false;
  for (int i = 0; i < q; ++i)
    for (int j = 0; j < q; ++j) Gs[(size_t)i * lds + j] = G[(size_t)i * ld + j] - g1[(size_t)i] * g1[(size_t)j] / g11;
  return true;
}

// ---- local groups: the local search with groups and a hierarchy (slm_solve_l0_local_groups; csrc/l0_local_group_kernels.hpp;
// tests/l0_local_groups_host_test.cpp) -----------------------------------------------------------------------------------------
//
// For a cell (alpha, eta), H = G + 2 eta I:
//     F(beta) = 1/2 beta^T H beta - c^T beta + alpha |cl(S(beta))|   over |beta_j| <= big_M,
// S(beta) the groups that hold a non-zero coefficient, cl its closure under the hierarchy (S and every group its members need,
// transitively): slm_solve_l0's objective with max_groups = n_groups and T = I.  Nothing is proven (DESIGN 4d "Local search with
// groups").  Groups are CONTIGUOUS and ASCENDING in column order: group g is the columns gstart[g] .. gstart[g + 1] - 1.  The
// hierarchy is the CLOSED list need*(g) per group in CSR form (l0_lg_close; g itself is not in it, so cycles are legal).
//
// The state: beta, r = c - H beta, d = diag H as for the local search; per group nz_g (its non-zero coefficients) and held_g (the
// groups h != g with nz_h > 0 that need g); z_g = (nz_g > 0 or held_g > 0) says whether g is in cl(S).  The PRICE of a group
// that is empty -- or of a non-empty one as if it had just been emptied -- is what |cl(S)| changes by when it enters (leaves):
//     m_g = [held_g == 0] (1 + #{h in need*(g): nz_h == 0 and held_h == 0 without g's own hold}).
//   1. Group descent, g = 0 .. n_groups - 1 cyclically.  A group with z_g = 1 gets a step; an inactive one only when it passes
//      the screen C_g = sum_{j in g, d_j > 0} gain(r_j, d_j) > alpha m_g / L0_LG_SCREEN.  The step: up to L0_LG_INNER passes of
//      beta_j <- b_j over the group's columns in ascending order, no threshold (a column with d_j <= 1e-12 max d stays 0), ended by
//      a pass whose max |delta| sqrt(d) <= tol; then the group's value v_g = 1/2 beta_g^T (r_g + r'_g) with
//      r' = r + sum_{j in g} H[:, j] beta_j (exact for any beta_g); the group is kept iff v_g > alpha m_g (strictly), else
//      beta_g <- 0 and r <- r'.  A sweep ends the descent when no group entered or left and the kept steps' max |delta| sqrt(d)
//      <= tol; L0_CD_SWEEPS sweeps end it unconverged.
//   2. Group swap scan (unless swaps == 0): i ascending over the groups with nz_i > 0 and held_i == 0.  i is removed (v_i, m_i,
//      r'); the candidate j is the empty group other than i with the largest C_j(r') - alpha m_j (prices in the state without i;
//      ties: the lowest j); j is fitted from zero by the inner passes (v_j); the swap is accepted iff
//      v_j - alpha m_j > v_i - alpha m_i + L0_LS_SWAP_TOL max(|v_i|, alpha) and the rule returns to 1; else beta and r are
//      restored from saved copies and the scan goes on.  No swap ends the problem; L0_LS_SWAPS accepted swaps end it unconverged.
// A start may have any support, closed or not; F always counts |cl(S)|.  Every accepted move lowers F.  With singleton groups
// and no hierarchy this is the local search's rule: v_g is the coordinate's gain, m_g = 1, the screen lets through every column
// the threshold would.
constexpr double L0_LG_SCREEN = 4.0;  // A HEURISTIC: the gain of a block has no bound in terms of its coordinates' gains at the
                                      // current r (two columns that cancel each other's correlation with r can gain together what
                                      // neither shows alone), so a group below the screen can be one that would have paid
constexpr int L0_LG_INNER = 8;        // passes over a group's columns in one step
constexpr int L0_LG_STATS = 6;        // ints per problem: sweeps, swaps, status word, |cl(S)|, non-zero columns, group trials

// need*(g) for every group from the direct lists (CSR: need_ptr [ng + 1], need_idx; NULL: no hierarchy): everything reachable
// from g, without g itself, ascending.  The indices must lie in 0 .. ng - 1 (l0_lg_check).
inline void l0_lg_close(int ng, const int* need_ptr, const int* need_idx, std::vector<int>& cptr, std::vector<int>& cidx) {
  cptr.assign((size_t)ng + 1, 0);
  cidx.clear();
  if (!need_ptr) return;
  std::vector<char> seen((size_t)ng);
  std::vector<int> stack;
  for (int g = 0; g < ng; ++g) {
    std::fill(seen.begin(), seen.end(), 0);
    stack.assign(1, g);
    while (!stack.empty()) {
      const int h = stack.back();
      stack.pop_back();
      for (int k = need_ptr[h]; k < need_ptr[h + 1]; ++k) {
        const int t = need_idx[k];
        if (seen[(size_t)t]) continue;
        seen[(size_t)t] = 1;
        stack.push_back(t);
      }
    }
    for (int h = 0; h < ng; ++h)
      if (seen[(size_t)h] && h != g) cidx.push_back(h);
    cptr[(size_t)g + 1] = (int)cidx.size();
  }
}

// cl(S) of a coefficient vector: in[g] = 1 where group g holds a non-zero or is needed by one that does.  Returns |cl(S)|.
inline int l0_lg_closure(const double* beta, int ng, const int* gstart, const int* cptr, const int* cidx, int* in) {
  for (int g = 0; g < ng; ++g) in[g] = 0;
  for (int g = 0; g < ng; ++g) {
    bool any = false;
    for (int j = gstart[g]; j < gstart[g + 1]; ++j) any = any || beta[j] != 0.0;
    if (!any) continue;
    in[g] = 1;
    for (int k = cptr[g]; k < cptr[g + 1]; ++k) in[cidx[k]] = 1;
  }
  int count = 0;
  for (int g = 0; g < ng; ++g) count += in[g];
  return count;
}

struct L0LgResult {
  double F = 0.0;  // the objective at the returned beta, with alpha |cl(S)|
  int sweeps = 0, swaps = 0, status = 0, closed = 0, nnz = 0, trials = 0;  // (trials: fits of a group that was not in cl(S), or of a swap's candidate)
  long long changes = 0;  // columns of H applied to r or r' after the start: what the time goes to
};

// The rule on one problem: the kernel's twin, l0_local_group_kernel without a device.  G: [p][ld] (symmetric), c: [p]; 2 eta goes
// on the diagonal here.  gstart: [ng + 1]; cptr, cidx: the CLOSED lists (cptr may be NULL: no hierarchy).  start: [p] inside the
// box or NULL; beta: [p] out.
inline L0LgResult l0_lg_solve(const double* G, size_t ld, const double* c, int p, int ng, const int* gstart, const int* cptr, const int* cidx,
                              double alpha, double eta, double big_M, double yy, bool swaps, const double* start, double* beta) {
  L0LgResult R;
  std::vector<double> r(c, c + p), d((size_t)p), rp((size_t)p), sb((size_t)p), sr((size_t)p);
  std::vector<int> nz((size_t)ng, 0), held((size_t)ng, 0);
  const double eta2 = 2.0 * eta;
  double dmax = 0.0;
  for (int j = 0; j < p; ++j) {
    d[(size_t)j] = G[(size_t)j * ld + j] + eta2;
    dmax = std::max(dmax, d[(size_t)j]);
  }
  for (int j = 0; j < p; ++j) {
    if (!(d[(size_t)j] > L0_PIVOT * dmax)) d[(size_t)j] = 0.0;  // (0 marks a column that stays out)
    beta[j] = start && d[(size_t)j] > 0.0 ? start[j] : 0.0;
  }
  auto axpy = [&](std::vector<double>& x, int j, double w) {  // x += w H[:, j]
    const double* row = G + (size_t)j * ld;
    for (int k = 0; k < p; ++k) x[(size_t)k] += w * (k == j ? row[k] + eta2 : row[k]);
    ++R.changes;
  };
  for (int j = 0; j < p; ++j)
    if (beta[j] != 0.0) axpy(r, j, -beta[j]);
  R.changes = 0;  // (the start is not counted)
  const double tol = L0_CD_TOL * std::sqrt(yy);
  auto first = [&](int g) { return cptr ? cptr[g] : 0; };
  auto last = [&](int g) { return cptr ? cptr[g + 1] : 0; };
  auto count = [&](int g) {
    int n = 0;
    for (int j = gstart[g]; j < gstart[g + 1]; ++j) n += beta[j] != 0.0;
    return n;
  };
  auto hold = [&](int g, int by) {
    for (int k = first(g); k < last(g); ++k) held[(size_t)cidx[k]] += by;
  };
  auto price = [&](int g) {  // m_g: of an empty group, or of a non-empty one as if it had just been emptied
    if (held[(size_t)g] > 0) return 0;
    const int own = nz[(size_t)g] > 0 ? 1 : 0;  // (its own hold on the groups it needs)
    int m = 1;
    for (int k = first(g); k < last(g); ++k) m += nz[(size_t)cidx[k]] == 0 && held[(size_t)cidx[k]] == own;
    return m;
  };
  auto gains = [&](int g) {  // C_g, summed in ascending column order
    double C = 0.0;
    for (int j = gstart[g]; j < gstart[g + 1]; ++j) C += d[(size_t)j] > 0.0 ? l0_ls_coord(r[(size_t)j], d[(size_t)j], big_M).gain : 0.0;
    return C;
  };
  auto fit = [&](int g, bool& changed) {  // the inner passes; the largest |delta| sqrt(d) of any of them
    double worst = 0.0;
    for (int pass = 0; pass < L0_LG_INNER; ++pass) {
      double mp = 0.0;
      for (int j = gstart[g]; j < gstart[g + 1]; ++j) {
        const double dj = d[(size_t)j];
        if (!(dj > 0.0)) continue;
        const double b = l0_ls_coord(r[(size_t)j] + dj * beta[j], dj, big_M).b, delta = b - beta[j];
        if (delta == 0.0) continue;
        beta[j] = b;
        axpy(r, j, -delta);
        changed = true;
        mp = std::max(mp, std::fabs(delta) * std::sqrt(dj));
      }
      worst = std::max(worst, mp);
      if (mp <= tol) break;
    }
    return worst;
  };
  auto value = [&](int g) {  // v_g; rp <- r'
    rp = r;
    for (int j = gstart[g]; j < gstart[g + 1]; ++j)
      if (beta[j] != 0.0) axpy(rp, j, beta[j]);
    double v = 0.0;
    for (int j = gstart[g]; j < gstart[g + 1]; ++j) v += beta[j] * (r[(size_t)j] + rp[(size_t)j]);
    return 0.5 * v;
  };
  auto empty = [&](int g) {  // beta_g <- 0, r <- r'
    for (int j = gstart[g]; j < gstart[g + 1]; ++j) beta[j] = 0.0;
    r = rp;
  };
  for (int g = 0; g < ng; ++g) nz[(size_t)g] = count(g);
  for (int g = 0; g < ng; ++g)
    if (nz[(size_t)g] > 0) hold(g, 1);
  for (;;) {
    // ---- 1. the group descent to its fixed point ------------------------------------------------------------------------------
    for (int sw = 0;; ++sw) {
      if (sw == L0_CD_SWEEPS) {
        R.status |= L0_LS_SWEEPS_OUT;
        break;
      }
      bool moved = false;
      double maxd = 0.0;
      for (int g = 0; g < ng; ++g) {
        const bool was = nz[(size_t)g] > 0;
        const int m = price(g);
        if (!was && held[(size_t)g] == 0) {
          if (!(gains(g) > alpha * (double)m / L0_LG_SCREEN)) continue;
          ++R.trials;
        }
        bool changed = false;
        const double w = fit(g, changed);
        const double v = value(g);
        if (v > alpha * (double)m) {
          const int now = count(g);
          if ((now > 0) != was) {
            hold(g, now > 0 ? 1 : -1);
            moved = true;
          }
          nz[(size_t)g] = now;
          maxd = std::max(maxd, w);
        } else {
          empty(g);
          nz[(size_t)g] = 0;
          if (was) {
            hold(g, -1);
            moved = true;
          }
        }
      }
      ++R.sweeps;
      if (!moved && maxd <= tol) break;
    }
    if (!swaps || R.status) break;
    // ---- 2. the group swap scan: the first i that an empty group replaces with a gain --------------------------------------------
    bool swapped = false;
    for (int i = 0; i < ng && !swapped; ++i) {
      if (nz[(size_t)i] == 0 || held[(size_t)i] > 0) continue;
      std::copy(beta, beta + p, sb.begin());
      sr = r;
      const int nzi = nz[(size_t)i], mi = price(i);
      const double vi = value(i);
      empty(i);
      nz[(size_t)i] = 0;
      hold(i, -1);
      int jb = -1;
      double best = -HUGE_VAL;
      for (int j = 0; j < ng; ++j) {
        if (j == i || nz[(size_t)j] > 0) continue;
        const double score = gains(j) - alpha * (double)price(j);
        if (score > best) {  // (ties: the lowest j)
          best = score;
          jb = j;
        }
      }
      bool ok = false;
      if (jb >= 0) {
        const int mj = price(jb);
        bool changed = false;
        ++R.trials;
        fit(jb, changed);
        const double vj = value(jb), a = std::fabs(vi);
        ok = vj - alpha * (double)mj > vi - alpha * (double)mi + L0_LS_SWAP_TOL * (a > alpha ? a : alpha);
      }
      if (ok) {
        nz[(size_t)jb] = count(jb);
        if (nz[(size_t)jb] > 0) hold(jb, 1);
        ++R.swaps;
        swapped = true;
      } else {
        std::copy(sb.begin(), sb.end(), beta);
        r = sr;
        nz[(size_t)i] = nzi;
        hold(i, 1);
      }
    }
    if (!swapped) break;
    if (R.swaps == L0_LS_SWAPS) {
      R.status |= L0_LS_SWAPS_OUT;
      break;
    }
  }
  double acc = 0.0;
  for (int j = 0; j < p; ++j) {
    acc += beta[j] * (c[j] + r[(size_t)j]);
    R.nnz += beta[j] != 0.0;
  }
  for (int g = 0; g < ng; ++g) R.closed += nz[(size_t)g] > 0 || held[(size_t)g] > 0;
  R.F = -0.5 * acc + alpha * (double)R.closed;
  return R;
}

// What slm_solve_l0_local_groups refuses before a device is touched, in this order: everything l0_lsf_check refuses (`lsf`);
// a group index that is not 0 at column 0 or does not rise by 0 or 1 from a column to the next (groups not contiguous or not
// ascending: the caller must order the columns; which: the column); a need_ptr that does not start at 0 or falls (which: the
// group); a need_idx outside the search groups, or a NULL need_idx under a non-empty need_ptr (which: the entry); a row-sharded
// dataset.  gid: [p] the dataset's group index, or NULL for singleton groups; *n_search: the groups of the searched columns.
enum L0LgKind { L0_LG_OK = 0, L0_LG_LSF, L0_LG_ORDER, L0_LG_NEED_PTR, L0_LG_NEED_IDX, L0_LG_SHARDED };
struct L0LgRefusal {
  L0LgKind kind = L0_LG_OK;
  L0LsfRefusal lsf;
  long long which = 0;
};
inline L0LgRefusal l0_lg_check(long long count, const double* const* row_weights, const long long* n_effs, long long n, bool intercept,
                               bool last_alone, long long n_cells, const double* alphas, const double* etas, double big_M,
                               long long n_starts, const double* starts, long long p, const int* gid, const int* need_ptr,
                               const int* need_idx, bool sharded, int* n_search = nullptr) {
  L0LgRefusal R;
  auto refuse = [&](L0LgKind kind, long long which) {
    R.kind = kind;
    R.which = which;
    return R;
  };
  R.lsf = l0_lsf_check(count, row_weights, n_effs, n, intercept, last_alone, n_cells, alphas, etas, big_M, n_starts, starts, p);
  if (R.lsf.kind != L0_LSF_OK) return refuse(L0_LG_LSF, R.lsf.which);
  const long long ps = p - (intercept ? 1 : 0);
  for (long long j = 0; gid && j < p; ++j) {
    const int step = j == 0 ? gid[0] + 1 : gid[j] - gid[j - 1];
    if (step != 0 && step != 1) return refuse(L0_LG_ORDER, j);
    if (j == 0 && step != 1) return refuse(L0_LG_ORDER, j);
  }
  const long long ng = ps < 1 ? 0 : (gid ? (long long)gid[ps - 1] + 1 : ps);
  if (n_search) *n_search = (int)ng;
  if (need_ptr) {
    if (need_ptr[0] != 0) return refuse(L0_LG_NEED_PTR, 0);
    for (long long g = 0; g < ng; ++g)
      if (need_ptr[g + 1] < need_ptr[g]) return refuse(L0_LG_NEED_PTR, g + 1);
    if (need_ptr[ng] > 0 && !need_idx) return refuse(L0_LG_NEED_IDX, 0);
    for (long long k = 0; k < need_ptr[ng]; ++k)
      if (need_idx[k] < 0 || need_idx[k] >= ng) return refuse(L0_LG_NEED_IDX, k);
  }
  if (sharded) return refuse(L0_LG_SHARDED, 0);
  return R;
}

// ---- local bound (slm_solve_l0_local_bound; csrc/l0_local_bound_kernels.hpp; tests/l0_local_bound_host_test.cpp) ----------------
//
// The half the local search lacks: a PROVEN lower bound on the objective it minimises.  For a cell (alpha, eta) and the box
// |beta_j| <= M,  F(beta) = 1/2 beta^T (G + 2 eta I) beta - c^T beta + alpha ||beta||_0.  The indicator is relaxed by the
// perspective of the ridge term with the big-M link (z_j in [0, 1], |beta_j| <= M z_j, cost eta beta_j^2 / z_j + alpha z_j);
// minimising over z leaves a separable convex penalty phi.  With tau = sqrt(alpha / eta) (infinite at eta = 0):
//     M >= tau:  phi(b) = 2 sqrt(alpha eta) |b| on |b| <= tau,  eta b^2 + alpha on tau <= |b| <= M
//     M <  tau:  phi(b) = (eta M + alpha / M) |b| on |b| <= M
// and phi*(t) = max(0, h(t) - alpha) with h(t) = t^2 / (4 eta) on |t| <= 2 eta M, else |t| M - eta M^2 (eta = 0: |t| M).  g(b) =
// 1/2 b^T G b - c^T b is convex, so by Fenchel duality, for EVERY vector u, with t = c - G u (the plain G: the ridge is in phi),
//     L(u) = -1/2 u^T G u - sum over ALL p columns of max(0, h(t_j) - alpha)   <=   min F.
// It is tightest at the minimiser of P(b) = g(b) + sum phi(b_j), where L = P; cyclic coordinate descent on P finds it
// (l0_lb_coord is the exact coordinate minimiser).  A column whose G_jj <= L0_PIVOT max G_kk keeps u_j = 0 and is still counted
// in the sum.  The bound is tight with a ridge or a real box and weak at eta = 0 under a loose M (DESIGN 4d "Local bound").
//
// The functions below hold every number kernel and twin compute, with contraction of a*b + c switched off where the compiler
// would decide it, so that both give the same bits on any host (one with fused multiply-adds too); the one contracted step is
// the rank-one update of t (l0_ls_axpy on the device, std::fma here).  Under clang -- the device pass and hipcc's host pass --
// L0_LB_STRICT at the head of a body switches contraction off for that body; under GCC, which has no such pragma inside a
// function, the whole section stands between push_options / optimize("fp-contract=off") / pop_options.  (The tests and tools
// that compile this header pass -ffp-contract=off as well.)
// l0_lb_coord, l0_lb_phi, l0_lb_conj, l0_lb_changed and l0_lb_closed are the ONE definition kernel and twin share: constexpr
// functions, which HIP-clang treats as __host__ __device__ without the words (as it does l0_ls_coord and l0_ls_coord_l1 above),
// so that a plain C++ compiler reads this header too.
#if defined(__clang__)
#define L0_LB_STRICT _Pragma("clang fp contract(off)")
#define L0_LB_INLINE __attribute__((always_inline))  // (a call left in the kernel would cost it its registers)
#else
#define L0_LB_STRICT
#define L0_LB_INLINE
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
constexpr int L0_LB_SWEEPS = 10000;       // sweeps of one cell where the caller names none
constexpr double L0_LB_GAP_DEFAULT = 1e-9;  // the default of the callers above the ABI: P - L <= gap_tol max(|P|, alpha) ends a cell
constexpr int L0_LB_MODE = 11;            // slm_point_info.mode of the entry

// what a cell's phi needs beside (alpha, eta, M): lam, its slope at zero, and tauc = min(tau, M), where its linear piece ends.
// Computed once per cell on the host (the one place with a square root) and handed to kernel and twin alike.  big_M > 0.
struct L0LbCell {
  double lam, tauc;
};
inline L0LbCell l0_lb_cell(double alpha, double eta, double big_M) {
  L0_LB_STRICT
  if (eta > 0.0) {
    const double tau = std::sqrt(alpha / eta);
    if (big_M >= tau) return L0LbCell{2.0 * std::sqrt(alpha * eta), tau};
    return L0LbCell{eta * big_M + alpha / big_M, big_M};
  }
  return L0LbCell{alpha / big_M, big_M};
}
// the coordinate step: the minimiser over |b| <= M of 1/2 a b^2 - s b + phi(b), a = G_jj > 0, s = t_j + a u_j
L0_LB_INLINE constexpr double l0_lb_coord(double s, double a, double eta, double lam, double tauc, double big_M) {
  L0_LB_STRICT
  const double as = s < 0.0 ? -s : s;
  const double b1 = as > lam ? (as - lam) / a : 0.0;
  if (b1 <= tauc) return s < 0.0 ? -b1 : b1;
  double b2 = as / (a + 2.0 * eta);
  b2 = b2 < tauc ? tauc : (b2 > big_M ? big_M : b2);
  return s < 0.0 ? -b2 : b2;
}
L0_LB_INLINE constexpr double l0_lb_phi(double b, double alpha, double eta, double lam, double tauc) {
  L0_LB_STRICT
  const double ab = b < 0.0 ? -b : b;
  return ab <= tauc ? lam * ab : eta * ab * ab + alpha;
}
// phi*(t) = max(0, h(t) - alpha)
L0_LB_INLINE constexpr double l0_lb_conj(double t, double alpha, double eta, double big_M) {
  L0_LB_STRICT
  const double at = t < 0.0 ? -t : t;
  double h = 0.0;
  if (eta > 0.0)
    h = at <= 2.0 * eta * big_M ? at * at / (4.0 * eta) : at * big_M - eta * big_M * big_M;
  else if (at > 0.0)
    h = at * big_M;
  const double v = h - alpha;
  return v > 0.0 ? v : 0.0;
}
// has the coordinate changed?  (A NaN -- non-finite data -- is no change: it must not keep a cell sweeping.)
L0_LB_INLINE constexpr bool l0_lb_changed(double nb, double old) { return nb < old || nb > old; }
// the stopping rule after a sweep
L0_LB_INLINE constexpr bool l0_lb_closed(double P, double L, double alpha, double gap_tol) {
  L0_LB_STRICT
  const double ap = P < 0.0 ? -P : P;
  return P - L <= gap_tol * (ap > alpha ? ap : alpha);
}

// The kernel's sum of one term per column, in its order: lane j & 63 adds its columns in ascending order from zero, then the
// wave's butterfly (l0_wave_sum: v += v[lane ^ off], off = 32 .. 1), which leaves the same bits in every lane.
inline double l0_lb_wave_sum(const double* lanes) {
  L0_LB_STRICT
  double v[64], w[64];
  for (int i = 0; i < 64; ++i) v[i] = lanes[i];
  for (int off = 32; off >= 1; off >>= 1) {
    for (int i = 0; i < 64; ++i) w[i] = v[i] + v[i ^ off];
    for (int i = 0; i < 64; ++i) v[i] = w[i];
  }
  return v[0];
}
// P(u) and L(u) from u and t = c - G u, with u^T G u = u^T (c - t):
//     P = -1/2 sum u_j (c_j + t_j) + sum phi(u_j),     L = -1/2 sum u_j (c_j - t_j) - sum phi*(t_j)
struct L0LbValues {
  double P, L;
};
inline L0LbValues l0_lb_values(const double* u, const double* t, const double* c, int p, double alpha, double eta, double big_M,
                               const L0LbCell& cell) {
  L0_LB_STRICT
  double qp[64] = {0.0}, ql[64] = {0.0}, sp[64] = {0.0}, sc[64] = {0.0};
  for (int j = 0; j < p; ++j) {
    const int l = j & 63;
    qp[l] += u[j] * (c[j] + t[j]);
    ql[l] += u[j] * (c[j] - t[j]);
    sp[l] += l0_lb_phi(u[j], alpha, eta, cell.lam, cell.tauc);
    sc[l] += l0_lb_conj(t[j], alpha, eta, big_M);
  }
  return L0LbValues{-0.5 * l0_lb_wave_sum(qp) + l0_lb_wave_sum(sp), -0.5 * l0_lb_wave_sum(ql) - l0_lb_wave_sum(sc)};
}

struct L0LbResult {
  double lower = 0.0;   // max(L(u), L(0)): the bound
  double primal = 0.0;  // P(u): the relaxation's value at u
  int sweeps = 0, status = 0;  // status: L0_LS_SWEEPS_OUT when the sweeps ran out before the gap closed
  long long changes = 0;       // columns of G applied to t in the sweeps: what the time goes to
};
// The kernel's twin without a device, change for change.  G: [p][ld] (row j is read for column j), c: [p], start: [p] or NULL
// (clipped into the box), u: [p] out.  big_M > 0; max_sweeps >= 1; gap_tol >= 0 (0: every sweep is run).
inline L0LbResult l0_bound_solve(const double* G, size_t ld, const double* c, int p, double alpha, double eta, double big_M,
                                 const double* start, int max_sweeps, double gap_tol, double* u) {
  L0_LB_STRICT
  L0LbResult R;
  const L0LbCell cell = l0_lb_cell(alpha, eta, big_M);
  std::vector<double> t(c, c + p), a((size_t)p);
  double amax = 0.0;
  for (int j = 0; j < p; ++j) {
    a[(size_t)j] = G[(size_t)j * ld + j];
    u[j] = 0.0;
    amax = std::fmax(amax, a[(size_t)j]);
  }
  for (int j = 0; j < p; ++j)
    if (!(a[(size_t)j] > L0_PIVOT * amax)) a[(size_t)j] = 0.0;  // a = 0 marks a column that keeps u_j = 0
  const double L0 = l0_lb_values(u, t.data(), c, p, alpha, eta, big_M, cell).L;
  auto axpy = [&](int j, double w) {  // t += w G[:, j]: the device's contracted multiply-add
    const double* row = G + (size_t)j * ld;
    for (int k = 0; k < p; ++k) t[(size_t)k] = std::fma(w, row[k], t[(size_t)k]);
  };
  auto build = [&]() {  // t = c - G u, column by column in ascending order
    for (int k = 0; k < p; ++k) t[(size_t)k] = c[k];
    for (int j = 0; j < p; ++j)
      if (u[j] != 0.0) axpy(j, -u[j]);
  };
  if (start)
    for (int j = 0; j < p; ++j)
      if (a[(size_t)j] > 0.0) u[j] = start[j] < -big_M ? -big_M : (start[j] > big_M ? big_M : start[j]);
  build();
  for (int sw = 0;; ++sw) {
    if (sw == max_sweeps) {
      R.status |= L0_LS_SWEEPS_OUT;
      break;
    }
    for (int j = 0; j < p; ++j) {
      const double aj = a[(size_t)j];
      if (!(aj > 0.0)) continue;
      const double nb = l0_lb_coord(t[(size_t)j] + aj * u[j], aj, eta, cell.lam, cell.tauc, big_M);
      if (!l0_lb_changed(nb, u[j])) continue;
      const double delta = nb - u[j];
      u[j] = nb;
      axpy(j, -delta);
      ++R.changes;
    }
    ++R.sweeps;
    const L0LbValues v = l0_lb_values(u, t.data(), c, p, alpha, eta, big_M, cell);
    if (l0_lb_closed(v.P, v.L, alpha, gap_tol)) break;
  }
  build();  // no running residual feeds the certificate
  const L0LbValues v = l0_lb_values(u, t.data(), c, p, alpha, eta, big_M, cell);
  R.lower = v.L > L0 ? v.L : L0;
  R.primal = v.P;
  return R;
}

#if !defined(__clang__)
#pragma GCC pop_options
#endif

// What slm_solve_l0_local_bound refuses before a device is touched, in this order (slm_solve_l0_local's where the checks
// coincide); which: the offending cell, or entry of starts.
enum L0LbRefusal { L0_LB_OK = 0, L0_LB_NULL, L0_LB_CELLS, L0_LB_PROBLEMS, L0_LB_BIG_M, L0_LB_ALPHA, L0_LB_ETA, L0_LB_GAP_TOL, L0_LB_WIDTH,
                   L0_LB_START, L0_LB_GROUPS, L0_LB_SHARDED };
inline L0LbRefusal l0_bound_check(long long n_cells, const double* alphas, const double* etas, double big_M, const double* starts,
                                  long long p, double gap_tol, bool singleton, bool sharded, long long* which = nullptr) {
  if (!alphas || !etas) return L0_LB_NULL;
  if (n_cells < 1) return L0_LB_CELLS;
  if (n_cells > L0_LS_MAX_PROBLEMS) return L0_LB_PROBLEMS;
  if (!(big_M >= 0.0)) return L0_LB_BIG_M;
  for (long long e = 0; e < n_cells; ++e) {
    if (which) *which = e;
    if (!(alphas[e] >= 0.0) || !std::isfinite(alphas[e])) return L0_LB_ALPHA;
    if (!(etas[e] >= 0.0) || !std::isfinite(etas[e])) return L0_LB_ETA;
  }
  if (!(gap_tol >= 0.0)) return L0_LB_GAP_TOL;
  if (p > L0_LS_PMAX) return L0_LB_WIDTH;
  for (long long e = 0; starts && e < n_cells * p; ++e)
    if (!std::isfinite(starts[e])) {
      if (which) *which = e;
      return L0_LB_START;
    }
  if (!singleton) return L0_LB_GROUPS;
  if (sharded) return L0_LB_SHARDED;
  return L0_LB_OK;
}

// ---- local proof (slm_solve_l0_local_nodes, slm_solve_l0_local_prove; csrc/l0_local_node_kernels.hpp; tests/l0_local_prove_host_test.cpp)
//
// Branch and bound on the local bound (the L0BnB scheme of Hazimeh, Mazumder and Saab).  A NODE gives every column one of
// three states: FREE, IN (the column pays alpha whether its coefficient is zero or not) or OUT (beta_j = 0).  The bound's
// relaxation on a node is the same separable convex problem with three kinds of coordinate: with t = c - G u, for EVERY u,
//     L_node(u) = -1/2 u^T G u - sum over FREE of max(0, h(t_j) - alpha) - sum over IN of (h(t_j) - alpha)
//              <=  min { F(beta) : |beta_j| <= M, beta_OUT = 0, IN columns pay alpha whether zero or not }
// (h: l0_lb_conj without its max).  g(beta) >= -1/2 u^T G u - t^T beta by convexity; the conjugate of eta b^2 + alpha on the box
// is h - alpha, that of the indicator of {0} is 0.  The coordinate step: FREE l0_lb_coord, IN clip(s / (a + 2 eta), +-M), OUT
// u_j = 0; a column that fails the pivot test keeps u_j = 0 in any state and its conjugate term is still counted.  Beside L and
// P_node(u) a node returns F(u) = 1/2 u^T (G + 2 eta I) u - c^T u + alpha nnz(u), an upper bound of the cell because u lies in
// the box.  The tree (l0_prove_tree) is device-free and templated on the callable that bounds a batch of nodes: the engine
// passes the launch of l0_local_node_kernel, the twin l0_node_solve -- one body, the same tree node for node.
#if !defined(__clang__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
constexpr int L0_ND_FREE = 0, L0_ND_IN = 1, L0_ND_OUT = 2;  // a column's state in a node
constexpr int L0_ND_WORDS = L0_LS_SLOTS;  // 64-bit words of a node's IN mask, and of its OUT mask: bit `lane` of word `slot`
constexpr int L0_ND_MAX_BATCH = 8192;     // nodes of one launch
constexpr int L0_ND_MODE = 12, L0_PV_MODE = 13;  // slm_point_info.mode of the two entries
constexpr int L0_PV_OPTIMAL = 0, L0_PV_NODE_LIMIT = 1;  // a cell's status

// a cell as kernel and twin take it: (alpha, eta, M) and l0_lb_cell's two numbers
struct L0NodeCell {
  double alpha, eta, big_M, lam, tauc;
};
inline L0NodeCell l0_node_cell(double alpha, double eta, double big_M) {
  const L0LbCell c = l0_lb_cell(alpha, eta, big_M);
  return L0NodeCell{alpha, eta, big_M, c.lam, c.tauc};
}
L0_LB_INLINE constexpr int l0_node_state(const unsigned long long* in_mask, const unsigned long long* out_mask, int j) {
  return (int)((in_mask[j >> 6] >> (j & 63)) & 1ull) | ((int)((out_mask[j >> 6] >> (j & 63)) & 1ull) << 1);
}
// h(t): the conjugate of eta b^2 on the box, l0_lb_conj's h in its own arithmetic
L0_LB_INLINE constexpr double l0_node_h(double t, double eta, double big_M) {
  L0_LB_STRICT
  const double at = t < 0.0 ? -t : t;
  double h = 0.0;
  if (eta > 0.0)
    h = at <= 2.0 * eta * big_M ? at * at / (4.0 * eta) : at * big_M - eta * big_M * big_M;
  else if (at > 0.0)
    h = at * big_M;
  return h;
}
// the coordinate step by state (a > 0: an OUT column and one that fails the pivot test never get here)
L0_LB_INLINE constexpr double l0_node_coord(double s, double a, double eta, double lam, double tauc, double big_M, int state) {
  L0_LB_STRICT
  if (state == L0_ND_FREE) return l0_lb_coord(s, a, eta, lam, tauc, big_M);
  if (state != L0_ND_IN) return 0.0;
  const double b = s / (a + 2.0 * eta);
  return b < -big_M ? -big_M : (b > big_M ? big_M : b);
}
// a column's term of P_node: FREE phi(b), IN eta b^2 + alpha (paid at zero too), OUT nothing
L0_LB_INLINE constexpr double l0_node_phi(double b, double alpha, double eta, double lam, double tauc, int state) {
  L0_LB_STRICT
  if (state == L0_ND_FREE) return l0_lb_phi(b, alpha, eta, lam, tauc);
  if (state != L0_ND_IN) return 0.0;
  return eta * b * b + alpha;
}
// a column's term of -L_node: FREE max(0, h - alpha), IN h - alpha, OUT nothing
L0_LB_INLINE constexpr double l0_node_conj(double t, double alpha, double eta, double big_M, int state) {
  L0_LB_STRICT
  if (state == L0_ND_FREE) return l0_lb_conj(t, alpha, eta, big_M);
  if (state != L0_ND_IN) return 0.0;
  return l0_node_h(t, eta, big_M) - alpha;
}
// P_node, L_node and F from the six sums over the columns (each a wave sum: l0_lb_wave_sum's order)
struct L0NodeValues {
  double P, L, F;
};
L0_LB_INLINE constexpr L0NodeValues l0_node_combine(double qp, double ql, double sp, double sc, double s2, double nz, double alpha, double eta) {
  L0_LB_STRICT
  const double half = -0.5 * qp;
  return L0NodeValues{half + sp, -0.5 * ql - sc, (half + eta * s2) + alpha * nz};
}
inline L0NodeValues l0_node_values(const double* u, const double* t, const double* c, int p, const L0NodeCell& cell, const unsigned char* state) {
  L0_LB_STRICT
  double qp[64] = {0.0}, ql[64] = {0.0}, sp[64] = {0.0}, sc[64] = {0.0}, s2[64] = {0.0}, nz[64] = {0.0};
  for (int j = 0; j < p; ++j) {
    const int l = j & 63;
    qp[l] += u[j] * (c[j] + t[j]);
    ql[l] += u[j] * (c[j] - t[j]);
    sp[l] += l0_node_phi(u[j], cell.alpha, cell.eta, cell.lam, cell.tauc, state[j]);
    sc[l] += l0_node_conj(t[j], cell.alpha, cell.eta, cell.big_M, state[j]);
    s2[l] += u[j] * u[j];
    nz[l] += u[j] != 0.0 ? 1.0 : 0.0;
  }
  return l0_node_combine(l0_lb_wave_sum(qp), l0_lb_wave_sum(ql), l0_lb_wave_sum(sp), l0_lb_wave_sum(sc), l0_lb_wave_sum(s2), l0_lb_wave_sum(nz),
                         cell.alpha, cell.eta);
}

struct L0NodeResult {
  double lower = 0.0;   // max(L_node(u), L_node(0)): a bound of the node
  double primal = 0.0;  // P_node(u)
  double upper = 0.0;   // F(u): an upper bound of the cell
  int sweeps = 0, status = 0;
  long long changes = 0;
};
// The node kernel's twin without a device, change for change: l0_bound_solve with three kinds of coordinate -- its stopping
// rule, its sums, its rebuilt certificate.  With both masks empty it returns l0_bound_solve's bits.  in_mask, out_mask:
// L0_ND_WORDS words each; start: [p] or NULL (clipped into the box; an OUT column starts at zero); u: [p] out.
inline L0NodeResult l0_node_solve(const double* G, size_t ld, const double* c, int p, const L0NodeCell& cell, const unsigned long long* in_mask,
                                  const unsigned long long* out_mask, const double* start, int max_sweeps, double gap_tol, double* u) {
  L0_LB_STRICT
  L0NodeResult R;
  const double big_M = cell.big_M;
  std::vector<double> t(c, c + p), a((size_t)p);
  std::vector<unsigned char> state((size_t)p);
  double amax = 0.0;
  for (int j = 0; j < p; ++j) {
    a[(size_t)j] = G[(size_t)j * ld + j];
    u[j] = 0.0;
    state[(size_t)j] = (unsigned char)l0_node_state(in_mask, out_mask, j);
    amax = std::fmax(amax, a[(size_t)j]);
  }
  for (int j = 0; j < p; ++j)
    if (!(a[(size_t)j] > L0_PIVOT * amax) || state[(size_t)j] == L0_ND_OUT) a[(size_t)j] = 0.0;  // a = 0 marks a column that keeps u_j = 0
  const double L0 = l0_node_values(u, t.data(), c, p, cell, state.data()).L;
  auto axpy = [&](int j, double w) {
    const double* row = G + (size_t)j * ld;
    for (int k = 0; k < p; ++k) t[(size_t)k] = std::fma(w, row[k], t[(size_t)k]);
  };
  auto build = [&]() {
    for (int k = 0; k < p; ++k) t[(size_t)k] = c[k];
    for (int j = 0; j < p; ++j)
      if (u[j] != 0.0) axpy(j, -u[j]);
  };
  if (start)
    for (int j = 0; j < p; ++j)
      if (a[(size_t)j] > 0.0) u[j] = start[j] < -big_M ? -big_M : (start[j] > big_M ? big_M : start[j]);
  build();
  for (int sw = 0;; ++sw) {
    if (sw == max_sweeps) {
      R.status |= L0_LS_SWEEPS_OUT;
      break;
    }
    for (int j = 0; j < p; ++j) {
      const double aj = a[(size_t)j];
      if (!(aj > 0.0)) continue;
      const double nb = l0_node_coord(t[(size_t)j] + aj * u[j], aj, cell.eta, cell.lam, cell.tauc, big_M, state[(size_t)j]);
      if (!l0_lb_changed(nb, u[j])) continue;
      const double delta = nb - u[j];
      u[j] = nb;
      axpy(j, -delta);
      ++R.changes;
    }
    ++R.sweeps;
    const L0NodeValues v = l0_node_values(u, t.data(), c, p, cell, state.data());
    if (l0_lb_closed(v.P, v.L, cell.alpha, gap_tol)) break;
  }
  build();  // no running residual feeds the certificate
  const L0NodeValues v = l0_node_values(u, t.data(), c, p, cell, state.data());
  R.lower = v.L > L0 ? v.L : L0;
  R.primal = v.P;
  R.upper = v.F;
  return R;
}

// A batch of nodes as the tree hands it to its callable: n <= L0_ND_MAX_BATCH nodes, for each its cell, its two masks, its
// parent's bound and its start; back come lower = max(the node's bound, parent_lower), primal, upper, u and (sweeps, status).
struct L0NodeBatch {
  int n;
  const int* cell;                    // [n]
  const unsigned long long* in_mask;  // [n][L0_ND_WORDS]
  const unsigned long long* out_mask; // [n][L0_ND_WORDS]
  const double* parent_lower;         // [n]
  const double* starts;               // [n][p]
  double *lower, *primal, *upper;     // [n] each
  double* u;                          // [n][p]
  int* stat;                          // [n][2]
};
// the batch on the host: the twin, node after node
inline int l0_node_batch_host(const double* G, size_t ld, const double* c, int p, const L0NodeCell* cells, int max_sweeps, double gap_tol,
                              const L0NodeBatch& b) {
  for (int i = 0; i < b.n; ++i) {
    const L0NodeResult r = l0_node_solve(G, ld, c, p, cells[b.cell[i]], b.in_mask + (size_t)i * L0_ND_WORDS, b.out_mask + (size_t)i * L0_ND_WORDS,
                                         b.starts ? b.starts + (size_t)i * p : nullptr, max_sweeps, gap_tol, b.u + (size_t)i * p);
    b.lower[i] = !b.parent_lower || r.lower > b.parent_lower[i] ? r.lower : b.parent_lower[i];  // (parent_lower NULL: none, as the kernel)
    b.primal[i] = r.primal;
    b.upper[i] = r.upper;
    b.stat[2 * i] = r.sweeps;
    b.stat[2 * i + 1] = r.status;
  }
  return 0;
}

// ---- local proof with groups (slm_solve_l0_local_group_nodes, slm_solve_l0_local_group_prove; csrc/l0_local_group_node_kernels.hpp;
// tests/l0_local_group_prove_host_test.cpp; DESIGN 4d "Local proof with groups") ------------------------------------------------
//
// The objective is the group search's, F(beta) = 1/2 beta^T H beta - c^T beta + alpha |cl(S(beta))|.  Each GROUP's indicator is
// relaxed to z_g in [0, 1] with |beta_j| <= M z_g for j in g and the cost eta ||beta_g||^2 / z_g + alpha z_g; minimising over z
// leaves phi_g(b) = min over z in [||b||_inf / M, 1] of eta ||b||^2 / z + alpha z, whose conjugate is
// phi_g*(t_g) = max(0, sum_{j in g} h(t_j) - alpha).  A node gives every GROUP one state, and for EVERY u, with t = c - G u,
//     L_node(u) = -1/2 u^T G u - sum over FREE g of max(0, sum_{j in g} h(t_j) - alpha) - sum over IN g of (sum_{j in g} h(t_j) - alpha)
// is at or below the minimum of F over the node: the relaxation ignores the hierarchy, and |cl(S)| >= |S|.  The hierarchy lives
// in the branching (l0_prove_tree with a group map).
//
// THE DESCENT on P(b) = 1/2 b^T G b - c^T b + sum phi_g(b_g), column by column in ascending order:
//   * an IN group's column steps clip(s / (a + 2 eta), +-M); an OUT group's and a failed pivot keep 0;
//   * a FREE group of one column, and a column whose group is zero elsewhere, step l0_lb_coord: phi_g is the bound's phi there;
//   * a FREE column whose group holds other non-zeros (R = their sum of squares, m = their largest modulus) gets the EXACT
//     minimiser over x of 1/2 a x^2 - s x + phi_g, by bisection on the monotone derivative (l0_gn_coord; phi_g has the three
//     regimes 2 sqrt(alpha eta) ||b||_2, eta ||b||^2 + alpha and eta M ||b||^2 / ||b||_inf + alpha ||b||_inf / M, told apart
//     without a square root), never by alternating between b and z;
//   * a FREE group of several columns that is ZERO moves iff S = sum_{j in g} h(t_j) > alpha, the exact test for zero; it then
//     moves AS ONE to eps b*, b*_j = argmax t_j b - eta b^2 on the box, with eps = min(1, (S - alpha) / D), D an upper bound of
//     |g| b*^T G b* (l0_gn_jump) -- a step that lowers P -- and the sweep goes on behind the group.
// Sums over a group are walked in ascending column order by kernel, twin and restatement alike.  The group terms of P and L are
// added in the lane of the group's FIRST column, so that singleton groups give l0_node_solve's bits.
constexpr int L0_GN_BISECT = 48;                 // halvings of one coordinate's bracket [0, min(M, |s| / a)]
constexpr int L0_GN_MODE = 14, L0_GP_MODE = 15;  // slm_point_info.mode of the two entries

// groups as the node rule and the tree take them: contiguous ascending column ranges, the CLOSED need lists (l0_lg_close) and
// their reverse (rptr, ridx: the groups that need g, transitively); cptr == NULL: no hierarchy
struct L0GroupMap {
  int ng = 0;
  const int* gstart = nullptr;
  const int* cptr = nullptr;
  const int* cidx = nullptr;
  const int* rptr = nullptr;
  const int* ridx = nullptr;
};
// the reverse of closed lists: rptr / ridx list for every group the groups whose closed list holds it, ascending
inline void l0_gp_reverse(int ng, const std::vector<int>& cptr, const std::vector<int>& cidx, std::vector<int>& rptr, std::vector<int>& ridx) {
  rptr.assign((size_t)ng + 1, 0);
  ridx.assign(cidx.size(), 0);
  for (int v : cidx) ++rptr[(size_t)v + 1];
  for (int g = 0; g < ng; ++g) rptr[(size_t)g + 1] += rptr[(size_t)g];
  std::vector<int> at(rptr.begin(), rptr.end() - 1);
  for (int g = 0; g < ng; ++g)
    for (int k = cptr[(size_t)g]; k < cptr[(size_t)g + 1]; ++k) ridx[(size_t)at[(size_t)cidx[(size_t)k]]++] = g;
}
L0_LB_INLINE constexpr int l0_gn_bit(const unsigned long long* mask, int g) { return (int)((mask[g >> 6] >> (g & 63)) & 1ull); }
// b*(t): the maximiser of t b - eta b^2 over the box
L0_LB_INLINE constexpr double l0_gn_bstar(double t, double eta, double big_M) {
  L0_LB_STRICT
  if (eta > 0.0) {
    const double b = t / (2.0 * eta);
    return b < -big_M ? -big_M : (b > big_M ? big_M : b);
  }
  return t > 0.0 ? big_M : (t < 0.0 ? -big_M : 0.0);
}
// eps of a zero group's move (0: it stays): S its sum of h(t_j), n its columns, amax the largest pivot.  b*^T G b* <= n amax
// ||b*||^2, and ||b*||^2 <= S / eta (eta > 0: eta b*^2 <= h) or <= n M^2 (eta = 0).
L0_LB_INLINE constexpr double l0_gn_jump(double S, double alpha, double eta, double big_M, double amax, int n) {
  L0_LB_STRICT
  if (!(S > alpha)) return 0.0;
  const double dn = (double)n;
  const double den = eta > 0.0 ? dn * amax * S / eta : dn * dn * amax * big_M * big_M;
  const double e = (S - alpha) / den;
  return e < 1.0 ? e : 1.0;
}
// is the derivative of 1/2 a x^2 - as x + phi_g at x >= 0 at or below zero?  (R > 0, so m > 0.)
L0_LB_INLINE constexpr bool l0_gn_below(double x, double as, double a, double R, double m, double alpha, double eta, double big_M) {
  L0_LB_STRICT
  const double w = as - a * x;
  if (!(eta > 0.0)) return (x > m ? alpha / big_M : 0.0) <= w;
  const double N2 = R + x * x, inf = x > m ? x : m;
  if (eta * N2 >= alpha) return 2.0 * eta * x <= w;  // z = 1
  if (eta * N2 * big_M * big_M <= alpha * inf * inf)  // the link binds: z = ||b||_inf / M
    return (x > m ? eta * big_M * (1.0 - R / (x * x)) + alpha / big_M : 2.0 * eta * big_M * x / m) <= w;
  return w >= 0.0 && 4.0 * alpha * eta * x * x <= w * w * N2;  // 2 sqrt(alpha eta) x / ||b||_2 <= w, squared
}
// the coordinate step of a FREE column whose group holds other non-zeros
L0_LB_INLINE constexpr double l0_gn_coord(double s, double a, double R, double m, double alpha, double eta, double big_M) {
  L0_LB_STRICT
  const double as = s < 0.0 ? -s : s;
  double hi = as / a, lo = 0.0;
  if (hi > big_M) hi = big_M;
  if (l0_gn_below(hi, as, a, R, m, alpha, eta, big_M)) {
    lo = hi;
  } else {
    for (int i = 0; i < L0_GN_BISECT; ++i) {
      const double mid = 0.5 * (lo + hi);
      if (l0_gn_below(mid, as, a, R, m, alpha, eta, big_M)) lo = mid;
      else hi = mid;
    }
  }
  return s < 0.0 ? -lo : lo;
}
// phi_g of a group of several columns from N2 = ||b||^2 and inf = ||b||_inf
L0_LB_INLINE constexpr double l0_gn_phi(double N2, double inf, double alpha, double eta, double big_M) {
  L0_LB_STRICT
  if (!(N2 > 0.0)) return 0.0;
  if (!(eta > 0.0)) return alpha * inf / big_M;
  if (eta * N2 >= alpha) return eta * N2 + alpha;
  if (eta * N2 * big_M * big_M <= alpha * inf * inf) return eta * big_M * N2 / inf + alpha * inf / big_M;
  return __builtin_sqrt(4.0 * alpha * eta * N2);
}
// a group's terms of P_node and of -L_node by state (several columns; S = sum of h(t_j))
L0_LB_INLINE constexpr double l0_gn_group_phi(double N2, double inf, double alpha, double eta, double big_M, int state) {
  L0_LB_STRICT
  if (state == L0_ND_FREE) return l0_gn_phi(N2, inf, alpha, eta, big_M);
  if (state != L0_ND_IN) return 0.0;
  return eta * N2 + alpha;
}
L0_LB_INLINE constexpr double l0_gn_group_conj(double S, double alpha, int state) {
  L0_LB_STRICT
  const double v = S - alpha;
  if (state == L0_ND_FREE) return v > 0.0 ? v : 0.0;
  if (state != L0_ND_IN) return 0.0;
  return v;
}

// cl(S(u)) by groups: in[g] = 1 where g holds a non-zero or is needed by a group that does.  Returns |cl(S)|.
inline int l0_gp_closure(const double* u, const L0GroupMap& gm, int* in) {
  for (int g = 0; g < gm.ng; ++g) in[g] = 0;
  for (int g = 0; g < gm.ng; ++g) {
    bool any = false;
    for (int j = gm.gstart[g]; j < gm.gstart[g + 1]; ++j) any = any || u[j] != 0.0;
    if (!any) continue;
    in[g] = 1;
    for (int k = gm.cptr ? gm.cptr[g] : 0; gm.cptr && k < gm.cptr[g + 1]; ++k) in[gm.cidx[k]] = 1;
  }
  int count = 0;
  for (int g = 0; g < gm.ng; ++g) count += in[g];
  return count;
}
inline L0NodeValues l0_gn_values(const double* u, const double* t, const double* c, int p, const L0NodeCell& cell, const L0GroupMap& gm,
                                 const unsigned char* gstate, double ncl) {
  L0_LB_STRICT
  double qp[64] = {0.0}, ql[64] = {0.0}, sp[64] = {0.0}, sc[64] = {0.0}, s2[64] = {0.0};
  for (int j = 0; j < p; ++j) {
    const int l = j & 63;
    qp[l] += u[j] * (c[j] + t[j]);
    ql[l] += u[j] * (c[j] - t[j]);
    s2[l] += u[j] * u[j];
  }
  for (int g = 0; g < gm.ng; ++g) {
    const int lo = gm.gstart[g], hi = gm.gstart[g + 1], l = lo & 63, st = gstate[g];
    if (hi - lo == 1) {
      sp[l] += l0_node_phi(u[lo], cell.alpha, cell.eta, cell.lam, cell.tauc, st);
      sc[l] += l0_node_conj(t[lo], cell.alpha, cell.eta, cell.big_M, st);
      continue;
    }
    double N2 = 0.0, inf = 0.0, S = 0.0;
    for (int k = lo; k < hi; ++k) {
      const double x = u[k], ax = x < 0.0 ? -x : x;
      N2 += x * x;
      inf = ax > inf ? ax : inf;
      S += l0_node_h(t[k], cell.eta, cell.big_M);
    }
    sp[l] += l0_gn_group_phi(N2, inf, cell.alpha, cell.eta, cell.big_M, st);
    sc[l] += l0_gn_group_conj(S, cell.alpha, st);
  }
  return l0_node_combine(l0_lb_wave_sum(qp), l0_lb_wave_sum(ql), l0_lb_wave_sum(sp), l0_lb_wave_sum(sc), l0_lb_wave_sum(s2), ncl, cell.alpha,
                         cell.eta);
}

// The group node kernel's twin without a device, change for change.  gin, gout: L0_ND_WORDS words each, bit g for group g.
// With singleton groups and no hierarchy it returns l0_node_solve's bits.
inline L0NodeResult l0_group_node_solve(const double* G, size_t ld, const double* c, int p, const L0NodeCell& cell, const L0GroupMap& gm,
                                        const unsigned long long* gin, const unsigned long long* gout, const double* start, int max_sweeps,
                                        double gap_tol, double* u) {
  L0_LB_STRICT
  L0NodeResult R;
  const double big_M = cell.big_M, alpha = cell.alpha, eta = cell.eta;
  std::vector<double> t(c, c + p), a((size_t)p);
  std::vector<unsigned char> gstate((size_t)gm.ng);
  std::vector<int> gof((size_t)p), closed((size_t)gm.ng);
  for (int g = 0; g < gm.ng; ++g) {
    gstate[(size_t)g] = (unsigned char)(l0_gn_bit(gin, g) | (l0_gn_bit(gout, g) << 1));
    for (int j = gm.gstart[g]; j < gm.gstart[g + 1]; ++j) gof[(size_t)j] = g;
  }
  double amax = 0.0;
  for (int j = 0; j < p; ++j) {
    a[(size_t)j] = G[(size_t)j * ld + j];
    u[j] = 0.0;
    amax = std::fmax(amax, a[(size_t)j]);
  }
  for (int j = 0; j < p; ++j)
    if (!(a[(size_t)j] > L0_PIVOT * amax) || gstate[(size_t)gof[(size_t)j]] == L0_ND_OUT) a[(size_t)j] = 0.0;
  const double L0 = l0_gn_values(u, t.data(), c, p, cell, gm, gstate.data(), 0.0).L;
  auto axpy = [&](int j, double w) {
    const double* row = G + (size_t)j * ld;
    for (int k = 0; k < p; ++k) t[(size_t)k] = std::fma(w, row[k], t[(size_t)k]);
  };
  auto build = [&]() {
    for (int k = 0; k < p; ++k) t[(size_t)k] = c[k];
    for (int j = 0; j < p; ++j)
      if (u[j] != 0.0) axpy(j, -u[j]);
  };
  if (start)
    for (int j = 0; j < p; ++j)
      if (a[(size_t)j] > 0.0) u[j] = start[j] < -big_M ? -big_M : (start[j] > big_M ? big_M : start[j]);
  build();
  for (int sw = 0;; ++sw) {
    if (sw == max_sweeps) {
      R.status |= L0_LS_SWEEPS_OUT;
      break;
    }
    for (int j = 0; j < p; ++j) {
      const double aj = a[(size_t)j];
      if (!(aj > 0.0)) continue;
      const int g = gof[(size_t)j], lo = gm.gstart[g], hi = gm.gstart[g + 1], st = gstate[(size_t)g];
      const double s = t[(size_t)j] + aj * u[j];
      double nb = 0.0;
      if (st != L0_ND_FREE || hi - lo == 1) {
        nb = l0_node_coord(s, aj, eta, cell.lam, cell.tauc, big_M, st);
      } else {
        double Rr = 0.0, m = 0.0, S = 0.0;
        for (int k = lo; k < hi; ++k) {
          S += l0_node_h(t[(size_t)k], eta, big_M);
          if (k == j) continue;
          const double x = u[k], ax = x < 0.0 ? -x : x;
          Rr += x * x;
          m = ax > m ? ax : m;
        }
        if (!(Rr > 0.0) && u[j] == 0.0) {  // the group is zero: it moves as one, or not at all
          const double eps = l0_gn_jump(S, alpha, eta, big_M, amax, hi - lo);
          nb = eps * l0_gn_bstar(t[(size_t)j], eta, big_M);
          if (!l0_lb_changed(nb, 0.0)) continue;
          for (int k = lo; k < hi; ++k)
            if (a[(size_t)k] > 0.0) u[k] = eps * l0_gn_bstar(t[(size_t)k], eta, big_M);
          for (int k = lo; k < hi; ++k)
            if (u[k] != 0.0) {
              axpy(k, -u[k]);
              ++R.changes;
            }
          j = hi - 1;
          continue;
        }
        nb = !(Rr > 0.0) ? l0_lb_coord(s, aj, eta, cell.lam, cell.tauc, big_M) : l0_gn_coord(s, aj, Rr, m, alpha, eta, big_M);
      }
      if (!l0_lb_changed(nb, u[j])) continue;
      const double delta = nb - u[j];
      u[j] = nb;
      axpy(j, -delta);
      ++R.changes;
    }
    ++R.sweeps;
    const L0NodeValues v = l0_gn_values(u, t.data(), c, p, cell, gm, gstate.data(), 0.0);
    if (l0_lb_closed(v.P, v.L, alpha, gap_tol)) break;
  }
  build();
  const L0NodeValues v = l0_gn_values(u, t.data(), c, p, cell, gm, gstate.data(), (double)l0_gp_closure(u, gm, closed.data()));
  R.lower = v.L > L0 ? v.L : L0;
  R.primal = v.P;
  R.upper = v.F;
  return R;
}
// the batch on the host: the group twin, node after node
inline int l0_group_node_batch_host(const double* G, size_t ld, const double* c, int p, const L0NodeCell* cells, const L0GroupMap& gm,
                                    int max_sweeps, double gap_tol, const L0NodeBatch& b) {
  for (int i = 0; i < b.n; ++i) {
    const L0NodeResult r = l0_group_node_solve(G, ld, c, p, cells[b.cell[i]], gm, b.in_mask + (size_t)i * L0_ND_WORDS,
                                               b.out_mask + (size_t)i * L0_ND_WORDS, b.starts ? b.starts + (size_t)i * p : nullptr, max_sweeps,
                                               gap_tol, b.u + (size_t)i * p);
    b.lower[i] = !b.parent_lower || r.lower > b.parent_lower[i] ? r.lower : b.parent_lower[i];
    b.primal[i] = r.primal;
    b.upper[i] = r.upper;
    b.stat[2 * i] = r.sweeps;
    b.stat[2 * i + 1] = r.status;
  }
  return 0;
}

// The GROUP a node is split on: the FREE group whose optimal z_g is closest to 1/2 among those strictly between 0 and 1 (ties:
// the lowest index); where every FREE z_g is 0 or 1, the FREE group of largest ||u_g||_inf > 0, and where all are zero that of
// largest sum of h(t_j), t = c - G u.  z_g of one column is the column rule's min(|u| / tauc, 1); of several it is
// sqrt(eta ||u_g||^2 / alpha) held in [||u_g||_inf / M, 1] (eta = 0: ||u_g||_inf / M).  -1: no group is FREE.
inline int l0_gp_branch(const double* G, size_t ld, const double* c, int p, const L0NodeCell& cell, const L0GroupMap& gm,
                        const unsigned long long* gin, const unsigned long long* gout, const double* u) {
  L0_LB_STRICT
  int pick = -1;
  double dist = 1.0, top = 0.0;
  for (int g = 0; g < gm.ng; ++g) {
    if (l0_gn_bit(gin, g) || l0_gn_bit(gout, g)) continue;
    const int lo = gm.gstart[g], hi = gm.gstart[g + 1];
    double z = 0.0;
    if (hi - lo == 1) {
      const double au = std::fabs(u[lo]);
      z = cell.tauc > 0.0 ? (au / cell.tauc < 1.0 ? au / cell.tauc : 1.0) : (au > 0.0 ? 1.0 : 0.0);
    } else {
      double N2 = 0.0, inf = 0.0;
      for (int k = lo; k < hi; ++k) {
        N2 += u[k] * u[k];
        inf = std::fabs(u[k]) > inf ? std::fabs(u[k]) : inf;
      }
      if (N2 > 0.0) {
        const double low = inf / cell.big_M;
        if (!(cell.eta > 0.0)) {
          z = low;
        } else {
          const double zs = cell.alpha > 0.0 ? std::sqrt(cell.eta * N2 / cell.alpha) : 1.0;
          z = zs < low ? low : (zs > 1.0 ? 1.0 : zs);
        }
      }
    }
    if (!(z > 0.0 && z < 1.0)) continue;
    const double d = std::fabs(z - 0.5);
    if (d < dist) {
      dist = d;
      pick = g;
    }
  }
  if (pick >= 0) return pick;
  for (int g = 0; g < gm.ng; ++g) {
    if (l0_gn_bit(gin, g) || l0_gn_bit(gout, g)) continue;
    double inf = 0.0;
    for (int k = gm.gstart[g]; k < gm.gstart[g + 1]; ++k) inf = std::fabs(u[k]) > inf ? std::fabs(u[k]) : inf;
    if (inf > top) {
      top = inf;
      pick = g;
    }
  }
  if (pick >= 0) return pick;
  std::vector<double> t(c, c + p);
  for (int k = 0; k < p; ++k)
    if (u[k] != 0.0)
      for (int j = 0; j < p; ++j) t[(size_t)j] -= G[(size_t)k * ld + j] * u[k];
  top = -1.0;
  for (int g = 0; g < gm.ng; ++g) {
    if (l0_gn_bit(gin, g) || l0_gn_bit(gout, g)) continue;
    double S = 0.0;
    for (int k = gm.gstart[g]; k < gm.gstart[g + 1]; ++k) S += l0_node_h(t[(size_t)k], cell.eta, cell.big_M);
    if (S > top) {
      top = S;
      pick = g;
    }
  }
  return pick;
}
// the masks of the children of a split on group g: the IN child takes g and need*(g), the OUT child g and every group that needs g
inline void l0_gp_child(const L0GroupMap& gm, int g, bool in_child, unsigned long long* mask) {
  mask[g >> 6] |= 1ull << (g & 63);
  const int* ptr = in_child ? gm.cptr : gm.rptr;
  const int* idx = in_child ? gm.cidx : gm.ridx;
  for (int k = ptr ? ptr[g] : 0; ptr && k < ptr[g + 1]; ++k) mask[idx[k] >> 6] |= 1ull << (idx[k] & 63);
}

// The column a node is split on: the FREE column whose z_j = min(|u_j| / tauc, 1) (tauc = 0: 1 where u_j != 0) is closest to
// 1/2 among those strictly between 0 and 1, ties to the lowest index; where every FREE z_j is 0 or 1, the FREE column of largest
// |u_j| > 0, and where all are zero that of largest |t_j|, t = c - G u.  -1: no column is FREE.
inline int l0_prove_branch(const double* G, size_t ld, const double* c, int p, double tauc, const unsigned long long* in_mask,
                           const unsigned long long* out_mask, const double* u) {
  L0_LB_STRICT
  int pick = -1;
  double dist = 1.0, top = 0.0;
  for (int j = 0; j < p; ++j) {
    if (l0_node_state(in_mask, out_mask, j) != L0_ND_FREE) continue;
    const double au = std::fabs(u[j]);
    const double z = tauc > 0.0 ? (au / tauc < 1.0 ? au / tauc : 1.0) : (au > 0.0 ? 1.0 : 0.0);
    if (!(z > 0.0 && z < 1.0)) continue;
    const double d = std::fabs(z - 0.5);
    if (d < dist) {
      dist = d;
      pick = j;
    }
  }
  if (pick >= 0) return pick;
  for (int j = 0; j < p; ++j)
    if (l0_node_state(in_mask, out_mask, j) == L0_ND_FREE && std::fabs(u[j]) > top) {
      top = std::fabs(u[j]);
      pick = j;
    }
  if (pick >= 0) return pick;
  std::vector<double> t(c, c + p);
  for (int k = 0; k < p; ++k)
    if (u[k] != 0.0)
      for (int j = 0; j < p; ++j) t[(size_t)j] -= G[(size_t)k * ld + j] * u[k];
  top = -1.0;
  for (int j = 0; j < p; ++j)
    if (l0_node_state(in_mask, out_mask, j) == L0_ND_FREE && std::fabs(t[(size_t)j]) > top) {
      top = std::fabs(t[(size_t)j]);
      pick = j;
    }
  return pick;
}
// F(beta) = 1/2 beta^T (G + 2 eta I) beta - c^T beta + alpha nnz(beta), summed over the support in l0_boxed's order
inline double l0_prove_value(const double* G, size_t ld, const double* c, int p, double alpha, double eta, const double* beta) {
  L0_LB_STRICT
  double val = 0.0;
  int nnz = 0;
  for (int r = 0; r < p; ++r) {
    if (beta[r] == 0.0) continue;
    double t = 0.0;
    for (int k = 0; k < p; ++k)
      if (beta[k] != 0.0) t += (G[(size_t)r * ld + k] + (r == k ? 2.0 * eta : 0.0)) * beta[k];
    val += beta[r] * (0.5 * t - c[r]);
    ++nnz;
  }
  return val + alpha * (double)nnz;
}
// should a node of bound `lower` be dropped against the incumbent `best`?
inline bool l0_prove_pruned(double best, double lower, double alpha, double rel_gap) {
  L0_LB_STRICT
  const double ab = std::fabs(best);
  return best - lower <= rel_gap * (ab > alpha ? ab : alpha);
}

// the leaves a proof rests on: every node that was dropped (pruned against the incumbent, or with no FREE column left)
struct L0ProveLeaves {
  long long capacity = 0, count = 0;  // count goes on past capacity: what the caller's arrays would have had to hold
  int* cell = nullptr;                // [capacity]
  unsigned long long* in_mask = nullptr;   // [capacity][L0_ND_WORDS]
  unsigned long long* out_mask = nullptr;  // [capacity][L0_ND_WORDS]
  double* u = nullptr;                // [capacity][p]
  double* lower = nullptr;            // [capacity]
};

// The tree, for every cell of a grid at once.  Per cell: the incumbent (the caller's where its value is below 0, else the empty
// support at 0); the root; then rounds: the `width` open nodes of lowest bound are popped (ties: the older node), each is split
// on l0_prove_branch's column into an IN child and an OUT child, both started from the parent's u; ALL children of ALL cells of a
// round go into ONE call of `bound`, at most L0_ND_MAX_BATCH nodes (the width of a round is cut to fit, and cells the batch has
// no room for wait for the next round).  A child whose F(u) is below the incumbent replaces it, and l0_ls_polish_on on its support
// replaces that where it is lower still.  A node is dropped when best - lower <= rel_gap max(|best|, alpha).  A cell ends
// L0_PV_OPTIMAL when no node is open, L0_PV_NODE_LIMIT when max_nodes bound evaluations leave no room for two more (or a node
// with no FREE column left is still open: its relaxation ran out of sweeps); either way lower_bound = min(best, the lowest open
// bound) is proven.  Deterministic: the same `bound` bits give the same tree.  Returns what `bound` returned when that is not 0.
template <class Bound>
inline int l0_prove_tree(const double* G, size_t ld, const double* c, int p, int n_cells, const L0NodeCell* cells, const double* incumbents,
                         double rel_gap, int max_nodes, int width, Bound&& bound, double* beta_out, double* objective_out,
                         double* lower_out, int* nodes_out, int* rounds_out, int* status_out, L0ProveLeaves* leaves = nullptr,
                         const L0GroupMap* groups = nullptr) {
  struct Node {
    unsigned long long in[L0_ND_WORDS], out[L0_ND_WORDS];
    double lower;
    std::vector<double> u;
  };
  struct Cell {
    std::map<std::pair<double, long long>, Node> open;
    std::vector<double> beta;
    double best = 0.0, stuck = INFINITY;
    int nodes = 0, rounds = 0;
    bool done = false, limit = false;
  };
  std::vector<Cell> T((size_t)n_cells);
  long long seq = 0;
  auto leaf = [&](int e, const Node& nd) {
    if (!leaves) return;
    const long long at = leaves->count++;
    if (at >= leaves->capacity) return;
    leaves->cell[at] = e;
    memcpy(leaves->in_mask + (size_t)at * L0_ND_WORDS, nd.in, sizeof(nd.in));
    memcpy(leaves->out_mask + (size_t)at * L0_ND_WORDS, nd.out, sizeof(nd.out));
    memcpy(leaves->u + (size_t)at * p, nd.u.data(), sizeof(double) * (size_t)p);
    leaves->lower[at] = nd.lower;
  };
  for (int e = 0; e < n_cells; ++e) {
    Cell& t = T[(size_t)e];
    t.beta.assign((size_t)p, 0.0);
    if (incumbents) {
      std::vector<int> closed(groups ? (size_t)groups->ng : 0);
      const double F = groups ? l0_prove_value(G, ld, c, p, 0.0, cells[e].eta, incumbents + (size_t)e * p) +
                                    cells[e].alpha * (double)l0_gp_closure(incumbents + (size_t)e * p, *groups, closed.data())
                              : l0_prove_value(G, ld, c, p, cells[e].alpha, cells[e].eta, incumbents + (size_t)e * p);
      if (F < 0.0) {
        t.best = F;
        t.beta.assign(incumbents + (size_t)e * p, incumbents + (size_t)(e + 1) * p);
      }
    }
  }
  std::vector<int> b_cell;
  std::vector<unsigned long long> b_in, b_out;
  std::vector<double> b_parent, b_start, b_lower, b_primal, b_upper, b_u;
  std::vector<int> b_stat;
  for (int round = 0;; ++round) {
    b_cell.clear(); b_in.clear(); b_out.clear(); b_parent.clear(); b_start.clear();
    auto push = [&](int e, const unsigned long long* in, const unsigned long long* out, double parent, const double* start) {
      b_cell.push_back(e);
      b_in.insert(b_in.end(), in, in + L0_ND_WORDS);
      b_out.insert(b_out.end(), out, out + L0_ND_WORDS);
      b_parent.push_back(parent);
      if (start) b_start.insert(b_start.end(), start, start + p);
      else b_start.insert(b_start.end(), (size_t)p, 0.0);
    };
    if (round == 0) {
      const unsigned long long none[L0_ND_WORDS] = {0};
      for (int e = 0; e < n_cells; ++e) {
        push(e, none, none, -INFINITY, nullptr);
        ++T[(size_t)e].rounds;
      }
    } else {
      int active = 0;
      for (int e = 0; e < n_cells; ++e) active += !T[(size_t)e].done;
      if (active == 0) break;
      const int fit = std::max(1, std::min(width, L0_ND_MAX_BATCH / 2 / active));
      for (int e = 0; e < n_cells; ++e) {
        Cell& t = T[(size_t)e];
        if (t.done) continue;
        int popped = 0;
        while (!t.open.empty() && popped < fit) {
          if (t.nodes + 2 * (popped + 1) > max_nodes) {
            t.limit = true;
            break;
          }
          if ((int)b_cell.size() + 2 > L0_ND_MAX_BATCH) break;  // no room in this round: the cell waits
          Node nd = std::move(t.open.begin()->second);
          t.open.erase(t.open.begin());
          const int j = groups ? l0_gp_branch(G, ld, c, p, cells[e], *groups, nd.in, nd.out, nd.u.data())
                               : l0_prove_branch(G, ld, c, p, cells[e].tauc, nd.in, nd.out, nd.u.data());
          if (j < 0) {  // every column is fixed and the node is still open: its relaxation was not closed
            t.stuck = std::min(t.stuck, nd.lower);
            leaf(e, nd);
            continue;
          }
          if (groups) {  // (a split on a GROUP: the IN child takes what the group needs, the OUT child what needs the group)
            unsigned long long child[L0_ND_WORDS];
            memcpy(child, nd.in, sizeof(child));
            l0_gp_child(*groups, j, true, child);
            push(e, child, nd.out, nd.lower, nd.u.data());
            memcpy(child, nd.out, sizeof(child));
            l0_gp_child(*groups, j, false, child);
            push(e, nd.in, child, nd.lower, nd.u.data());
            ++popped;
            continue;
          }
          nd.in[j >> 6] |= 1ull << (j & 63);
          push(e, nd.in, nd.out, nd.lower, nd.u.data());
          nd.in[j >> 6] &= ~(1ull << (j & 63));
          nd.out[j >> 6] |= 1ull << (j & 63);
          push(e, nd.in, nd.out, nd.lower, nd.u.data());
          ++popped;
        }
        if (popped) ++t.rounds;
        if (t.open.empty() && popped == 0) t.done = true;
        if (t.limit && popped == 0) t.done = true;
      }
    }
    const int n = (int)b_cell.size();
    if (n == 0) continue;  // (cells ended in this round: the next round sees none active)
    b_lower.assign((size_t)n, 0.0); b_primal.assign((size_t)n, 0.0); b_upper.assign((size_t)n, 0.0);
    b_u.assign((size_t)n * p, 0.0); b_stat.assign((size_t)n * 2, 0);
    const L0NodeBatch batch{n, b_cell.data(), b_in.data(), b_out.data(), b_parent.data(), b_start.data(), b_lower.data(), b_primal.data(),
                            b_upper.data(), b_u.data(), b_stat.data()};
    const int rc = bound(batch);
    if (rc != 0) return rc;
    for (int i = 0; i < n; ++i) {  // the incumbents first, so that every child of the round meets the round's best
      const int e = b_cell[(size_t)i];
      Cell& t = T[(size_t)e];
      ++t.nodes;
      if (!(b_upper[(size_t)i] < t.best)) continue;
      const double* u = b_u.data() + (size_t)i * p;
      t.best = b_upper[(size_t)i];
      t.beta.assign(u, u + p);
      std::vector<double> pol(u, u + p);
      std::vector<int> cols;
      int nnz = 0;
      if (groups) {  // (the group search's polish: every column of the groups in cl(S), inside the box; alpha counts cl(S) after it)
        std::vector<int> closed((size_t)groups->ng);
        l0_gp_closure(u, *groups, closed.data());
        for (int g = 0; g < groups->ng; ++g)
          for (int j = groups->gstart[g]; closed[(size_t)g] && j < groups->gstart[g + 1]; ++j) cols.push_back(j);
      } else {
        for (int j = 0; j < p; ++j)
          if (pol[(size_t)j] != 0.0) cols.push_back(j);
      }
      const double quad = l0_ls_polish_on(G, ld, c, cells[e].eta, cells[e].big_M, cols, pol.data());
      if (groups) {
        std::vector<int> closed((size_t)groups->ng);
        nnz = l0_gp_closure(pol.data(), *groups, closed.data());
      } else {
        for (int j = 0; j < p; ++j) nnz += pol[(size_t)j] != 0.0;
      }
      const double F = quad + cells[e].alpha * (double)nnz;
      if (F < t.best) {
        t.best = F;
        t.beta = pol;
      }
    }
    for (int i = 0; i < n; ++i) {
      const int e = b_cell[(size_t)i];
      Cell& t = T[(size_t)e];
      Node nd;
      memcpy(nd.in, b_in.data() + (size_t)i * L0_ND_WORDS, sizeof(nd.in));
      memcpy(nd.out, b_out.data() + (size_t)i * L0_ND_WORDS, sizeof(nd.out));
      nd.lower = b_lower[(size_t)i];
      nd.u.assign(b_u.data() + (size_t)i * p, b_u.data() + (size_t)(i + 1) * p);
      if (l0_prove_pruned(t.best, nd.lower, cells[e].alpha, rel_gap)) leaf(e, nd);
      else t.open.emplace(std::make_pair(nd.lower, seq++), std::move(nd));
    }
    for (int e = 0; e < n_cells; ++e) {  // an incumbent that improved closes open nodes: from the highest bound down
      Cell& t = T[(size_t)e];
      while (!t.open.empty()) {
        auto last = std::prev(t.open.end());
        if (!l0_prove_pruned(t.best, last->second.lower, cells[e].alpha, rel_gap)) break;
        leaf(e, last->second);
        t.open.erase(last);
      }
    }
  }
  for (int e = 0; e < n_cells; ++e) {
    const Cell& t = T[(size_t)e];
    double low = std::min(t.best, t.stuck);
    if (!t.open.empty()) low = std::min(low, t.open.begin()->first.first);
    memcpy(beta_out + (size_t)e * p, t.beta.data(), sizeof(double) * (size_t)p);
    objective_out[e] = t.best;
    lower_out[e] = low;
    nodes_out[e] = t.nodes;
    rounds_out[e] = t.rounds;
    status_out[e] = t.open.empty() && l0_prove_pruned(t.best, t.stuck, cells[e].alpha, rel_gap) ? L0_PV_OPTIMAL : L0_PV_NODE_LIMIT;
  }
  return 0;
}
#if !defined(__clang__)
#pragma GCC pop_options
#endif

// What slm_solve_l0_local_nodes refuses before a device is touched, in this order; which: the offending cell, node or entry.
enum L0NdRefusal { L0_ND_OK = 0, L0_ND_NULL, L0_ND_CELLS, L0_ND_PROBLEMS, L0_ND_NODES, L0_ND_BATCH, L0_ND_BIG_M, L0_ND_ALPHA, L0_ND_ETA,
                   L0_ND_GAP_TOL, L0_ND_WIDTH, L0_ND_CELL, L0_ND_MASK, L0_ND_PARENT, L0_ND_START, L0_ND_GROUPS, L0_ND_SHARDED };
inline L0NdRefusal l0_nodes_check(long long n_cells, const double* alphas, const double* etas, double big_M, long long n_nodes,
                                  const int* cell, const unsigned long long* in_mask, const unsigned long long* out_mask,
                                  const double* parent_lower, const double* starts, long long p, double gap_tol, bool singleton, bool sharded,
                                  long long* which = nullptr) {
  if (!alphas || !etas || !cell || !in_mask || !out_mask) return L0_ND_NULL;
  if (n_cells < 1) return L0_ND_CELLS;
  if (n_cells > L0_LS_MAX_PROBLEMS) return L0_ND_PROBLEMS;
  if (n_nodes < 1) return L0_ND_NODES;
  if (n_nodes > L0_ND_MAX_BATCH) return L0_ND_BATCH;
  if (!(big_M >= 0.0)) return L0_ND_BIG_M;
  for (long long e = 0; e < n_cells; ++e) {
    if (which) *which = e;
    if (!(alphas[e] >= 0.0) || !std::isfinite(alphas[e])) return L0_ND_ALPHA;
    if (!(etas[e] >= 0.0) || !std::isfinite(etas[e])) return L0_ND_ETA;
  }
  if (!(gap_tol >= 0.0)) return L0_ND_GAP_TOL;
  if (p > L0_LS_PMAX) return L0_ND_WIDTH;
  for (long long i = 0; i < n_nodes; ++i) {
    if (which) *which = i;
    if (cell[i] < 0 || cell[i] >= n_cells) return L0_ND_CELL;
    for (int w = 0; w < L0_ND_WORDS; ++w)  // a column is IN or OUT, not both
      if (in_mask[i * L0_ND_WORDS + w] & out_mask[i * L0_ND_WORDS + w]) return L0_ND_MASK;
  }
  for (long long i = 0; parent_lower && i < n_nodes; ++i)  // a parent's bound is a number or -infinity: a NaN, or +infinity, is neither
    if (!(parent_lower[i] < INFINITY)) {
      if (which) *which = i;
      return L0_ND_PARENT;
    }
  for (long long e = 0; starts && e < n_nodes * p; ++e)
    if (!std::isfinite(starts[e])) {
      if (which) *which = e;
      return L0_ND_START;
    }
  if (!singleton) return L0_ND_GROUPS;
  if (sharded) return L0_ND_SHARDED;
  return L0_ND_OK;
}

// What slm_solve_l0_local_prove refuses before a device is touched, in this order: the bound's, and the tree's own.
enum L0PvRefusal { L0_PV_OK = 0, L0_PV_NULL, L0_PV_CELLS, L0_PV_PROBLEMS, L0_PV_BIG_M, L0_PV_ALPHA, L0_PV_ETA, L0_PV_REL_GAP, L0_PV_MAX_NODES,
                   L0_PV_TREE_WIDTH, L0_PV_WIDTH, L0_PV_INCUMBENT, L0_PV_GROUPS, L0_PV_SHARDED };
inline L0PvRefusal l0_prove_check(long long n_cells, const double* alphas, const double* etas, double big_M, const double* incumbents,
                                  long long p, double rel_gap, long long max_nodes, long long width, bool singleton, bool sharded,
                                  long long* which = nullptr) {
  if (!alphas || !etas) return L0_PV_NULL;
  if (n_cells < 1) return L0_PV_CELLS;
  if (n_cells > L0_LS_MAX_PROBLEMS) return L0_PV_PROBLEMS;
  if (!(big_M >= 0.0)) return L0_PV_BIG_M;
  for (long long e = 0; e < n_cells; ++e) {
    if (which) *which = e;
    if (!(alphas[e] >= 0.0) || !std::isfinite(alphas[e])) return L0_PV_ALPHA;
    if (!(etas[e] >= 0.0) || !std::isfinite(etas[e])) return L0_PV_ETA;
  }
  if (!(rel_gap >= 1e-10 && rel_gap <= 1.0)) return L0_PV_REL_GAP;
  if (max_nodes < 1) return L0_PV_MAX_NODES;
  if (width < 1) return L0_PV_TREE_WIDTH;
  if (p > L0_LS_PMAX) return L0_PV_WIDTH;
  for (long long e = 0; incumbents && e < n_cells * p; ++e)
    if (!(std::fabs(incumbents[e]) <= big_M)) {  // (a NaN fails too)
      if (which) *which = e;
      return L0_PV_INCUMBENT;
    }
  if (!singleton) return L0_PV_GROUPS;
  if (sharded) return L0_PV_SHARDED;
  return L0_PV_OK;
}

// What the two grouped entries refuse before a device is touched, in this order: everything slm_solve_l0_local_nodes
// (slm_solve_l0_local_prove) refuses up to its groups (nd, pv); groups that are not contiguous and ascending (which: the
// column); a need_ptr that does not start at 0 or falls (which: the group); a need_idx outside the groups, or a NULL need_idx
// under a non-empty need_ptr (which: the entry); for the nodes entry a mask bit beyond the groups, then masks that are not
// CLOSED -- an IN group whose need*(g) is not all IN, or an OUT group needed by one that is not OUT (which: the node); a
// row-sharded dataset.  gid: [p] the dataset's group index, or NULL for singleton groups; *n_groups: the groups found.
enum L0GpKind { L0_GP_OK = 0, L0_GP_FIRST, L0_GP_ORDER, L0_GP_NEED_PTR, L0_GP_NEED_IDX, L0_GP_RANGE, L0_GP_UNCLOSED, L0_GP_SHARDED };
struct L0GpRefusal {
  L0GpKind kind = L0_GP_OK;
  L0NdRefusal nd = L0_ND_OK;
  L0PvRefusal pv = L0_PV_OK;
  long long which = 0;
};
inline L0GpKind l0_gp_groups_check(long long p, const int* gid, const int* need_ptr, const int* need_idx, long long* which, int* n_groups) {
  for (long long j = 0; gid && j < p; ++j) {
    const int step = j == 0 ? gid[0] + 1 : gid[j] - gid[j - 1];
    if ((step != 0 && step != 1) || (j == 0 && step != 1)) {
      *which = j;
      return L0_GP_ORDER;
    }
  }
  const long long ng = p < 1 ? 0 : (gid ? (long long)gid[p - 1] + 1 : p);
  if (n_groups) *n_groups = (int)ng;
  if (need_ptr) {
    *which = 0;
    if (need_ptr[0] != 0) return L0_GP_NEED_PTR;
    for (long long g = 0; g < ng; ++g)
      if (need_ptr[g + 1] < need_ptr[g]) {
        *which = g + 1;
        return L0_GP_NEED_PTR;
      }
    if (need_ptr[ng] > 0 && !need_idx) return L0_GP_NEED_IDX;
    for (long long k = 0; k < need_ptr[ng]; ++k)
      if (need_idx[k] < 0 || need_idx[k] >= ng) {
        *which = k;
        return L0_GP_NEED_IDX;
      }
  }
  return L0_GP_OK;
}
inline L0GpRefusal l0_group_nodes_check(long long n_cells, const double* alphas, const double* etas, double big_M, long long n_nodes,
                                        const int* cell, const unsigned long long* in_mask, const unsigned long long* out_mask,
                                        const double* parent_lower, const double* starts, long long p, double gap_tol, const int* gid,
                                        const int* need_ptr, const int* need_idx, bool sharded, int* n_groups = nullptr) {
  L0GpRefusal R;
  R.nd = l0_nodes_check(n_cells, alphas, etas, big_M, n_nodes, cell, in_mask, out_mask, parent_lower, starts, p, gap_tol, true, false, &R.which);
  if (R.nd != L0_ND_OK) {
    R.kind = L0_GP_FIRST;
    return R;
  }
  int ng = 0;
  R.kind = l0_gp_groups_check(p, gid, need_ptr, need_idx, &R.which, &ng);
  if (n_groups) *n_groups = ng;
  if (R.kind != L0_GP_OK) return R;
  std::vector<int> cptr, cidx;
  l0_lg_close(ng, need_ptr, need_idx, cptr, cidx);
  for (long long i = 0; i < n_nodes; ++i) {
    const unsigned long long *in = in_mask + i * L0_ND_WORDS, *out = out_mask + i * L0_ND_WORDS;
    R.which = i;
    for (int g = ng; g < 64 * L0_ND_WORDS; ++g)
      if (l0_gn_bit(in, g) || l0_gn_bit(out, g)) {
        R.kind = L0_GP_RANGE;
        return R;
      }
    for (int g = 0; g < ng; ++g)
      for (int k = cptr[(size_t)g]; k < cptr[(size_t)g + 1]; ++k) {
        const int h = cidx[(size_t)k];  // g needs h
        if ((l0_gn_bit(in, g) && !l0_gn_bit(in, h)) || (l0_gn_bit(out, h) && !l0_gn_bit(out, g))) {
          R.kind = L0_GP_UNCLOSED;
          return R;
        }
      }
  }
  R.which = 0;
  if (sharded) R.kind = L0_GP_SHARDED;
  return R;
}
inline L0GpRefusal l0_group_prove_check(long long n_cells, const double* alphas, const double* etas, double big_M, const double* incumbents,
                                        long long p, double rel_gap, long long max_nodes, long long width, const int* gid, const int* need_ptr,
                                        const int* need_idx, bool sharded, int* n_groups = nullptr) {
  L0GpRefusal R;
  R.pv = l0_prove_check(n_cells, alphas, etas, big_M, incumbents, p, rel_gap, max_nodes, width, true, false, &R.which);
  if (R.pv != L0_PV_OK) {
    R.kind = L0_GP_FIRST;
    return R;
  }
  R.kind = l0_gp_groups_check(p, gid, need_ptr, need_idx, &R.which, n_groups);
  if (R.kind != L0_GP_OK) return R;
  R.which = 0;
  if (sharded) R.kind = L0_GP_SHARDED;
  return R;
}

}  // namespace slm
