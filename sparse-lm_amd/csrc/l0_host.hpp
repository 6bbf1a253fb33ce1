// Host side of the exact l0 search (l0_kernels.hpp, engine_l0.hip): the limits and tolerances the kernel and the host share,
// the factor of H on a growing list of columns as the kernel keeps it, the boxed descent candidates are compared by, and the
// value and coefficients of one support, the same for l1 mode (a lasso per support: the descent, its polish, the dual
// bound on all columns), and for profile mode the pruning rule and the two questions its table answers.  Like host_logic.hpp and tail_logic.hpp it is free of HIP types so that g++
// compiles it alone: tests/host_logic_test.cpp, tests/l1l0_host_test.cpp and tests/l0_profile_host_test.cpp run these functions on the CPU under the sanitizers, and slm_solve_l0 / slm_solve_l0_l1 / slm_solve_l0_profile call
// THESE functions for the seed, the bound q_all and the winner's coefficients -- what is tested is what runs.  The wide mode
// (slm_solve_l0_wide, slm_solve_l0_profile_wide; tests/l0_wide_host_test.cpp) adds masks of two words, a factor with a capacity
// parameter and the capacity rule.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <cmath>
#include <memory>
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

// A proven lower bound on f(all columns) = min_b 1/2 b^T G b - c^T b + eta ||b||_1 (the box can only raise it): the larger of
// q_all and the lasso dual value at a feasible point.  With the primal 1/(2n)||y - X b||^2 + eta ||b||_1 = f + yy / 2
// (yy = y^T W y / n), the dual is  max D(nu) = yy/2 - n/2 ||nu - y/n||^2  over ||X^T nu||_inf <= eta.  For any b,
// nu = s (y - X b) / n has X^T nu = -s (G b - c), feasible for s = min(1, eta / ||G b - c||_inf), and
//     D(nu) - yy/2 = -1/2 s^2 rr + s ry - 1/2 yy,    rr = yy - 2 c^T b + b^T G b,  ry = yy - c^T b
// (at eta -> 0, s = 1 and b the least-squares solution this is -1/2 c^T b = q_all).  b comes from the descent on all
// columns without the box; only its quality, never its validity, depends on how far that descent got.  The value is
// lowered by a margin that covers the rounding of the sums and of a Gram that is itself a rounded product.
inline double l0_l1_lower_bound(const double* G, const double* c, int p, double yy, double eta, double q_all) {
  if (p <= 0 || p > L0_PMAX || !(eta > 0.0)) return q_all;
  int cols[L0_PMAX];
  double b[L0_PMAX];
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

}  // namespace slm
