// Host side of the exact l0 search (l0_kernels.hpp, engine_l0.hip): the limits and tolerances the kernel and the host share,
// the factor of H on a growing list of columns as the kernel keeps it, the boxed descent candidates are compared by, and the
// value and coefficients of one support.  Like host_logic.hpp and tail_logic.hpp it is free of HIP types so that g++
// compiles it alone: tests/host_logic_test.cpp runs these functions on the CPU under the sanitizers, and slm_solve_l0 calls
// THESE functions for the seed, the bound q_all and the winner's coefficients -- what is tested is what runs.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace slm {

constexpr int L0_PMAX = 64;        // columns, and groups
constexpr int L0_CD_SWEEPS = 10000;
constexpr double L0_CD_TOL = 1e-12;
constexpr double L0_PIVOT = 1e-12;

// The factor of H on a growing list of columns, as the kernel keeps it: L row by row, w = L^-1 c, value = -1/2 ||w||^2.
struct L0Factor {
  const double* H;
  const double* c;
  int p;
  double L[L0_PMAX][L0_PMAX];
  double w[L0_PMAX];
  int col[L0_PMAX];
  int m = 0;
  double ss = 0.0;
  L0Factor(const double* H_, const double* c_, int p_) : H(H_), c(c_), p(p_) {}
  bool push(int j) {  // false: the column depends on the included ones (the kernel's pivot rule)
    double x[L0_PMAX];
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
inline double l0_support(const double* H, const double* c, int p, const std::vector<int>& gstart, unsigned long long mask, double big_M,
                  bool polish, double* beta) {
  L0Factor f(H, c, p);
  const int ng = (int)gstart.size() - 1;
  for (int g = 0; g < ng; ++g)
    if ((mask >> g) & 1)
      for (int j = gstart[(size_t)g]; j < gstart[(size_t)g + 1]; ++j) (void)f.push(j);
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

}  // namespace slm
