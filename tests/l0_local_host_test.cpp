// CPU test of the host side of the l0 local search (slm_solve_l0_local) in csrc/l0_host.hpp: l0_local_solve<false>, the rule without a
// device and the kernel's twin, l0_ls_polish and the argument checks l0_ls_check -- meant to run under AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_l0_local_cpu.py builds and runs it both plainly and sanitized).  Checks are against
// a dense enumeration of all supports, the optimality conditions, or a certificate recomputed from the coefficients alone;
// never against another run of the code under test.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../sparse-lm_amd/csrc/l0_host.hpp"

using namespace slm;

static int failures = 0;
#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) {                                                            \
      fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__); \
      ++failures;                                                             \
    }                                                                         \
  } while (0)

// G = A^T A / n [p][ld] (the padding poisoned), c = A^T y / n, yy of an n x p design from a fixed recurrence with neighbouring
// columns correlated (rho); zero_col >= 0: that column of A is zero.
struct Problem {
  int p = 0;
  size_t ld = 0;
  std::vector<double> G, c;
  double yy = 0.0;
};
static Problem problem(int n, int p, size_t ld, double rho, int zero_col = -1) {
  Problem P;
  P.p = p;
  P.ld = ld;
  std::vector<double> A((size_t)n * p), y((size_t)n);
  unsigned v = 90210u;
  auto next = [&]() {
    v = v * 1103515245u + 12345u;
    return (double)((v >> 16) & 0x3ff) / 512.0 - 1.0;
  };
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < p; ++j) A[(size_t)i * p + j] = (j ? rho * A[(size_t)i * p + j - 1] : 0.0) + next();
  for (int i = 0; i < n && zero_col >= 0; ++i) A[(size_t)i * p + zero_col] = 0.0;
  for (int i = 0; i < n; ++i) {
    y[(size_t)i] = 0.5 * next();
    for (int j = 1; j < p; j += 3) y[(size_t)i] += ((j & 1) ? -1.0 : 1.0) * A[(size_t)i * p + j];
    P.yy += y[(size_t)i] * y[(size_t)i] / n;
  }
  P.G.assign((size_t)p * ld, NAN);  // (whoever reads the padding sees it in every result)
  P.c.assign((size_t)p, 0.0);
  for (int i = 0; i < p; ++i) {
    for (int j = 0; j < p; ++j) {
      double t = 0.0;
      for (int k = 0; k < n; ++k) t += A[(size_t)k * p + i] * A[(size_t)k * p + j];
      P.G[(size_t)i * ld + j] = t / n;
    }
    for (int k = 0; k < n; ++k) P.c[(size_t)i] += A[(size_t)k * p + i] * y[(size_t)k] / n;
  }
  return P;
}
static double Hij(const Problem& P, double eta, int i, int j) { return P.G[(size_t)i * P.ld + j] + (i == j ? 2.0 * eta : 0.0); }
static double objective(const Problem& P, double alpha, double eta, const double* b) {
  double F = 0.0;
  for (int i = 0; i < P.p; ++i) {
    if (b[i] == 0.0) continue;
    double t = 0.0;
    for (int j = 0; j < P.p; ++j) t += Hij(P, eta, i, j) * b[j];
    F += b[i] * (0.5 * t - P.c[(size_t)i]) + alpha;
  }
  return F;
}

// min over ALL supports of the unconstrained quadratic value + alpha |S| (Gaussian elimination per support; singular: skipped)
static double enumerate(const Problem& P, double alpha, double eta) {
  const int p = P.p;
  double best = 0.0;
  for (unsigned mask = 1; mask < (1u << p); ++mask) {
    int cols[16], m = 0;
    for (int j = 0; j < p; ++j)
      if (mask >> j & 1) cols[m++] = j;
    double M[16][17];
    for (int a = 0; a < m; ++a) {
      for (int b = 0; b < m; ++b) M[a][b] = Hij(P, eta, cols[a], cols[b]);
      M[a][m] = P.c[(size_t)cols[a]];
    }
    bool ok = true;
    for (int k = 0; k < m && ok; ++k) {
      int piv = k;
      for (int a = k + 1; a < m; ++a)
        if (fabs(M[a][k]) > fabs(M[piv][k])) piv = a;
      if (fabs(M[piv][k]) < 1e-12) ok = false;
      for (int b = 0; b <= m && ok; ++b) std::swap(M[k][b], M[piv][b]);
      for (int a = k + 1; a < m && ok; ++a) {
        const double f = M[a][k] / M[k][k];
        for (int b = k; b <= m; ++b) M[a][b] -= f * M[k][b];
      }
    }
    if (!ok) continue;
    double x[16], val = 0.0;
    for (int k = m - 1; k >= 0; --k) {
      double t = M[k][m];
      for (int b = k + 1; b < m; ++b) t -= M[k][b] * x[b];
      x[k] = t / M[k][k];
    }
    for (int a = 0; a < m; ++a) val -= 0.5 * x[a] * P.c[(size_t)cols[a]];  // the value at the minimiser: -1/2 c_S^T x
    best = fmin(best, val + alpha * m);
  }
  return best;
}

// From beta alone: every one-coordinate decision and (swaps) every (i, j) swap, recomputed; tol relative to the decision's scale.
static bool inescapable(const Problem& P, double alpha, double eta, double M, const double* beta, bool swaps, double tol) {
  const int p = P.p;
  std::vector<double> r((size_t)p), d((size_t)p);
  double dmax = 0.0;
  for (int i = 0; i < p; ++i) {
    d[(size_t)i] = Hij(P, eta, i, i);
    dmax = fmax(dmax, d[(size_t)i]);
    r[(size_t)i] = P.c[(size_t)i];
    for (int j = 0; j < p; ++j) r[(size_t)i] -= Hij(P, eta, i, j) * beta[j];
  }
  auto gain = [&](double u, double dj, double* b_out) {
    const double b = fmin(fmax(u / dj, -M), M);
    if (b_out) *b_out = b;
    return u * b - 0.5 * dj * b * b;
  };
  for (int j = 0; j < p; ++j) {
    if (!(d[(size_t)j] > 1e-12 * dmax)) {
      if (beta[j] != 0.0) return false;
      continue;
    }
    double b;
    const double g = gain(r[(size_t)j] + d[(size_t)j] * beta[j], d[(size_t)j], &b);
    if (beta[j] != 0.0 && (!(g > alpha - tol * fmax(g, alpha)) || fabs(b - beta[j]) > tol * fmax(fabs(b), 1.0))) return false;
    if (beta[j] == 0.0 && g > alpha + tol * fmax(g, alpha)) return false;
  }
  for (int i = 0; i < p && swaps; ++i) {
    if (beta[i] == 0.0) continue;
    const double gi = gain(r[(size_t)i] + d[(size_t)i] * beta[i], d[(size_t)i], nullptr);
    for (int j = 0; j < p; ++j) {
      if (beta[j] != 0.0 || !(d[(size_t)j] > 1e-12 * dmax)) continue;
      const double gj = gain(r[(size_t)j] + Hij(P, eta, j, i) * beta[i], d[(size_t)j], nullptr);
      if (gj > gi + (1e-10 + tol) * fmax(fabs(gi), alpha)) return false;
    }
  }
  return true;
}

static void test_against_enumeration() {
  int hits = 0, strictly = 0;
  for (int trial = 0; trial < 6; ++trial) {
    const int p = 10;
    const Problem P = problem(24, p, trial % 2 ? 13 : 10, 0.5 + 0.08 * trial);
    for (double rel : {0.002, 0.01, 0.05}) {
      const double alpha = rel * P.yy, eta = trial == 5 ? 0.05 : 0.0, M = 100.0;
      std::vector<double> b0((size_t)p), b1((size_t)p);
      const L0LsResult R0 = l0_local_solve<false>(P.G.data(), P.ld, P.c.data(), p, alpha, eta, M, P.yy, false, nullptr, b0.data());
      const L0LsResult R1 = l0_local_solve<false>(P.G.data(), P.ld, P.c.data(), p, alpha, eta, M, P.yy, true, nullptr, b1.data());
      const double exact = enumerate(P, alpha, eta), tol = 1e-9 * fmax(fabs(exact), alpha);
      CHECK(R0.status == 0 && R1.status == 0 && R0.swaps == 0);
      CHECK(fabs(R0.F - objective(P, alpha, eta, b0.data())) <= tol && fabs(R1.F - objective(P, alpha, eta, b1.data())) <= tol);
      CHECK(R1.F >= exact - tol);  // never below the optimum
      CHECK(R1.F <= R0.F + tol);   // swaps start from the descent's fixed point
      CHECK(inescapable(P, alpha, eta, M, b0.data(), false, 1e-8));
      CHECK(inescapable(P, alpha, eta, M, b1.data(), true, 1e-8));
      int nnz = 0;
      for (int j = 0; j < p; ++j) nnz += b1[(size_t)j] != 0.0;
      CHECK(nnz == R1.nnz);
      hits += fabs(R1.F - exact) <= tol;
      strictly += R1.F < R0.F - tol;
      // the polish: the exact minimiser on the support, and no worse than what it was given
      std::vector<double> bp = b1;
      const double quad = l0_ls_polish(P.G.data(), P.ld, P.c.data(), p, eta, M, bp.data());
      CHECK(quad + alpha * nnz <= R1.F + tol && fabs(quad + alpha * nnz - objective(P, alpha, eta, bp.data())) <= tol);
      for (int j = 0; j < p; ++j) {
        CHECK((bp[(size_t)j] != 0.0) == (b1[(size_t)j] != 0.0));
        if (bp[(size_t)j] == 0.0) continue;
        double g = -P.c[(size_t)j];
        for (int k = 0; k < p; ++k) g += Hij(P, eta, j, k) * bp[(size_t)k];
        CHECK(fabs(g) <= 1e-12 * sqrt(P.yy));  // stationary on the support
      }
    }
  }
  CHECK(hits >= 1);  // (the search is not required to be exact; that it never is would be a bug)
  printf("  enumeration: %d of 18 at the optimum, swaps strictly better in %d\n", hits, strictly);
}

static void test_box() {
  const int p = 10;
  const Problem P = problem(24, p, 12, 0.6);
  const double alpha = 0.002 * P.yy, M = 0.4;
  std::vector<double> b((size_t)p);
  const L0LsResult R = l0_local_solve<false>(P.G.data(), P.ld, P.c.data(), p, alpha, 0.0, M, P.yy, true, nullptr, b.data());
  CHECK(R.status == 0);
  int bound = 0;
  for (int j = 0; j < p; ++j) {
    CHECK(fabs(b[(size_t)j]) <= M);
    bound += fabs(b[(size_t)j]) == M;
  }
  CHECK(bound >= 1);  // the box binds on an active coordinate
  CHECK(inescapable(P, alpha, 0.0, M, b.data(), true, 1e-8));
  std::vector<double> bp = b;
  const double quad = l0_ls_polish(P.G.data(), P.ld, P.c.data(), p, 0.0, M, bp.data());
  CHECK(quad + alpha * R.nnz <= R.F + 1e-12 * fabs(R.F));
  for (int j = 0; j < p; ++j) {  // the optimality conditions of the box on the support
    CHECK(fabs(bp[(size_t)j]) <= M && (bp[(size_t)j] != 0.0) == (b[(size_t)j] != 0.0));
    if (bp[(size_t)j] == 0.0) continue;
    double g = -P.c[(size_t)j];
    for (int k = 0; k < p; ++k) g += Hij(P, 0.0, j, k) * bp[(size_t)k];
    if (bp[(size_t)j] == M) CHECK(g <= 1e-10);
    else if (bp[(size_t)j] == -M) CHECK(g >= -1e-10);
    else CHECK(fabs(g) <= 1e-10);
  }
}

static void test_zero_column_and_singular() {
  const int p = 10;
  const Problem Z = problem(24, p, 10, 0.5, 4);  // column 4 (a true one) is zero: d_4 = 0, it stays out and nothing divides by it
  std::vector<double> b((size_t)p);
  L0LsResult R = l0_local_solve<false>(Z.G.data(), Z.ld, Z.c.data(), p, 0.0, 0.0, 100.0, Z.yy, true, nullptr, b.data());
  CHECK(R.status == 0 && b[4] == 0.0 && std::isfinite(R.F) && R.nnz == p - 1);  // (alpha = 0: every live column enters)
  for (int j = 0; j < p; ++j) CHECK(std::isfinite(b[(size_t)j]));
  std::vector<double> st((size_t)p, 0.0);
  st[4] = 1.0;  // a start ON the dead column is dropped
  R = l0_local_solve<false>(Z.G.data(), Z.ld, Z.c.data(), p, 0.01 * Z.yy, 0.0, 100.0, Z.yy, true, st.data(), b.data());
  CHECK(R.status == 0 && b[4] == 0.0 && inescapable(Z, 0.01 * Z.yy, 0.0, 100.0, b.data(), true, 1e-8));
  // n < p: G is singular, eta > 0 makes H definite
  const Problem S = problem(5, p, 11, 0.3);
  const double eta = 0.05, alpha = 0.01 * S.yy;
  R = l0_local_solve<false>(S.G.data(), S.ld, S.c.data(), p, alpha, eta, 100.0, S.yy, true, nullptr, b.data());
  CHECK(R.status == 0 && std::isfinite(R.F) && R.F < 0.0);
  CHECK(fabs(R.F - objective(S, alpha, eta, b.data())) <= 1e-10 * fabs(R.F));
  CHECK(inescapable(S, alpha, eta, 100.0, b.data(), true, 1e-8));
  CHECK(R.F >= enumerate(S, alpha, eta) - 1e-10 * fabs(R.F));
}

static void test_wrong_start() {
  const int p = 10;
  const Problem P = problem(24, p, 10, 0.7);
  const double alpha = 0.01 * P.yy;
  std::vector<double> st((size_t)p, 0.0), b((size_t)p), b0((size_t)p);
  st[0] = 3.0; st[2] = -2.0; st[9] = 1.5;  // none of the true columns 1, 4, 7
  const double F_start = objective(P, alpha, 0.0, st.data());
  const L0LsResult R = l0_local_solve<false>(P.G.data(), P.ld, P.c.data(), p, alpha, 0.0, 100.0, P.yy, true, st.data(), b.data());
  CHECK(R.status == 0 && R.F <= F_start && R.F < 0.0);
  CHECK(fabs(R.F - objective(P, alpha, 0.0, b.data())) <= 1e-10 * fabs(R.F));
  CHECK(inescapable(P, alpha, 0.0, 100.0, b.data(), true, 1e-8));
  CHECK(st[0] == 3.0 && st[2] == -2.0 && st[9] == 1.5);  // the start is read, not written
  CHECK(R.F >= enumerate(P, alpha, 0.0) - 1e-10 * fabs(R.F));
  // an alpha above every gain empties the support, from a start too
  const L0LsResult E = l0_local_solve<false>(P.G.data(), P.ld, P.c.data(), p, 10.0 * P.yy, 0.0, 100.0, P.yy, true, st.data(), b0.data());
  CHECK(E.status == 0 && E.nnz == 0 && E.F == 0.0);
  for (int j = 0; j < p; ++j) CHECK(b0[(size_t)j] == 0.0);
}

static void test_checks() {
  const double ok[2] = {0.1, 0.0}, neg[2] = {0.1, -1.0}, nan_[2] = {NAN, 0.0}, inf_[2] = {0.1, INFINITY};
  const double st[4] = {0.0, 1.0, -2.0, 0.5};
  long long which = -1;
  CHECK(l0_ls_check(2, ok, ok, 1.0, 1, nullptr, 2) == L0_LS_OK);
  CHECK(l0_ls_check(2, nullptr, ok, 1.0, 1, nullptr, 2) == L0_LS_NULL && l0_ls_check(2, ok, nullptr, 1.0, 1, nullptr, 2) == L0_LS_NULL);
  CHECK(l0_ls_check(0, ok, ok, 1.0, 1, nullptr, 2) == L0_LS_CELLS && l0_ls_check(-3, ok, ok, 1.0, 1, nullptr, 2) == L0_LS_CELLS);
  CHECK(l0_ls_check(2, ok, ok, 1.0, 0, nullptr, 2) == L0_LS_STARTS);
  CHECK(l0_ls_check(L0_LS_MAX_PROBLEMS, ok, ok, 1.0, 2, nullptr, 2) == L0_LS_PROBLEMS);  // (before the arrays are read)
  CHECK(l0_ls_check(1ll << 40, ok, ok, 1.0, 1ll << 40, nullptr, 2) == L0_LS_PROBLEMS);
  CHECK(l0_ls_check(2, ok, ok, -1.0, 1, nullptr, 2) == L0_LS_BIG_M && l0_ls_check(2, ok, ok, NAN, 1, nullptr, 2) == L0_LS_BIG_M);
  CHECK(l0_ls_check(2, neg, ok, 1.0, 1, nullptr, 2, &which) == L0_LS_ALPHA && which == 1);
  CHECK(l0_ls_check(2, nan_, ok, 1.0, 1, nullptr, 2, &which) == L0_LS_ALPHA && which == 0);
  CHECK(l0_ls_check(2, ok, inf_, 1.0, 1, nullptr, 2, &which) == L0_LS_ETA && which == 1);
  CHECK(l0_ls_check(2, ok, ok, 1.0, 1, nullptr, L0_LS_PMAX) == L0_LS_OK && l0_ls_check(2, ok, ok, 1.0, 1, nullptr, L0_LS_PMAX + 1) == L0_LS_WIDTH);
  CHECK(l0_ls_check(2, ok, ok, 2.0, 1, st, 2) == L0_LS_OK);
  CHECK(l0_ls_check(2, ok, ok, 1.0, 1, st, 2, &which) == L0_LS_START_BOX && which == 2);
  CHECK(l0_ls_check(1, ok, ok, 1.0, 2, nan_, 1, &which) == L0_LS_START_BOX && which == 0);
  CHECK(L0_LS_SLOTS * 64 == L0_LS_PMAX);
}

int main() {
  test_against_enumeration();
  test_box();
  test_zero_column_and_singular();
  test_wrong_start();
  test_checks();
  if (failures) {
    fprintf(stderr, "l0_local_host_test: %d failure(s)\n", failures);
    return 1;
  }
  printf("l0_local_host_test: ok\n");
  return 0;
}
