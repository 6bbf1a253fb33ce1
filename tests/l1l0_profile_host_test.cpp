// CPU test of the host side of the l1 profile (slm_solve_l0_l1_profile, slm_solve_l0_l1_profile_wide) in csrc/l0_host.hpp:
// the lasso of one support for a mask of either width (l0_l1_support_of), the lasso dual bound on up to 128 columns
// (l0_l1_lower_bound) and the profile's pruning rule run with that bound in place of q_all -- meant to run under
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_l1l0_profile_cpu.py builds and runs it both plainly and
// sanitized).  Checks are against the narrow function that was there, a dense solve, the optimality conditions, or a full
// enumeration; never against another run of the code under test.
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

static bool near(double got, double want, double tol) { return fabs(got - want) <= tol * fmax(1.0, fabs(want)); }

// H = A^T A / n + ridge I and c = A^T y / n of an n x p design from a fixed recurrence: positive definite, dense.
static void problem(int n, int p, double ridge, std::vector<double>& H, std::vector<double>& c) {
  std::vector<double> A((size_t)n * p), y((size_t)n);
  unsigned v = 4711u;
  auto next = [&]() {
    v = v * 1103515245u + 12345u;
    return (double)((v >> 16) & 0x3ff) / 512.0 - 1.0;
  };
  for (double& a : A) a = next();
  for (int i = 0; i < n; ++i) {
    y[(size_t)i] = 0.3 * next();
    for (int j = 0; j < p; j += 7) y[(size_t)i] += (1.0 + 0.1 * j) * ((j & 1) ? -1.0 : 1.0) * A[(size_t)i * p + j];
  }
  H.assign((size_t)p * p, 0.0);
  c.assign((size_t)p, 0.0);
  for (int i = 0; i < p; ++i) {
    for (int j = 0; j < p; ++j) {
      double t = 0.0;
      for (int k = 0; k < n; ++k) t += A[(size_t)k * p + i] * A[(size_t)k * p + j];
      H[(size_t)i * p + j] = t / n + (i == j ? ridge : 0.0);
    }
    double t = 0.0;
    for (int k = 0; k < n; ++k) t += A[(size_t)k * p + i] * y[(size_t)k];
    c[(size_t)i] = t / n;
  }
}

// The largest violation of the optimality conditions of min 1/2 b^T H b - c^T b + eta ||b||_1 over |b_j| <= M on `cols`.
static double kkt(const double* H, const double* c, int p, const int* cols, int m, double eta, double M, const double* b) {
  double worst = 0.0;
  for (int r = 0; r < m; ++r) {
    double g = -c[cols[r]];
    for (int k = 0; k < m; ++k) g += H[(size_t)cols[r] * p + cols[k]] * b[k];
    double v;
    if (b[r] == 0.0) v = fmax(fabs(g) - eta, 0.0);
    else if (b[r] >= M) v = fmax(g + eta, 0.0);
    else if (b[r] <= -M) v = fmax(eta - g, 0.0);
    else v = fabs(g + (b[r] > 0.0 ? eta : -eta));
    worst = fmax(worst, v);
  }
  return worst;
}

static void test_generic_is_the_narrow_one() {
  // 12 columns in groups of sizes 1, 3, 2, 4, 2 (one of them holds a duplicated column: the pivot rule skips it, the descent keeps it)
  const int p = 12;
  std::vector<double> H, c;
  problem(30, p, 0.0, H, c);
  for (int i = 0; i < p; ++i) {  // column 5 := column 4 (same group)
    c[5] = c[4];
    H[(size_t)i * p + 5] = H[(size_t)i * p + 4];
  }
  for (int j = 0; j < p; ++j) H[(size_t)5 * p + j] = H[(size_t)j * p + 5];
  H[5 * p + 5] = H[4 * p + 4];
  const std::vector<int> gstart = {0, 1, 4, 6, 10, 12};
  std::vector<double> b0((size_t)p), b1((size_t)p), b2((size_t)p);
  for (unsigned long long mask = 0; mask < 32; ++mask)
    for (double eta : {0.0, 0.02, 0.3})
      for (double M : {100.0, 0.2})
        for (int polish = 0; polish < 2; ++polish) {
          bool o1 = true, o2 = true;
          const double v0 = l0_l1_support(H.data(), c.data(), p, gstart, mask, eta, M, polish != 0, b0.data());
          const double v1 = l0_l1_support_of(H.data(), c.data(), p, gstart, mask, eta, M, polish != 0, b1.data(), &o1);
          const double v2 = l0_l1_support_of(H.data(), c.data(), p, gstart, L0Mask128{mask, 0ull}, eta, M, polish != 0, b2.data(), &o2);
          CHECK(memcmp(&v0, &v1, sizeof(double)) == 0 && memcmp(&v0, &v2, sizeof(double)) == 0);
          CHECK(memcmp(b0.data(), b1.data(), sizeof(double) * p) == 0 && memcmp(b0.data(), b2.data(), sizeof(double) * p) == 0);
          CHECK(!o1 && !o2);
        }
}

static void test_support_across_the_word_boundary() {
  const int p = 100;
  std::vector<double> H, c;
  problem(140, p, 0.05, H, c);
  std::vector<int> gstart((size_t)p + 1);
  for (int j = 0; j <= p; ++j) gstart[(size_t)j] = j;
  const int cols[6] = {3, 40, 63, 64, 70, 99};
  L0Mask128 mask = l0m_none<L0Mask128>();
  for (int j : cols) l0m_set(mask, j);
  std::vector<double> beta((size_t)p);
  double cmax = 0.0;
  for (int j : cols) cmax = fmax(cmax, fabs(c[(size_t)j]));
  for (double rel : {0.01, 0.4}) {
    const double eta = rel * cmax;
    bool over = true;
    const double v = l0_l1_support_of(H.data(), c.data(), p, gstart, mask, eta, 100.0, true, beta.data(), &over);
    CHECK(!over);
    double b[6];
    int nz = 0;
    for (int r = 0; r < 6; ++r) {
      b[r] = beta[(size_t)cols[r]];
      nz += b[r] != 0.0;
    }
    for (int j = 0; j < p; ++j) {  // nothing outside the support
      bool in = false;
      for (int r = 0; r < 6; ++r) in = in || cols[r] == j;
      if (!in) CHECK(beta[(size_t)j] == 0.0);
    }
    CHECK(near(l0_l1_value(H.data(), c.data(), p, cols, 6, eta, b), v, 1e-14));
    CHECK(kkt(H.data(), c.data(), p, cols, 6, eta, 100.0, b) <= 1e-12);
    // the dense solve on the sign pattern: H_FF x = c_F - eta sign(b_F), Gaussian elimination with partial pivoting
    std::vector<int> F;
    for (int r = 0; r < 6; ++r)
      if (b[r] != 0.0) F.push_back(r);
    const int f = (int)F.size();
    CHECK(f == nz && f >= 1);
    if (rel < 0.1) CHECK(f == 6);  // (a small eta zeroes nothing here: the dense solve covers the whole support)
    std::vector<double> M((size_t)f * (f + 1));
    for (int i = 0; i < f; ++i) {
      for (int j = 0; j < f; ++j) M[(size_t)i * (f + 1) + j] = H[(size_t)cols[F[(size_t)i]] * p + cols[F[(size_t)j]]];
      M[(size_t)i * (f + 1) + f] = c[(size_t)cols[F[(size_t)i]]] - (b[F[(size_t)i]] > 0.0 ? eta : -eta);
    }
    for (int k = 0; k < f; ++k) {
      int piv = k;
      for (int i = k + 1; i < f; ++i)
        if (fabs(M[(size_t)i * (f + 1) + k]) > fabs(M[(size_t)piv * (f + 1) + k])) piv = i;
      for (int j = 0; j <= f; ++j) std::swap(M[(size_t)k * (f + 1) + j], M[(size_t)piv * (f + 1) + j]);
      for (int i = k + 1; i < f; ++i) {
        const double t = M[(size_t)i * (f + 1) + k] / M[(size_t)k * (f + 1) + k];
        for (int j = k; j <= f; ++j) M[(size_t)i * (f + 1) + j] -= t * M[(size_t)k * (f + 1) + j];
      }
    }
    for (int i = f - 1; i >= 0; --i) {
      double t = M[(size_t)i * (f + 1) + f];
      for (int j = i + 1; j < f; ++j) t -= M[(size_t)i * (f + 1) + j] * M[(size_t)j * (f + 1) + f];
      M[(size_t)i * (f + 1) + f] = t / M[(size_t)i * (f + 1) + i];
    }
    for (int i = 0; i < f; ++i) CHECK(near(b[F[(size_t)i]], M[(size_t)i * (f + 1) + f], 1e-12));
  }
  // 64 columns fit, a 65th sets overflow and is left out; nothing is written past the arrays (the sanitizers watch)
  L0Mask128 m64 = l0m_none<L0Mask128>(), m65;
  for (int j = 30; j < 94; ++j) l0m_set(m64, j);
  m65 = m64;
  l0m_set(m65, 97);
  bool over = true;
  const double v64 = l0_l1_support_of(H.data(), c.data(), p, gstart, m64, 0.1 * cmax, 100.0, true, beta.data(), &over);
  CHECK(!over && v64 < 0.0);
  const double v65 = l0_l1_support_of(H.data(), c.data(), p, gstart, m65, 0.1 * cmax, 100.0, true, beta.data(), &over);
  CHECK(over && v65 == v64 && beta[97] == 0.0);
}

static void test_lower_bound_at_100_columns() {
  const int p = 100;
  std::vector<double> H, c;
  problem(140, p, 0.0, H, c);
  const double q_all = l0_q_all(H.data(), c.data(), p);
  const double yy = -2.0 * q_all + 0.5;  // c^T H^-1 c plus a residual's share: a consistent (H, c, yy)
  std::vector<int> cols((size_t)p);
  for (int j = 0; j < p; ++j) cols[(size_t)j] = j;
  double cmax = 0.0;
  for (double v : c) cmax = fmax(cmax, fabs(v));
  CHECK(l0_l1_lower_bound(H.data(), c.data(), p, yy, 0.0, q_all) == q_all);
  double last = q_all;
  for (double rel : {1e-3, 0.05, 0.3, 0.9}) {
    const double eta = rel * cmax;
    std::vector<double> b((size_t)p, 0.0);
    const double primal = l0_l1_descent(H.data(), c.data(), p, cols.data(), p, eta, HUGE_VAL, b.data());
    const double lb = l0_l1_lower_bound(H.data(), c.data(), p, yy, eta, q_all);
    CHECK(lb >= q_all && lb <= primal);
    CHECK(lb > q_all);                                            // (beyond 64 columns it was q_all itself)
    CHECK(primal - lb <= 1e-6 * fabs(primal) + 1e-8 * (yy - 2.0 * q_all));  // tight: the descent's point is nearly optimal
    CHECK(lb >= last - 1e-9 * yy);
    last = lb;
  }
  // the limits: 128 columns are taken, 129 fall back to q_all (and touch nothing)
  CHECK(l0_l1_lower_bound(H.data(), c.data(), L0_WIDE_PMAX + 1, yy, 0.1, q_all) == q_all);
}

// The profile search on the host: a sequential depth-first walk over the supports of 6 singleton groups, a node of cnt groups
// a candidate for row cnt, its value the lasso of the support, the subtree cut l0_profile_cut with `bound` for q_all.
struct Table {
  double q[7];
  long long nodes = 0;
};
static void dfs(const double* H, const double* c, const std::vector<int>& gstart, double eta, int depth, int cnt, unsigned long long incl,
                double bound, double alpha_min, bool prune, Table& t) {
  if (depth >= 6) return;
  if (prune && l0_profile_cut(bound, alpha_min, cnt, l0_profile_envelope(t.q + 1, cnt, alpha_min))) return;
  const unsigned long long mk = incl | (1ull << depth);
  double beta[6];
  const double v = l0_l1_support_of(H, c, 6, gstart, mk, eta, 100.0, false, beta);
  ++t.nodes;
  if (v < t.q[cnt + 1]) t.q[cnt + 1] = v;
  dfs(H, c, gstart, eta, depth + 1, cnt + 1, mk, bound, alpha_min, prune, t);
  dfs(H, c, gstart, eta, depth + 1, cnt, incl, bound, alpha_min, prune, t);
}

static void test_cut_with_an_l1_bound_against_enumeration() {
  const int p = 6;
  std::vector<double> H, c;
  problem(20, p, 0.0, H, c);
  const std::vector<int> gstart = {0, 1, 2, 3, 4, 5, 6};
  const double q_all = l0_q_all(H.data(), c.data(), p);
  const double yy = -2.0 * q_all + 0.1;
  double cmax = 0.0;
  for (double v : c) cmax = fmax(cmax, fabs(v));
  for (double rel : {0.02, 0.2, 0.5}) {
    const double eta = rel * cmax;
    // the enumeration: F_k over all 63 supports
    double F[7];
    F[0] = 0.0;
    for (int k = 1; k <= 6; ++k) F[k] = HUGE_VAL;
    double f_all = 0.0;
    for (unsigned long long mask = 1; mask < 64; ++mask) {
      double beta[6];
      const double v = l0_l1_support_of(H.data(), c.data(), p, gstart, mask, eta, 100.0, false, beta);
      const int k = __builtin_popcountll(mask);
      if (v < F[k]) F[k] = v;
      if (mask == 63) f_all = v;
    }
    for (int k = 1; k < 6; ++k) CHECK(F[k + 1] <= F[k] + 1e-12);  // f is monotone in the support, so the best of a size is too
    const double bound = l0_l1_lower_bound(H.data(), c.data(), p, yy, eta, q_all);
    CHECK(bound >= q_all && bound <= f_all);
    // alpha_min = 0: the table is the full one
    Table full;
    full.q[0] = 0.0;
    for (int k = 1; k <= 6; ++k) full.q[k] = HUGE_VAL;
    dfs(H.data(), c.data(), gstart, eta, 0, 0, 0ull, bound, 0.0, true, full);
    for (int k = 1; k <= 6; ++k) CHECK(full.q[k] == F[k]);
    // alpha_min > 0: fewer nodes, and every alpha >= alpha_min reads the optimum of the full table
    for (double am : {0.01 * fabs(f_all), 0.1 * fabs(f_all), 0.5 * fabs(f_all)}) {
      Table t;
      t.q[0] = 0.0;
      for (int k = 1; k <= 6; ++k) t.q[k] = HUGE_VAL;
      dfs(H.data(), c.data(), gstart, eta, 0, 0, 0ull, bound, am, true, t);
      CHECK(t.nodes <= full.nodes);
      for (double mult : {1.0, 1.5, 4.0, 50.0}) {
        const double alpha = am * mult;
        const int kf = l0_profile_regularized(F, 6, alpha), kt = l0_profile_regularized(t.q, 6, alpha);
        CHECK(near(t.q[kt] + alpha * kt, F[kf] + alpha * kf, 1e-14));  // (the sizes may differ only in an exact tie)
      }
    }
    // the l1 bound cuts at least as early as q_all does (it is the larger of the two)
    Table tq, tb;
    for (Table* t : {&tq, &tb}) {
      t->q[0] = 0.0;
      for (int k = 1; k <= 6; ++k) t->q[k] = HUGE_VAL;
    }
    dfs(H.data(), c.data(), gstart, eta, 0, 0, 0ull, q_all, 0.1 * fabs(f_all), true, tq);
    dfs(H.data(), c.data(), gstart, eta, 0, 0, 0ull, bound, 0.1 * fabs(f_all), true, tb);
    CHECK(tb.nodes <= tq.nodes);
  }
}

int main() {
  test_generic_is_the_narrow_one();
  test_support_across_the_word_boundary();
  test_lower_bound_at_100_columns();
  test_cut_with_an_l1_bound_against_enumeration();
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("l1l0_profile_host_test: ok\n");
  return 0;
}
