// CPU test of the host side of local subsets (slm_solve_l0_local_subsets) in csrc/l0_host.hpp: the argument check l0_lc_check
// with every refusal and their order, the problem index and the six-word status rows, and the host twin of the kernel's
// cardinality rule l0_local_solve<true> -- against enumeration of every support, against a certificate recomputed from beta alone, from
// starts that are too large and too small, at k >= p with a dead column, in a binding box, at a leading dimension with NaN
// padding -- and l0_ls_polish on its results.  Meant to run under AddressSanitizer and UndefinedBehaviorSanitizer
// (tests/test_l0_local_subsets_cpu.py builds and runs it both plainly and sanitized).
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

// the Gram [p][ld] (padding NaN), c and yy of an n x p design from a fixed recurrence with strongly correlated neighbours;
// column `dead` (if >= 0) is all zero
struct Problem {
  int p = 0;
  size_t ld = 0;
  std::vector<double> G, c;
  double yy = 0.0;
};
static Problem problem(int n, int p, size_t ld, int dead, unsigned seed) {
  std::vector<double> A((size_t)n * p), y((size_t)n);
  unsigned v = seed;
  auto next = [&]() {
    v = v * 1103515245u + 12345u;
    return (double)((v >> 16) & 0x3ff) / 512.0 - 1.0;
  };
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < p; ++j) A[(size_t)i * p + j] = j == dead ? 0.0 : (j && j - 1 != dead ? 0.8 * A[(size_t)i * p + j - 1] : 0.0) + 0.6 * next();
    y[(size_t)i] = 0.4 * next();
    for (int j = 1; j < p; j += 3) y[(size_t)i] += ((j & 2) ? -1.0 : 1.0) * A[(size_t)i * p + j];
  }
  Problem P;
  P.p = p;
  P.ld = ld;
  P.G.assign((size_t)p * ld, NAN);
  P.c.assign((size_t)p, 0.0);
  for (int a = 0; a < p; ++a) {
    for (int b = 0; b < p; ++b) {
      double s = 0.0;
      for (int i = 0; i < n; ++i) s += A[(size_t)i * p + a] * A[(size_t)i * p + b];
      P.G[(size_t)a * ld + b] = s / n;
    }
    for (int i = 0; i < n; ++i) P.c[(size_t)a] += A[(size_t)i * p + a] * y[(size_t)i] / n;
  }
  for (int i = 0; i < n; ++i) P.yy += y[(size_t)i] * y[(size_t)i] / n;
  return P;
}

static double quadratic(const Problem& P, double eta, const double* beta) {
  double q = 0.0;
  for (int a = 0; a < P.p; ++a) {
    double t = 0.0;
    for (int b = 0; b < P.p; ++b) t += (P.G[(size_t)a * P.ld + b] + (a == b ? 2.0 * eta : 0.0)) * beta[b];
    q += beta[a] * (0.5 * t - P.c[(size_t)a]);
  }
  return q;
}

// the optimum over every support of at most k columns of the first p <= 16 (the box not binding): Cholesky per support
static double enumerate(const Problem& P, int k, double eta) {
  double best = 0.0;
  for (unsigned mask = 1; mask < (1u << P.p); ++mask) {
    if (__builtin_popcount(mask) > k) continue;
    std::vector<int> cols;
    for (int j = 0; j < P.p; ++j)
      if (mask >> j & 1) cols.push_back(j);
    const int m = (int)cols.size();
    std::vector<double> M((size_t)m * m), x((size_t)m);
    for (int a = 0; a < m; ++a) {
      x[(size_t)a] = P.c[(size_t)cols[(size_t)a]];
      for (int b = 0; b < m; ++b) M[(size_t)a * m + b] = P.G[(size_t)cols[(size_t)a] * P.ld + cols[(size_t)b]] + (a == b ? 2.0 * eta : 0.0);
    }
    if (!l0_dense_chol(M, m)) continue;
    l0_dense_fwd(M, m, x.data());
    l0_dense_bwd(M, m, x.data());
    double val = 0.0;
    for (int a = 0; a < m; ++a) val -= 0.5 * P.c[(size_t)cols[(size_t)a]] * x[(size_t)a];
    best = std::min(best, val);
  }
  return best;
}

// from beta alone: nnz <= k, inside the box, every active coordinate at its one-coordinate value, below k nothing would enter,
// and (swaps) no column outside beats a column inside with that one removed
static bool inescapable(const Problem& P, int k, double eta, double big_M, const double* beta, bool swaps, double slack) {
  const int p = P.p;
  std::vector<double> r((size_t)p), d((size_t)p);
  double dmax = 0.0;
  int nnz = 0;
  for (int a = 0; a < p; ++a) {
    d[(size_t)a] = P.G[(size_t)a * P.ld + a] + 2.0 * eta;
    dmax = std::max(dmax, d[(size_t)a]);
    double t = 0.0;
    for (int b = 0; b < p; ++b) t += (P.G[(size_t)a * P.ld + b] + (a == b ? 2.0 * eta : 0.0)) * beta[b];
    r[(size_t)a] = P.c[(size_t)a] - t;
    nnz += beta[a] != 0.0;
    if (fabs(beta[a]) > big_M) return false;
  }
  if (nnz > k) return false;
  const double tol = (L0_CD_TOL + slack) * sqrt(P.yy);
  for (int j = 0; j < p; ++j) {
    const bool live = d[(size_t)j] > L0_PIVOT * dmax;
    if (!live) {
      if (beta[j] != 0.0) return false;
      continue;
    }
    if (beta[j] != 0.0) {
      const double b = l0_ls_coord(r[(size_t)j] + d[(size_t)j] * beta[j], d[(size_t)j], big_M).b;
      if (fabs(b - beta[j]) > slack * std::max(fabs(b), fabs(beta[j]))) return false;
    } else if (nnz < k && fabs(l0_ls_coord(r[(size_t)j], d[(size_t)j], big_M).b) * sqrt(d[(size_t)j]) > tol) {
      return false;
    }
  }
  for (int i = 0; i < p && swaps; ++i) {
    if (beta[i] == 0.0) continue;
    const double gi = l0_ls_coord(r[(size_t)i] + d[(size_t)i] * beta[i], d[(size_t)i], big_M).gain;
    for (int j = 0; j < p; ++j) {
      if (beta[j] != 0.0 || !(d[(size_t)j] > L0_PIVOT * dmax)) continue;
      const double gj = l0_ls_coord(r[(size_t)j] + P.G[(size_t)i * P.ld + j] * beta[i], d[(size_t)j], big_M).gain;
      if (gj > gi + (L0_LS_SWAP_TOL + slack) * fabs(gi)) return false;
    }
  }
  return true;
}

static void test_check() {
  const int sz[3] = {1, 4, 9};
  const double et[3] = {0.0, 0.5, 0.0};
  const double w0[4] = {1.0, 0.0, 2.0, 1.0}, w1[4] = {1.0, 1.0, 1.0, 1.0};
  const double* rw[3] = {w0, nullptr, w1};
  const long long ne[3] = {3, 0, 4};
  auto check = [&](long long count, const double* const* rws, const long long* nes, bool icpt, bool alone, long long cells, const int* s,
                   const double* e, double M, long long starts_n, const double* st, long long p) {
    return l0_lc_check(count, rws, nes, 4, icpt, alone, cells, s, e, M, starts_n, st, p);
  };
  CHECK(check(3, rw, ne, false, true, 3, sz, et, 1.0, 1, nullptr, 5).kind == L0_LC_OK);  // (a size above p is legal)
  CHECK(check(3, rw, ne, true, true, 3, sz, et, 1.0, 1, nullptr, 5).kind == L0_LC_OK);
  // NULL sizes or etas first, before the count and everything else
  CHECK(check(0, nullptr, nullptr, false, true, 3, nullptr, et, -1.0, 0, nullptr, 5000).kind == L0_LC_NULL);
  CHECK(check(0, nullptr, nullptr, false, true, 3, sz, nullptr, -1.0, 0, nullptr, 5000).kind == L0_LC_NULL);
  // then a size < 1, before a bad eta
  const int bad_sz[3] = {2, 0, -1};
  const double bad_et[3] = {-0.1, 0.0, INFINITY};
  L0LcRefusal R = check(0, nullptr, nullptr, false, true, 3, bad_sz, bad_et, -1.0, 0, nullptr, 5000);
  CHECK(R.kind == L0_LC_SIZE && R.which == 1);
  R = check(0, nullptr, nullptr, false, true, 3, sz, bad_et, -1.0, 0, nullptr, 5000);
  CHECK(R.kind == L0_LC_ETA && R.which == 0);
  const double nan_et[3] = {0.0, 0.0, NAN};
  R = check(3, rw, ne, false, true, 3, sz, nan_et, 1.0, 1, nullptr, 5);
  CHECK(R.kind == L0_LC_ETA && R.which == 2);
  // then l0_lsf_check's, in its order: the count, NULL tables, the problem counts, big_M, the width, the intercept, weights, box
  R = check(0, nullptr, nullptr, false, true, 3, sz, et, -1.0, 0, nullptr, 5000);
  CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_COUNT);
  R = check(17, rw, ne, false, true, 3, sz, et, 1.0, 1, nullptr, 5);
  CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_COUNT);
  R = check(3, nullptr, ne, false, true, 3, sz, et, -1.0, 0, nullptr, 5000);
  CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_NULL);
  R = check(3, rw, nullptr, false, true, 3, sz, et, -1.0, 0, nullptr, 5000);
  CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_NULL);
  R = check(3, rw, ne, false, true, 0, sz, et, -1.0, 0, nullptr, 5000);
  CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_LS && R.lsf.ls == L0_LS_CELLS);
  R = check(3, rw, ne, false, true, 3, sz, et, -1.0, 0, nullptr, 5000);
  CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_LS && R.lsf.ls == L0_LS_STARTS);
  {
    std::vector<int> s((size_t)L0_LS_MAX_PROBLEMS + 1, 2);
    std::vector<double> e((size_t)L0_LS_MAX_PROBLEMS + 1, 0.0);
    const double* sixteen[16] = {};
    const long long n16[16] = {};
    CHECK(check(16, sixteen, n16, false, true, 512, s.data(), e.data(), 1.0, 1, nullptr, 5).kind == L0_LC_OK);
    R = check(16, sixteen, n16, false, true, 513, s.data(), e.data(), -1.0, 1, nullptr, 5000);
    CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_PRODUCT);
    R = check(1, sixteen, n16, false, true, L0_LS_MAX_PROBLEMS + 1, s.data(), e.data(), 1.0, 1, nullptr, 5);
    CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_PRODUCT);
    R = check(2, sixteen, n16, false, true, 64, s.data(), e.data(), 1.0, 65, nullptr, 5);
    CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_PRODUCT);
  }
  R = check(3, rw, ne, false, true, 3, sz, et, -1.0, 1, nullptr, 5000);
  CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_LS && R.lsf.ls == L0_LS_BIG_M);
  R = check(3, rw, ne, false, true, 3, sz, et, NAN, 1, nullptr, 5);
  CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_LS && R.lsf.ls == L0_LS_BIG_M);
  R = check(3, rw, ne, false, false, 3, sz, et, 1.0, 1, nullptr, L0_LS_PMAX + 1);
  CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_LS && R.lsf.ls == L0_LS_WIDTH);
  CHECK(check(3, rw, ne, true, true, 3, sz, et, 1.0, 1, nullptr, L0_LS_PMAX + 1).kind == L0_LC_OK);  // (1024 beside the ones column)
  R = check(3, rw, ne, true, true, 3, sz, et, 1.0, 1, nullptr, L0_LS_PMAX + 2);
  CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_LS && R.lsf.ls == L0_LS_WIDTH);
  const double wbad[4] = {1.0, -1.0, 1.0, 1.0};
  const double* rwbad[3] = {w0, nullptr, wbad};
  const double outside[3 * 3 * 5] = {0.0, 0.0, 2.0};
  R = check(3, rwbad, ne, true, false, 3, sz, et, 1.0, 1, outside, 5);
  CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_INTERCEPT);
  R = check(3, rwbad, ne, false, true, 3, sz, et, 1.0, 1, outside, 5);
  CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_WEIGHT && R.lsf.row_set == 2 && R.lsf.which == 1);
  R = check(3, rw, ne, false, true, 3, sz, et, 1.0, 1, outside, 5);
  CHECK(R.kind == L0_LC_LSF && R.lsf.kind == L0_LSF_LS && R.lsf.ls == L0_LS_START_BOX && R.lsf.which == 2);
  std::vector<double> nanstart(3 * 3 * 4, 0.0);  // (with an intercept the starts have ps = p - 1 entries per problem)
  nanstart.back() = NAN;
  R = check(3, rw, ne, true, true, 3, sz, et, 1.0, 1, nanstart.data(), 5);
  CHECK(R.kind == L0_LC_LSF && R.lsf.ls == L0_LS_START_BOX && R.lsf.which == 35);
}

static void test_index() {
  // problem q = (r * n_cells + e) * n_starts + s; six status words per problem, rows disjoint
  const int count = 3, cells = 5, starts = 4;
  std::vector<int> seen((size_t)count * cells * starts * 6, 0);
  for (int r = 0; r < count; ++r)
    for (int e = 0; e < cells; ++e)
      for (int s = 0; s < starts; ++s) {
        const int q = l0_lsf_index(r, e, s, cells, starts);
        const L0LsfProblem back = l0_lsf_split(q, cells, starts);
        CHECK(back.r == r && back.e == e && back.s == s);
        for (int w = 0; w < 6; ++w) ++seen[(size_t)q * 6 + w];
      }
  for (int v : seen) CHECK(v == 1);
}

static void test_rule() {
  const double M = 100.0;
  for (unsigned seed = 1; seed <= 6; ++seed) {
    const Problem P = problem(30, 10, 13, -1, 4711u * seed);  // (ld != p, the padding NaN: never read)
    const int p = P.p;
    std::vector<double> beta((size_t)p), greedy((size_t)p), prev((size_t)p, 0.0);
    for (int k = 1; k <= 6; ++k) {
      const double eta = (seed & 1) ? 0.0 : 0.05;
      const L0LsResult g = l0_local_solve<true>(P.G.data(), P.ld, P.c.data(), p, k, eta, M, P.yy, false, nullptr, greedy.data());
      const L0LsResult s = l0_local_solve<true>(P.G.data(), P.ld, P.c.data(), p, k, eta, M, P.yy, true, nullptr, beta.data());
      CHECK(g.status == 0 && s.status == 0 && g.swaps == 0);
      CHECK(g.nnz == k && s.nnz == k && g.grows == k && g.drops == 0);
      CHECK(s.grows == k && s.drops == 0);  // (a swap is neither)
      CHECK(fabs(s.F - quadratic(P, eta, beta.data())) <= 1e-12 * fabs(s.F));
      CHECK(s.F <= g.F + 1e-12 * fabs(g.F));  // the swaps start where greedy stops
      const double best = enumerate(P, k, eta);
      CHECK(s.F >= best - 1e-10 * fabs(best));  // never below the optimum
      CHECK(inescapable(P, k, eta, M, beta.data(), true, 1e-8));
      CHECK(inescapable(P, k, eta, M, greedy.data(), false, 1e-8));
      // the polish keeps the support and does not raise Q
      std::vector<double> pol = beta;
      const double qp = l0_ls_polish(P.G.data(), P.ld, P.c.data(), p, eta, M, pol.data());
      CHECK(qp <= s.F + 1e-12 * fabs(s.F) && fabs(qp - quadratic(P, eta, pol.data())) <= 1e-12 * fabs(qp));
      for (int j = 0; j < p; ++j) CHECK((pol[(size_t)j] != 0.0) == (beta[(size_t)j] != 0.0));
      // from the winner of k - 1 (grown) the result is a fixed point of the rule too, and no worse than that winner
      if (k > 1) {
        std::vector<double> chain((size_t)p);
        const L0LsResult c = l0_local_solve<true>(P.G.data(), P.ld, P.c.data(), p, k, eta, M, P.yy, true, prev.data(), chain.data());
        CHECK(c.status == 0 && c.nnz == k && c.grows == 1 && c.drops == 0);
        CHECK(c.F <= quadratic(P, eta, prev.data()) + 1e-12);
        CHECK(inescapable(P, k, eta, M, chain.data(), true, 1e-8));
      }
      // from the winner of k (shrunk to k - 1, then to 1): the surplus leaves, nothing grows beyond the size
      if (k > 1) {
        std::vector<double> down((size_t)p);
        const L0LsResult c = l0_local_solve<true>(P.G.data(), P.ld, P.c.data(), p, 1, eta, M, P.yy, true, beta.data(), down.data());
        CHECK(c.status == 0 && c.nnz == 1 && c.drops == k - 1 && c.grows == 0);
        CHECK(inescapable(P, 1, eta, M, down.data(), true, 1e-8));
      }
      prev = beta;
    }
  }
}

static void test_edges() {
  // p = 1
  {
    const double G[1] = {2.0}, c[1] = {3.0};
    double beta[1];
    L0LsResult R = l0_local_solve<true>(G, 1, c, 1, 1, 0.0, 100.0, 5.0, true, nullptr, beta);
    CHECK(R.status == 0 && R.nnz == 1 && R.grows == 1 && R.swaps == 0 && beta[0] == 1.5 && fabs(R.F + 2.25) < 1e-15);
    R = l0_local_solve<true>(G, 1, c, 1, 7, 0.25, 1.0, 5.0, true, nullptr, beta);  // the box binds; eta on the diagonal
    CHECK(R.nnz == 1 && beta[0] == 1.0 && fabs(R.F - (0.5 * 2.5 - 3.0)) < 1e-15);
  }
  // k >= p with a dead column: the grow stops at the live columns
  {
    const Problem P = problem(25, 7, 7, 3, 99u);
    std::vector<double> beta(7), start(7, 0.5);
    L0LsResult R = l0_local_solve<true>(P.G.data(), P.ld, P.c.data(), 7, 7, 0.0, 100.0, P.yy, true, nullptr, beta.data());
    CHECK(R.status == 0 && R.nnz == 6 && R.grows == 6 && beta[3] == 0.0);
    CHECK(inescapable(P, 7, 0.0, 100.0, beta.data(), true, 1e-8));
    R = l0_local_solve<true>(P.G.data(), P.ld, P.c.data(), 7, 20, 0.0, 100.0, P.yy, true, start.data(), beta.data());  // (a start on the dead column)
    CHECK(R.status == 0 && R.nnz == 6 && R.grows == 0 && R.drops == 0 && beta[3] == 0.0);
    const double all = enumerate(P, 7, 0.0);
    CHECK(fabs(R.F - all) <= 1e-9 * fabs(all));
  }
  // a binding box: every coordinate inside it, the certificate holds with the clip
  {
    const Problem P = problem(30, 9, 9, -1, 7u);
    std::vector<double> beta(9);
    const L0LsResult R = l0_local_solve<true>(P.G.data(), P.ld, P.c.data(), 9, 3, 0.0, 0.3, P.yy, true, nullptr, beta.data());
    int at_bound = 0;
    for (double b : beta) {
      CHECK(fabs(b) <= 0.3);
      at_bound += fabs(b) == 0.3;
    }
    CHECK(R.status == 0 && R.nnz == 3 && at_bound >= 1);
    CHECK(inescapable(P, 3, 0.0, 0.3, beta.data(), true, 1e-8));
  }
}

int main() {
  test_check();
  test_index();
  test_rule();
  test_edges();
  if (failures) {
    fprintf(stderr, "l0_local_subsets_host_test: %d failure(s)\n", failures);
    return 1;
  }
  printf("l0_local_subsets_host_test: ok\n");
  return 0;
}
