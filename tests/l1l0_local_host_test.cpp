// CPU test of the host side of the l0 local search with an l1 term (slm_solve_l0_local_l1) in csrc/l0_host.hpp:
// l0_local_solve<false, true>, the rule without a device and the kernel's twin, l0_ls_coord_l1, the polish l0_l1l_polish and the
// argument check l0_l1l_check -- meant to run under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_l1l0_local_cpu.py
// builds and runs it both plainly and sanitized).  Checks are against an enumeration of all supports with a lasso on each, the
// optimality conditions, the penalised twin at lam = 0, and -- given a file as the first argument -- cases exported from the numpy
// restatement of the rule (tests/_l1l0_local_reference.py): support, swaps, sweeps and F of every case.
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
// columns correlated (rho)
struct Problem {
  int p = 0;
  size_t ld = 0;
  std::vector<double> G, c;
  double yy = 0.0;
};
static Problem problem(int n, int p, size_t ld, double rho) {
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
static double objective(const Problem& P, double alpha, double lam, double eta, const double* b) {
  double F = 0.0;
  for (int i = 0; i < P.p; ++i) {
    if (b[i] == 0.0) continue;
    double t = 0.0;
    for (int j = 0; j < P.p; ++j) t += Hij(P, eta, i, j) * b[j];
    F += b[i] * (0.5 * t - P.c[(size_t)i]) + lam * fabs(b[i]) + alpha;
  }
  return F;
}

// min over ALL supports of (the lasso minimiser on the support, by its own plain descent to the last digit) + alpha on its non-zeros
static double enumerate(const Problem& P, double alpha, double lam, double eta, double M) {
  const int p = P.p;
  double best = 0.0;
  std::vector<double> b((size_t)p);
  for (unsigned mask = 1; mask < (1u << p); ++mask) {
    std::fill(b.begin(), b.end(), 0.0);
    for (int sweep = 0; sweep < 100000; ++sweep) {
      double worst = 0.0;
      for (int j = 0; j < p; ++j) {
        if (!(mask >> j & 1)) continue;
        double u = P.c[(size_t)j];
        for (int k = 0; k < p; ++k)
          if (k != j) u -= Hij(P, eta, j, k) * b[(size_t)k];
        const double s = u > lam ? u - lam : (u < -lam ? u + lam : 0.0);
        const double nb = fmin(fmax(s / Hij(P, eta, j, j), -M), M);
        worst = fmax(worst, fabs(nb - b[(size_t)j]));
        b[(size_t)j] = nb;
      }
      if (worst <= 1e-15) break;
    }
    best = fmin(best, objective(P, alpha, lam, eta, b.data()));
  }
  return best;
}

// From beta alone: every one-coordinate decision and (swaps) every (i, j) swap, recomputed with the coordinate written out here
static bool inescapable(const Problem& P, double alpha, double lam, double eta, double M, const double* beta, bool swaps, double tol) {
  const int p = P.p;
  std::vector<double> r((size_t)p), d((size_t)p);
  for (int i = 0; i < p; ++i) {
    d[(size_t)i] = Hij(P, eta, i, i);
    r[(size_t)i] = P.c[(size_t)i];
    for (int j = 0; j < p; ++j) r[(size_t)i] -= Hij(P, eta, i, j) * beta[j];
  }
  auto gain = [&](double u, double dj, double* b_out) {
    const double s = u > lam ? u - lam : (u < -lam ? u + lam : 0.0);
    const double b = fmin(fmax(s / dj, -M), M);
    if (b_out) *b_out = b;
    return u * b - 0.5 * dj * b * b - lam * fabs(b);
  };
  for (int j = 0; j < p; ++j) {
    double b;
    const double g = gain(r[(size_t)j] + d[(size_t)j] * beta[j], d[(size_t)j], &b);
    if (beta[j] != 0.0 && (!(g > alpha - tol * fmax(g, alpha)) || fabs(b - beta[j]) > tol * fmax(fabs(b), 1.0))) return false;
    if (beta[j] == 0.0 && g > alpha + tol * fmax(g, alpha)) return false;
  }
  for (int i = 0; i < p && swaps; ++i) {
    if (beta[i] == 0.0) continue;
    const double gi = gain(r[(size_t)i] + d[(size_t)i] * beta[i], d[(size_t)i], nullptr);
    for (int j = 0; j < p; ++j) {
      if (beta[j] != 0.0) continue;
      const double gj = gain(r[(size_t)j] + Hij(P, eta, j, i) * beta[i], d[(size_t)j], nullptr);
      if (gj > gi + (1e-10 + tol) * fmax(fabs(gi), alpha)) return false;
    }
  }
  return true;
}

static void test_coordinate() {
  // lam = 0: l0_ls_coord's b and gain
  for (double u : {-3.0, -0.2, 0.0, 0.7, 5.0}) {
    const L0LsCoord a = l0_ls_coord(u, 2.0, 1.5), b = l0_ls_coord_l1(u, 2.0, 1.5, 0.0);
    CHECK(a.b == b.b && a.gain == b.gain);
  }
  // the soft threshold, the clip behind it, the gain: F without alpha falls by it from 0 to b
  const L0LsCoord in = l0_ls_coord_l1(0.3, 2.0, 10.0, 0.5), pos = l0_ls_coord_l1(1.5, 2.0, 10.0, 0.5), neg = l0_ls_coord_l1(-1.5, 2.0, 10.0, 0.5);
  CHECK(in.b == 0.0 && in.gain == 0.0);
  CHECK(pos.b == 0.5 && neg.b == -0.5 && pos.gain == neg.gain && fabs(pos.gain - (1.5 * 0.5 - 0.25 - 0.25)) < 1e-15);
  const L0LsCoord clipped = l0_ls_coord_l1(9.0, 2.0, 1.0, 0.5);
  CHECK(clipped.b == 1.0 && fabs(clipped.gain - (9.0 - 1.0 - 0.5)) < 1e-15);
  static_assert(l0_ls_coord_l1(1.5, 2.0, 10.0, 0.5).b == 0.5, "constexpr: the kernel calls this very function");
}

static void test_against_enumeration() {
  int hits = 0, strictly = 0, cases = 0;
  for (int trial = 0; trial < 4; ++trial) {
    const int p = 8;
    const Problem P = problem(24, p, trial % 2 ? 11 : 8, 0.5 + 0.1 * trial);
    for (double rel : {0.002, 0.02})
      for (double lrel : {0.02, 0.1}) {
        const double alpha = rel * P.yy, lam = lrel * sqrt(P.yy), eta = trial == 3 ? 0.05 : 0.0, M = 100.0;
        std::vector<double> b0((size_t)p), b1((size_t)p);
        const L0LsResult R0 = l0_local_solve<false, true>(P.G.data(), P.ld, P.c.data(), p, alpha, eta, M, P.yy, false, nullptr, b0.data(), lam);
        const L0LsResult R1 = l0_local_solve<false, true>(P.G.data(), P.ld, P.c.data(), p, alpha, eta, M, P.yy, true, nullptr, b1.data(), lam);
        const double exact = enumerate(P, alpha, lam, eta, M), tol = 1e-9 * fmax(fabs(exact), alpha);
        CHECK(R0.status == 0 && R1.status == 0 && R0.swaps == 0);
        CHECK(fabs(R0.F - objective(P, alpha, lam, eta, b0.data())) <= tol && fabs(R1.F - objective(P, alpha, lam, eta, b1.data())) <= tol);
        CHECK(R1.F >= exact - tol);  // never below the optimum
        CHECK(R1.F <= R0.F + tol);   // swaps start from the descent's fixed point
        CHECK(inescapable(P, alpha, lam, eta, M, b0.data(), false, 1e-8));
        CHECK(inescapable(P, alpha, lam, eta, M, b1.data(), true, 1e-8));
        hits += fabs(R1.F - exact) <= tol;
        strictly += R1.F < R0.F - tol;
        ++cases;
        // the polish: the lasso's optimality conditions on the support, F not raised, alpha on the non-zeros that go back
        std::vector<double> bp = b1;
        const double val = l0_l1l_polish(P.G.data(), P.ld, P.c.data(), p, eta, lam, M, bp.data());
        int nnz = 0;
        for (int j = 0; j < p; ++j) nnz += bp[(size_t)j] != 0.0;
        CHECK(nnz <= R1.nnz && val + alpha * nnz <= R1.F + tol);
        CHECK(fabs(val + alpha * nnz - objective(P, alpha, lam, eta, bp.data())) <= tol);
        for (int j = 0; j < p; ++j) {
          if (b1[(size_t)j] == 0.0) {
            CHECK(bp[(size_t)j] == 0.0);  // the support is kept: zeros stay zero
            continue;
          }
          double g = -P.c[(size_t)j];
          for (int k = 0; k < p; ++k) g += Hij(P, eta, j, k) * bp[(size_t)k];
          if (bp[(size_t)j] > 0.0) CHECK(fabs(g + lam) <= 1e-12 * sqrt(P.yy));
          else if (bp[(size_t)j] < 0.0) CHECK(fabs(g - lam) <= 1e-12 * sqrt(P.yy));
          else CHECK(fabs(g) <= lam * (1.0 + 1e-12));
        }
      }
  }
  CHECK(hits >= 1);  // (the search is not required to be exact; that it never is would be a bug)
  printf("  enumeration: %d of %d at the optimum, swaps strictly better in %d\n", hits, cases, strictly);
}

static void test_lam_zero_is_the_penalised_twin() {
  for (int trial = 0; trial < 3; ++trial) {
    const int p = 12;
    const Problem P = problem(20, p, 16, 0.6 + 0.1 * trial);
    for (double rel : {0.003, 0.03}) {
      std::vector<double> a((size_t)p), b((size_t)p);
      const L0LsResult A = l0_local_solve<false>(P.G.data(), P.ld, P.c.data(), p, rel * P.yy, 0.01 * trial, 100.0, P.yy, true, nullptr, a.data());
      const L0LsResult B = l0_local_solve<false, true>(P.G.data(), P.ld, P.c.data(), p, rel * P.yy, 0.01 * trial, 100.0, P.yy, true, nullptr, b.data(), 0.0);
      CHECK(A.sweeps == B.sweeps && A.swaps == B.swaps && A.nnz == B.nnz && A.changes == B.changes && A.status == B.status);
      CHECK(fabs(A.F - B.F) <= 1e-14 * fabs(A.F));
      for (int j = 0; j < p; ++j) CHECK((a[(size_t)j] != 0.0) == (b[(size_t)j] != 0.0) && fabs(a[(size_t)j] - b[(size_t)j]) <= 1e-13 * fabs(a[(size_t)j]));
    }
  }
}

static void test_box_empty_and_polish_to_zero() {
  const int p = 10;
  const Problem P = problem(24, p, 12, 0.6);
  const double alpha = 0.002 * P.yy, lam = 0.02 * sqrt(P.yy), M = 0.4;
  std::vector<double> b((size_t)p);
  const L0LsResult R = l0_local_solve<false, true>(P.G.data(), P.ld, P.c.data(), p, alpha, 0.0, M, P.yy, true, nullptr, b.data(), lam);
  CHECK(R.status == 0);
  int bound = 0;
  for (int j = 0; j < p; ++j) {
    CHECK(fabs(b[(size_t)j]) <= M);
    bound += fabs(b[(size_t)j]) == M;
  }
  CHECK(bound >= 1);  // the box binds on an active coordinate
  CHECK(inescapable(P, alpha, lam, 0.0, M, b.data(), true, 1e-8));
  std::vector<double> bp = b;
  const double val = l0_l1l_polish(P.G.data(), P.ld, P.c.data(), p, 0.0, lam, M, bp.data());
  CHECK(val + alpha * R.nnz <= R.F + 1e-12 * fabs(R.F));
  for (int j = 0; j < p; ++j) {  // the optimality conditions of the box and the l1 term on the support
    CHECK(fabs(bp[(size_t)j]) <= M);
    if (bp[(size_t)j] == 0.0) continue;
    double g = -P.c[(size_t)j];
    for (int k = 0; k < p; ++k) g += Hij(P, 0.0, j, k) * bp[(size_t)k];
    g += bp[(size_t)j] > 0.0 ? lam : -lam;
    if (bp[(size_t)j] == M) CHECK(g <= 1e-10);
    else if (bp[(size_t)j] == -M) CHECK(g >= -1e-10);
    else CHECK(fabs(g) <= 1e-10);
  }
  // a lam above max |c| empties the support, from a start too
  double cmax = 0.0;
  for (int j = 0; j < p; ++j) cmax = fmax(cmax, fabs(P.c[(size_t)j]));
  const L0LsResult E = l0_local_solve<false, true>(P.G.data(), P.ld, P.c.data(), p, 0.0, 0.0, 100.0, P.yy, true, nullptr, b.data(), 1.01 * cmax);
  CHECK(E.status == 0 && E.nnz == 0 && E.F == 0.0);
  // a support the lasso does not use in full: the polish brings a coefficient to zero, it goes back as zero, F falls
  std::vector<double> st((size_t)p, 0.0);
  st[1] = -1.0; st[2] = 1e-3; st[4] = 1.0;
  const double lam2 = 0.05 * sqrt(P.yy), F_in = objective(P, alpha, lam2, 0.0, st.data());
  std::vector<double> out = st;
  const double v = l0_l1l_polish(P.G.data(), P.ld, P.c.data(), p, 0.0, lam2, 100.0, out.data());
  int nnz = 0;
  for (int j = 0; j < p; ++j) nnz += out[(size_t)j] != 0.0;
  CHECK(v + alpha * nnz <= F_in && fabs(v + alpha * nnz - objective(P, alpha, lam2, 0.0, out.data())) <= 1e-12 * fabs(F_in));
  for (int j = 0; j < p; ++j)
    if (st[(size_t)j] == 0.0) CHECK(out[(size_t)j] == 0.0);
  // nothing to polish
  std::vector<double> zero((size_t)p, 0.0);
  CHECK(l0_l1l_polish(P.G.data(), P.ld, P.c.data(), p, 0.0, lam, M, zero.data()) == 0.0);
}

static void test_checks() {
  const double ok[2] = {0.1, 0.0}, neg[2] = {0.1, -1.0}, nan_[2] = {NAN, 0.0}, inf_[2] = {0.1, INFINITY};
  const double w[3] = {1.0, 0.0, 2.0}, wbad[3] = {1.0, -1.0, 2.0};
  const double* rows[2] = {nullptr, w};
  const double* rows_bad[2] = {nullptr, wbad};
  const long long ne[2] = {0, 3};
  auto check = [&](long long count, const double* const* rw, const double* al, const double* l1, const double* rd, double M = 1.0,
                   long long cells = 2, long long starts = 1, const double* st = nullptr, long long p = 2, bool icpt = false, bool alone = true) {
    return l0_l1l_check(count, rw, ne, 3, icpt, alone, cells, al, l1, rd, M, starts, st, p);
  };
  CHECK(check(2, rows, ok, ok, ok).kind == L0_L1L_OK && check(2, rows, ok, ok, nullptr).kind == L0_L1L_OK);
  // 1. NULL alphas or l1s, before anything else (a bad count too)
  CHECK(check(0, rows, nullptr, ok, ok).kind == L0_L1L_NULL && check(2, rows, ok, nullptr, neg).kind == L0_L1L_NULL);
  // 2. the l1 weights, before the ridges and before everything of the row sets
  L0L1lRefusal R = check(0, rows, nan_, neg, neg);
  CHECK(R.kind == L0_L1L_L1 && R.which == 1);
  R = check(2, rows, ok, nan_, ok);
  CHECK(R.kind == L0_L1L_L1 && R.which == 0);
  CHECK(check(2, rows, ok, inf_, ok).kind == L0_L1L_L1);
  // 3. the ridges where given
  R = check(0, rows, nan_, ok, inf_);
  CHECK(R.kind == L0_L1L_RIDGE && R.which == 1);
  // 4. l0_lsf_check's, in its order
  CHECK(check(0, rows, ok, ok, ok).kind == L0_L1L_LSF && check(0, rows, ok, ok, ok).lsf.kind == L0_LSF_COUNT);
  CHECK(check(17, rows, ok, ok, nullptr).lsf.kind == L0_LSF_COUNT);
  CHECK(check(2, nullptr, ok, ok, ok).lsf.kind == L0_LSF_NULL);
  CHECK(check(2, rows, ok, ok, ok, 1.0, 2, L0_LS_MAX_PROBLEMS).lsf.kind == L0_LSF_PRODUCT);
  R = check(2, rows, ok, ok, ok, 1.0, 0);
  CHECK(R.lsf.kind == L0_LSF_LS && R.lsf.ls == L0_LS_CELLS);
  R = check(2, rows, ok, ok, ok, 1.0, 2, 0);
  CHECK(R.lsf.kind == L0_LSF_LS && R.lsf.ls == L0_LS_STARTS);
  R = check(2, rows, ok, ok, nullptr, -1.0);
  CHECK(R.lsf.kind == L0_LSF_LS && R.lsf.ls == L0_LS_BIG_M);
  R = check(2, rows, neg, ok, nullptr);
  CHECK(R.kind == L0_L1L_LSF && R.lsf.ls == L0_LS_ALPHA && R.lsf.which == 1);
  R = check(2, rows, ok, ok, ok, 1.0, 2, 1, nullptr, L0_LS_PMAX + 1);
  CHECK(R.lsf.kind == L0_LSF_LS && R.lsf.ls == L0_LS_WIDTH);
  CHECK(check(2, rows, ok, ok, ok, 1.0, 2, 1, nullptr, L0_LS_PMAX + 1, true).kind == L0_L1L_OK);  // (the intercept's column is not searched)
  CHECK(check(2, rows, ok, ok, ok, 1.0, 2, 1, nullptr, 2, true, false).lsf.kind == L0_LSF_INTERCEPT);
  R = check(2, rows_bad, ok, ok, ok);
  CHECK(R.lsf.kind == L0_LSF_WEIGHT && R.lsf.row_set == 1 && R.lsf.which == 1);
  const double st[8] = {0.0, 0.5, -0.5, 0.0, 0.0, 0.0, 2.0, 0.0};
  R = check(2, rows, ok, ok, ok, 1.0, 2, 1, st);
  CHECK(R.lsf.kind == L0_LSF_LS && R.lsf.ls == L0_LS_START_BOX && R.lsf.which == 6);
  CHECK(check(2, rows, ok, ok, ok, 2.0, 2, 1, st).kind == L0_L1L_OK);
}

// Cases exported from the numpy restatement, one per block:
//   p ld alpha lam eta big_M yy swaps(0/1) has_start want_swaps want_sweeps want_F / G rows (p x p) / c / start (if any) / support (p ints)
static void test_exported(const char* path) {
  FILE* fh = fopen(path, "r");
  CHECK(fh != nullptr);
  if (!fh) return;
  int cases = 0, p, ld, swaps, has_start, want_swaps, want_sweeps;
  double alpha, lam, eta, M, yy, want_F;
  while (fscanf(fh, "%d %d %lf %lf %lf %lf %lf %d %d %d %d %lf", &p, &ld, &alpha, &lam, &eta, &M, &yy, &swaps, &has_start, &want_swaps,
                &want_sweeps, &want_F) == 12) {
    std::vector<double> G((size_t)p * ld, NAN), c((size_t)p), st((size_t)p), b((size_t)p);
    std::vector<int> sup((size_t)p);
    bool ok = true;
    for (int i = 0; i < p; ++i)
      for (int j = 0; j < p; ++j) ok = ok && fscanf(fh, "%lf", &G[(size_t)i * ld + j]) == 1;
    for (int i = 0; i < p; ++i) ok = ok && fscanf(fh, "%lf", &c[(size_t)i]) == 1;
    for (int i = 0; i < p && has_start; ++i) ok = ok && fscanf(fh, "%lf", &st[(size_t)i]) == 1;
    for (int i = 0; i < p; ++i) ok = ok && fscanf(fh, "%d", &sup[(size_t)i]) == 1;
    CHECK(ok);
    if (!ok) break;
    const L0LsResult R = l0_local_solve<false, true>(G.data(), (size_t)ld, c.data(), p, alpha, eta, M, yy, swaps != 0, has_start ? st.data() : nullptr,
                                                     b.data(), lam);
    CHECK(R.status == 0 && R.swaps == want_swaps && R.sweeps == want_sweeps);
    CHECK(fabs(R.F - want_F) <= 1e-10 * fmax(fabs(want_F), alpha));
    for (int j = 0; j < p; ++j) CHECK((b[(size_t)j] != 0.0) == (sup[(size_t)j] != 0));
    ++cases;
  }
  fclose(fh);
  CHECK(cases >= 1);
  printf("  exported: %d cases\n", cases);
}

int main(int argc, char** argv) {
  test_coordinate();
  test_against_enumeration();
  test_lam_zero_is_the_penalised_twin();
  test_box_empty_and_polish_to_zero();
  test_checks();
  if (argc > 1) test_exported(argv[1]);
  if (failures) {
    fprintf(stderr, "l1l0_local_host_test: %d failure(s)\n", failures);
    return 1;
  }
  printf("l1l0_local_host_test: ok\n");
  return 0;
}
