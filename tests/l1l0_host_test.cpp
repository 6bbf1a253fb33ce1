// CPU test of the l1 mode of csrc/l0_host.hpp -- the host side of slm_solve_l0_l1 (L1L0): the coordinate step the kernel
// shares, the descent over all columns of a support, its polish, a support's value and coefficients, and the lasso dual
// bound on all columns -- meant to run under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_l1l0_cpu.py builds
// and runs it both plainly and sanitized).  Every check is against a closed form or against the optimality conditions,
// never against another run of the code under test.
#include <math.h>
#include <stdio.h>

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

// A 6 x 6 symmetric positive definite matrix from a fixed recurrence, and c.
static void spd6(double* H /* [36] */, double* c /* [6] */) {
  double A[8][6];
  unsigned v = 2024u;
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 6; ++j) {
      v = v * 1103515245u + 12345u;
      A[i][j] = (double)((v >> 16) & 0x3ff) / 512.0 - 1.0;
    }
  for (int i = 0; i < 6; ++i) {
    for (int j = 0; j < 6; ++j) {
      double t = i == j ? 0.25 : 0.0;
      for (int k = 0; k < 8; ++k) t += A[k][i] * A[k][j];
      H[i * 6 + j] = t;
    }
    c[i] = 0.5 * (double)(i + 1) * ((i & 1) ? -1.0 : 1.0);
  }
}

// The largest violation of the optimality conditions of min 1/2 b^T H b - c^T b + eta ||b||_1 over |b_j| <= M on `cols`.
static double kkt(const double* H, const double* c, int p, const int* cols, int m, double eta, double M, const double* b) {
  double worst = 0.0;
  for (int r = 0; r < m; ++r) {
    double g = -c[cols[r]];
    for (int k = 0; k < m; ++k) g += H[cols[r] * p + cols[k]] * b[k];
    double v;
    if (b[r] == 0.0) v = fmax(fabs(g) - eta, 0.0);
    else if (b[r] >= M) v = fmax(g + eta, 0.0);
    else if (b[r] <= -M) v = fmax(eta - g, 0.0);
    else v = fabs(g + (b[r] > 0.0 ? eta : -eta));
    worst = fmax(worst, v);
  }
  return worst;
}

static void test_step() {
  // soft-threshold, then the box; a column of zeros keeps a zero coefficient
  CHECK(l0_l1_step(0.0, -3.0, 2.0, 1.0, 10.0) == 1.0);    // u = 1.5, th = 0.5
  CHECK(l0_l1_step(0.0, 3.0, 2.0, 1.0, 10.0) == -1.0);
  CHECK(l0_l1_step(0.0, -0.5, 2.0, 1.0, 10.0) == 0.0);    // |u| = 0.25 <= th
  CHECK(l0_l1_step(1.0, -8.0, 2.0, 1.0, 3.0) == 3.0);     // u = 5, soft 4.5, clipped
  CHECK(l0_l1_step(-1.0, 8.0, 2.0, 1.0, 3.0) == -3.0);
  CHECK(l0_l1_step(1.0, -8.0, 0.0, 1.0, 3.0) == 0.0);
  CHECK(l0_l1_step(2.0, -1.0, 4.0, 0.0, 100.0) == 2.25);  // eta = 0: the plain step
}

static void test_identity_closed_form() {
  // H = I: b_j = clip(soft(c_j, eta), M), one sweep
  const double H[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, c[3] = {3.0, -0.2, -1.5};
  const int cols[3] = {0, 1, 2};
  double b[3] = {0, 0, 0};
  double v = l0_l1_descent(H, c, 3, cols, 3, 0.5, 100.0, b);
  CHECK(b[0] == 2.5 && b[1] == 0.0 && b[2] == -1.0);
  CHECK(near(v, (0.5 * 6.25 - 7.5 + 1.25) + (0.5 - 1.5 + 0.5), 1e-15));
  CHECK(near(l0_l1_value(H, c, 3, cols, 3, 0.5, b), v, 1e-15));
  // a binding box: b_0 = 2 exactly, value 1/2 4 - 6 + 1 = -3 on that coordinate
  double bb[3] = {0, 0, 0};
  v = l0_l1_descent(H, c, 3, cols, 3, 0.5, 2.0, bb);
  CHECK(bb[0] == 2.0 && bb[1] == 0.0 && bb[2] == -1.0);
  CHECK(near(v, -3.0 - 0.5, 1e-15));
  CHECK(near(l0_l1_polish(H, c, 3, cols, 3, 0.5, 2.0, bb), v, 1e-15) && bb[0] == 2.0);
  // a box of zero width, and no columns at all
  double bz[3] = {1, 1, 1};
  CHECK(l0_l1_descent(H, c, 3, cols, 3, 0.5, 0.0, bz) == 0.0 && bz[0] == 0.0 && bz[2] == 0.0);
  CHECK(l0_l1_descent(H, c, 3, cols, 0, 0.5, 1.0, bz) == 0.0);
  CHECK(l0_l1_polish(H, c, 3, cols, 0, 0.5, 1.0, bz) == 0.0);
}

static void test_dependent_column_carries_the_coefficient() {
  // columns a, b (orthonormal) and a + b; y = t (a + b).  Columns a and b alone: t - eta each, value -(t - eta)^2.  With the
  // third column the unique minimiser is (0, 0, t - eta / 2), value -(t - eta / 2)^2: the dependent column LOWERS the value.
  const double t = 3.0, eta = 0.5;
  const double H[9] = {1, 0, 1, 0, 1, 1, 1, 1, 2}, c[3] = {t, t, 2 * t};
  const std::vector<int> one_group = {0, 3}, singles = {0, 1, 2, 3};
  double beta[3];
  for (int polish = 0; polish < 2; ++polish) {
    double v = l0_l1_support(H, c, 3, one_group, 1ull, eta, 100.0, polish != 0, beta);
    CHECK(near(v, -(t - eta / 2) * (t - eta / 2), polish ? 1e-14 : 1e-10));
    CHECK(beta[0] == 0.0 && beta[1] == 0.0 && near(beta[2], t - eta / 2, polish ? 1e-14 : 1e-9));
    v = l0_l1_support(H, c, 3, singles, 3ull, eta, 100.0, polish != 0, beta);
    CHECK(near(v, -(t - eta) * (t - eta), 1e-14) && beta[2] == 0.0 && near(beta[0], t - eta, 1e-14) && near(beta[1], t - eta, 1e-14));
  }
  // without an l1 term the pivot rule's answer stands: the third column stays at zero, the value is -t^2
  CHECK(near(l0_support(H, c, 3, one_group, 1ull, 100.0, true, beta), -t * t, 1e-14) && beta[2] == 0.0);
  // the empty support
  CHECK(l0_l1_support(H, c, 3, singles, 0ull, eta, 100.0, true, beta) == 0.0 && beta[0] == 0.0 && beta[1] == 0.0 && beta[2] == 0.0);
}

static void test_descent_and_polish_on_a_dense_block() {
  double H[36], c[6];
  spd6(H, c);
  const int all[6] = {0, 1, 2, 3, 4, 5}, some[4] = {5, 0, 3, 2};
  for (int which = 0; which < 2; ++which) {
    const int* cols = which ? some : all;
    const int m = which ? 4 : 6;
    for (double eta : {0.05, 0.6, 1.4}) {
      for (double M : {100.0, 0.4}) {
        double b[6] = {0, 0, 0, 0, 0, 0};
        const double v = l0_l1_descent(H, c, 6, cols, m, eta, M, b);
        CHECK(near(l0_l1_value(H, c, 6, cols, m, eta, b), v, 1e-13));
        CHECK(kkt(H, c, 6, cols, m, eta, M, b) <= 1e-9);
        for (int k = 0; k < m; ++k) CHECK(fabs(b[k]) <= M);
        double bp[6];
        for (int k = 0; k < m; ++k) bp[k] = b[k];
        const double vp = l0_l1_polish(H, c, 6, cols, m, eta, M, bp);
        CHECK(vp <= v + 1e-14 * fmax(1.0, fabs(v)));  // not above the value of the descent (to rounding)
        CHECK(near(l0_l1_value(H, c, 6, cols, m, eta, bp), vp, 1e-15));
        CHECK(kkt(H, c, 6, cols, m, eta, M, bp) <= (M > 1.0 ? 1e-13 : 1e-9));  // (inside a wide box the exact solve is always taken)
        for (int k = 0; k < m; ++k) CHECK(fabs(bp[k]) <= M && (b[k] == 0.0) == (bp[k] == 0.0));
      }
    }
  }
  // eta at or above ||c||_inf: nothing enters
  double b[6] = {0, 0, 0, 0, 0, 0};
  CHECK(l0_l1_descent(H, c, 6, all, 6, 3.0, 100.0, b) == 0.0);
  for (int k = 0; k < 6; ++k) CHECK(b[k] == 0.0);
  // a column of zeros inside the support: no division by zero, its coefficient stays 0
  double Hz[9] = {2, 0, 1, 0, 0, 0, 1, 0, 3}, cz[3] = {1.0, 0.0, -2.0};
  const int cols3[3] = {0, 1, 2};
  double bz[3] = {0, 5.0, 0};
  const double vz = l0_l1_descent(Hz, cz, 3, cols3, 3, 0.1, 100.0, bz);
  CHECK(bz[1] == 0.0 && std::isfinite(vz) && kkt(Hz, cz, 3, cols3, 3, 0.1, 100.0, bz) <= 1e-10);
}

static void test_lower_bound() {
  double H[36], c[6];
  spd6(H, c);
  const int all[6] = {0, 1, 2, 3, 4, 5};
  L0Factor f(H, c, 6);
  for (int j = 0; j < 6; ++j) CHECK(f.push(j));
  const double q_all = -0.5 * f.ss;
  const double yy = f.ss + 1.0;  // y^T y / n = c^T H^-1 c + the residual's share: a consistent (H, c, yy)
  CHECK(l0_l1_lower_bound(H, c, 6, yy, 0.0, q_all) == q_all);
  double last = q_all;
  for (double eta : {1e-3, 0.05, 0.6, 1.4, 2.9}) {
    double b[6] = {0, 0, 0, 0, 0, 0};
    const double primal = l0_l1_descent(H, c, 6, all, 6, eta, HUGE_VAL, b);
    const double lb = l0_l1_lower_bound(H, c, 6, yy, eta, q_all);
    CHECK(lb >= q_all && lb <= primal);                                // a lower bound, never below the one there was
    CHECK(primal - lb <= 1e-6 * fabs(primal) + 1e-8 * (yy + f.ss));  // and tight: the descent's point is nearly optimal
    CHECK(lb >= last - 1e-9 * yy);                                     // monotone in eta, as f is (up to the margin)
    last = lb;
  }
  // eta >= ||c||_inf: f(all) = 0 and the bound reaches it up to its margin
  const double lb0 = l0_l1_lower_bound(H, c, 6, yy, 3.0, q_all);
  CHECK(lb0 <= 0.0 && lb0 >= -1e-9 * yy);
  // a non-finite yy, or no columns, fall back to q_all
  CHECK(l0_l1_lower_bound(H, c, 6, NAN, 0.6, q_all) == q_all);
  CHECK(l0_l1_lower_bound(H, c, 0, yy, 0.6, q_all) == q_all);
}

int main() {
  test_step();
  test_identity_closed_form();
  test_dependent_column_carries_the_coefficient();
  test_descent_and_polish_on_a_dense_block();
  test_lower_bound();
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("l1l0_host_test: ok\n");
  return 0;
}
