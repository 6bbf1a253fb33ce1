// CPU test of the constrained mode of csrc/l0_host.hpp -- the host side of slm_solve_l0_constrained: the splitting that values
// a support (the kernel's own), its face polish, the dual value at arbitrary admissible multipliers, the positive-definite
// check and the lower bound on all columns -- meant to run under AddressSanitizer and UndefinedBehaviorSanitizer
// (tests/test_l0_constrained_cpu.py builds and runs it both plainly and sanitized).  Every check is against a closed form or
// against the optimality conditions, never against another run of the code under test.
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

static unsigned rng_state = 2025u;
static double rnd() {  // uniform in [-1, 1)
  rng_state = rng_state * 1103515245u + 12345u;
  return (double)((rng_state >> 16) & 0x3ff) / 512.0 - 1.0;
}

// A problem with its storage: H = B^T B / n + ridge I, c, m rows scaled to unit norm, a box
struct Problem {
  int p, m;
  std::vector<double> H, c, A, lo, hi, blo, bhi;
  L0ConProblem view(int max_sweeps = 0) const {
    L0ConProblem P;
    P.H = H.data(); P.c = c.data(); P.p = p;
    P.A = A.data(); P.m = m; P.lo = lo.data(); P.hi = hi.data();
    P.blo = blo.data(); P.bhi = bhi.data();
    P.rho = l0_con_rho(H.data(), p, A.data(), m);
    P.max_sweeps = max_sweeps;
    return P;
  }
};

static Problem random_problem(int p, int m, int n, double ridge, bool nonneg) {
  Problem Q;
  Q.p = p; Q.m = m;
  std::vector<double> B((size_t)n * p);
  for (double& v : B) v = rnd();
  Q.H.assign((size_t)p * p, 0.0);
  Q.c.assign((size_t)p, 0.0);
  for (int i = 0; i < p; ++i) {
    for (int j = 0; j < p; ++j) {
      double t = i == j ? ridge : 0.0;
      for (int k = 0; k < n; ++k) t += B[(size_t)k * p + i] * B[(size_t)k * p + j] / n;
      Q.H[(size_t)i * p + j] = t;
    }
    Q.c[(size_t)i] = 2.0 * rnd();
  }
  Q.A.assign((size_t)m * p, 0.0);
  Q.lo.assign((size_t)m, 0.0);
  Q.hi.assign((size_t)m, 0.0);
  for (int i = 0; i < m; ++i) {
    double nn = 0.0;
    for (int j = 0; j < p; ++j) {
      Q.A[(size_t)i * p + j] = rnd();
      nn += Q.A[(size_t)i * p + j] * Q.A[(size_t)i * p + j];
    }
    for (int j = 0; j < p; ++j) Q.A[(size_t)i * p + j] /= sqrt(nn);
    // 0 is feasible for every row: one-sided, two-sided and equality rows in turn
    Q.lo[(size_t)i] = i % 3 == 0 ? -HUGE_VAL : (i % 3 == 1 ? -0.3 : 0.0);
    Q.hi[(size_t)i] = i % 3 == 0 ? 0.2 : (i % 3 == 1 ? 0.1 : 0.0);
  }
  Q.blo.assign((size_t)p, nonneg ? 0.0 : -3.0);
  Q.bhi.assign((size_t)p, 3.0);
  return Q;
}

// The largest violation of the optimality conditions of min 1/2 b^T H b - c^T b s.t. box, lo <= A b <= hi on `cols`, given
// the rows' multipliers y and the box multipliers mu: stationarity, feasibility, signs, complementarity.
static double kkt(const L0ConProblem& P, const int* cols, int ms, const L0ConPoint& R) {
  double worst = 0.0;
  for (int r = 0; r < ms; ++r) {
    double g = -P.c[cols[r]] + R.mu[(size_t)r];
    for (int k = 0; k < ms; ++k) g += P.H[cols[r] * P.p + cols[k]] * R.beta[(size_t)k];
    for (int i = 0; i < P.m; ++i) g += P.A[i * P.p + cols[r]] * R.y[(size_t)i];
    worst = fmax(worst, fabs(g));
    const double b = R.beta[(size_t)r], mu = R.mu[(size_t)r];
    worst = fmax(worst, fmax(P.blo[cols[r]] - b, b - P.bhi[cols[r]]));
    if (mu > 0.0) worst = fmax(worst, fabs(b - P.bhi[cols[r]]));
    if (mu < 0.0) worst = fmax(worst, fabs(b - P.blo[cols[r]]));
  }
  for (int i = 0; i < P.m; ++i) {
    double t = 0.0;
    for (int r = 0; r < ms; ++r) t += P.A[i * P.p + cols[r]] * R.beta[(size_t)r];
    worst = fmax(worst, fmax(P.lo[i] - t, t - P.hi[i]));
    if (R.y[(size_t)i] > 0.0) worst = fmax(worst, fabs(t - P.hi[i]));
    if (R.y[(size_t)i] < 0.0) worst = fmax(worst, fabs(t - P.lo[i]));
  }
  return worst;
}

static void test_shared_pieces() {
  CHECK(l0_con_sigma(2.0, -1.0, 3.0) == 6.0 && l0_con_sigma(-2.0, -1.0, 3.0) == 2.0 && l0_con_sigma(0.0, -HUGE_VAL, HUGE_VAL) == 0.0);
  CHECK(l0_con_sigma(1.0, 0.0, HUGE_VAL) == HUGE_VAL && l0_con_sigma(-1.0, -HUGE_VAL, 0.0) == HUGE_VAL);  // inadmissible signs
  CHECK(l0_con_box_mu(1.0, -0.5, 0.0, 1.0) == 0.5 && l0_con_box_mu(0.0, 0.5, 0.0, 1.0) == -0.5);
  CHECK(l0_con_box_mu(0.5, -0.5, 0.0, 1.0) == 0.0 && l0_con_box_mu(1.0, 0.5, 0.0, 1.0) == 0.0);
  CHECK(l0_con_step(0.5, 1.0, 2.0, 0.0, 1.0) == 0.0 && l0_con_step(0.5, -4.0, 2.0, 0.0, 1.0) == 1.0 && l0_con_step(0.5, 0.5, 2.0, 0.0, 1.0) == 0.25);
  CHECK(l0_con_violation(0.5, 0.0, 1.0, 2.0) == 0.0 && l0_con_violation(1.5, 0.0, 1.0, 2.0) == 0.25 && l0_con_violation(-3.0, -1.0, HUGE_VAL, 0.5) == 2.0);
  const L0ConDual d = l0_con_dual(4.0, 1.0, 3.0);
  CHECK(d.raw == -3.0 && d.mag == 5.0 && d.bound < d.raw && near(d.bound, -3.0 - 5e-10, 1e-15));
}

// H = I: min 1/2 ||b||^2 - c^T b s.t. a^T b <= h has b = c - lambda a, lambda = max(0, (a^T c - h) / ||a||^2)
static void test_closed_forms() {
  const int p = 4;
  Problem Q;
  Q.p = p; Q.m = 1;
  Q.H.assign(16, 0.0);
  for (int j = 0; j < p; ++j) Q.H[(size_t)j * p + j] = 1.0;
  Q.c = {1.0, 2.0, -1.0, 0.5};
  Q.A = {0.5, 0.5, 0.5, 0.5};
  Q.lo = {-HUGE_VAL};
  Q.hi = {0.25};
  Q.blo.assign(4, -10.0);
  Q.bhi.assign(4, 10.0);
  int cols[4] = {0, 1, 2, 3};
  {  // one active row
    const L0ConProblem P = Q.view();
    L0ConPoint R = l0_con_solve(P, cols, p, HUGE_VAL);
    CHECK(R.outcome == 0);
    CHECK(l0_con_polish(P, cols, p, R) && R.polished);
    const double lam = (0.5 * 2.5 - 0.25) / 1.0;
    CHECK(near(R.y[0], lam, 1e-13));
    for (int j = 0; j < p; ++j) CHECK(near(R.beta[(size_t)j], Q.c[(size_t)j] - lam * 0.5, 1e-13));
    double val = 0.0;
    for (int j = 0; j < p; ++j) val += R.beta[(size_t)j] * (0.5 * R.beta[(size_t)j] - Q.c[(size_t)j]);
    CHECK(near(R.primal, val, 1e-14) && R.bound <= val);
    CHECK(kkt(P, cols, p, R) <= 1e-13);
  }
  {  // an equality whose multiplier is negative: a^T b = 2 > a^T c
    Q.lo = {2.0};
    Q.hi = {2.0};
    const L0ConProblem P = Q.view();
    L0ConPoint R = l0_con_solve(P, cols, p, HUGE_VAL);
    CHECK(R.outcome == 0 && l0_con_polish(P, cols, p, R));
    const double lam = (0.5 * 2.5 - 2.0) / 1.0;
    CHECK(lam < 0.0 && near(R.y[0], lam, 1e-13));
    for (int j = 0; j < p; ++j) CHECK(near(R.beta[(size_t)j], Q.c[(size_t)j] - lam * 0.5, 1e-13));
  }
  {  // a row that never binds: the unconstrained minimiser in one sweep, multipliers zero
    Q.lo = {-HUGE_VAL};
    Q.hi = {5.0};
    const L0ConProblem P = Q.view();
    L0ConPoint R = l0_con_solve(P, cols, p, HUGE_VAL);
    CHECK(R.outcome == 0 && R.sweeps == 1 && R.y[0] == 0.0);
    CHECK(l0_con_polish(P, cols, p, R));
    for (int j = 0; j < p; ++j) CHECK(near(R.beta[(size_t)j], Q.c[(size_t)j], 1e-14) && R.mu[(size_t)j] == 0.0);
  }
  {  // a binding box beside a binding row: b_1 <= 1 (c_1 = 2)
    Q.hi = {0.25};
    Q.bhi[1] = 1.0;
    const L0ConProblem P = Q.view();
    L0ConPoint R = l0_con_solve(P, cols, p, HUGE_VAL);
    CHECK(R.outcome == 0 && l0_con_polish(P, cols, p, R));
    CHECK(kkt(P, cols, p, R) <= 1e-13 && R.beta[1] <= 1.0);
    Q.bhi[1] = 10.0;
  }
  {  // an infeasible support, seen without a solve: the row is zero on the columns {2, 3} and excludes 0
    Q.A = {0.5, 0.5, 0.0, 0.0};
    Q.lo = {1.0};
    Q.hi = {HUGE_VAL};
    const L0ConProblem P = Q.view();
    int sub[2] = {2, 3};
    const L0ConPoint R = l0_con_solve(P, sub, 2, HUGE_VAL);
    CHECK(R.outcome == 1 && R.bound == HUGE_VAL && R.sweeps == 0);
    int sup[2] = {0, 2};  // ... and feasible with column 0
    L0ConPoint R2 = l0_con_solve(P, sup, 2, HUGE_VAL);
    CHECK(R2.outcome == 0 && l0_con_polish(P, sup, 2, R2) && near(R2.beta[0], 2.0, 1e-13));
  }
  {  // an infeasible support the box makes so: b_0 + b_1 >= 3 sqrt(1/2) ... with b <= 1; rejected against the value cap
    Q.A = {sqrt(0.5), sqrt(0.5), 0.0, 0.0};
    Q.lo = {3.0 * sqrt(0.5)};
    Q.hi = {HUGE_VAL};
    Q.blo.assign(4, -1.0);
    Q.bhi.assign(4, 1.0);
    const L0ConProblem P = Q.view();
    const double cap = l0_con_value_cap(Q.H.data(), Q.c.data(), p, Q.blo.data(), Q.bhi.data());
    CHECK(near(cap, 4.5 + 2.0, 1e-14));
    const L0ConPoint R = l0_con_solve(P, cols, p, cap);
    CHECK(R.outcome == 1 && R.bound > cap);
  }
}

static void test_random_problems() {
  double worst = 0.0;
  int most = 0, polished = 0, total = 0;
  for (int trial = 0; trial < 24; ++trial) {
    const int p = 6 + trial % 7, m = 1 + trial % 6;
    const Problem Q = random_problem(p, m, 3 * p, 0.02, trial % 2 == 0);
    const L0ConProblem P = Q.view();
    CHECK(l0_con_pd(Q.H.data(), Q.c.data(), p));
    int cols[L0_PMAX];
    // the support of all columns and one of every other column
    for (int pass = 0; pass < 2; ++pass) {
      int ms = 0;
      for (int j = 0; j < p; j += 1 + pass) cols[ms++] = j;
      L0ConPoint R = l0_con_solve(P, cols, ms, HUGE_VAL);
      CHECK(R.outcome == 0);
      most = R.sweeps > most ? R.sweeps : most;
      const double before = R.primal, bound = R.bound;
      CHECK(bound <= before + 1e-6 * fmax(1.0, fabs(before)));  // (the point may undercut f(S) by its violation times the multipliers)
      ++total;
      if (l0_con_polish(P, cols, ms, R)) {
        ++polished;
        worst = fmax(worst, kkt(P, cols, ms, R));
        // the face point is the minimiser: the dual bound of the splitting is below it, and the splitting's point near it
        CHECK(bound <= R.primal && fabs(before - R.primal) <= 1e-7 * fmax(1.0, fabs(R.primal)));
        if (!(bound <= R.primal && fabs(before - R.primal) <= 1e-7 * fmax(1.0, fabs(R.primal))))
          fprintf(stderr, "  trial %d pass %d: bound %.17g, splitting %.17g, face %.17g\n", trial, pass, bound, before, R.primal);
        // weak duality at random admissible multipliers, and at the optimal ones where it is tight
        for (int draw = 0; draw < 8; ++draw) {
          std::vector<double> y((size_t)m), mu((size_t)ms);
          for (int i = 0; i < m; ++i) {
            double v = 2.0 * rnd();
            if (v > 0.0 && !(Q.hi[(size_t)i] < HUGE_VAL)) v = -v;
            if (v < 0.0 && !(Q.lo[(size_t)i] > -HUGE_VAL)) v = -v;
            y[(size_t)i] = v;
          }
          for (int r = 0; r < ms; ++r) mu[(size_t)r] = draw % 2 ? 0.5 * rnd() : 0.0;
          const L0ConDual d = l0_con_dual_at(P, cols, ms, y.data(), mu.data());
          CHECK(d.bound <= R.primal);
        }
        const L0ConDual tight = l0_con_dual_at(P, cols, ms, R.y.data(), R.mu.data());
        CHECK(tight.bound <= R.primal && R.primal - tight.raw <= 1e-9 * tight.mag);
        if (pass == 0) {  // F_lb <= the all-columns optimum
          const double q_all = l0_q_all(Q.H.data(), Q.c.data(), p);
          const double flb = l0_con_lower_bound(P, q_all);
          CHECK(flb >= q_all && flb <= R.primal);
        }
      }
    }
  }
  CHECK(worst <= 1e-11);
  CHECK(polished >= total - 6);  // (a degenerate face -- the optimum b = 0 under equality rows -- keeps the splitting's point)
  printf("random problems: %d of %d polished, worst KKT violation %.3e, most sweeps %d\n", polished, total, worst, most);
}

static void test_pd_check_and_starved_solve() {
  // a duplicated column: not positive definite, refused; with a ridge it passes
  const int p = 3;
  double H[9] = {1.0, 1.0, 0.2, 1.0, 1.0, 0.2, 0.2, 0.2, 1.0}, c[3] = {1.0, 1.0, 0.5};
  CHECK(!l0_con_pd(H, c, p));
  H[0] += 0.01; H[4] += 0.01; H[8] += 0.01;
  CHECK(l0_con_pd(H, c, p));
  // one sweep is not enough where a row binds: unsettled, and the bound holds
  const Problem Q = random_problem(8, 4, 24, 0.02, true);
  int cols[8] = {0, 1, 2, 3, 4, 5, 6, 7};
  const L0ConProblem P1 = Q.view(1), P = Q.view();
  L0ConPoint full = l0_con_solve(P, cols, 8, HUGE_VAL);
  CHECK(full.outcome == 0 && l0_con_polish(P, cols, 8, full));
  const L0ConPoint one = l0_con_solve(P1, cols, 8, HUGE_VAL);
  CHECK(one.sweeps == 1 && (one.outcome == 2 || full.sweeps == 1) && one.bound <= full.primal);
  // a solve told to stop above a threshold below the optimum is rejected
  const L0ConPoint rej = l0_con_solve(P, cols, 8, full.primal - 0.5 * fabs(full.primal) - 1.0);
  CHECK(rej.outcome == 1);
}

int main() {
  test_shared_pieces();
  test_closed_forms();
  test_random_problems();
  test_pd_check_and_starved_solve();
  if (failures) {
    fprintf(stderr, "l0_con_host_test: %d failure(s)\n", failures);
    return 1;
  }
  printf("l0_con_host_test: ok\n");
  return 0;
}
