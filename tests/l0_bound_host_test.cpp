// CPU test of the exclusion bound of csrc/l0_host.hpp -- the host side of slm_solve_l0_xb and slm_solve_l0_xb_wide: P, bhat,
// kappa_1 and delta from l0_excl_plan, and the exclusion factor (L0ExclFactor on (P, bhat), the kernel's append) against a
// long-double Cholesky of H on all \ E.  H = Q diag(lambda) Q^T at 8, 33 and 64 columns, kappa from 1e1 to 1e12 in decades,
// bhat of a random scale, random exclusion orders (checked after every column, so single columns and groups of any size are
// both covered).  Prints the worst overshoot of the UNGUARDED fp64 increment 1/2 ssx over the long-double increment in units of
// kappa_1 2^-53 1/2 ssx: L0_XB_C is 16 times that figure, rounded up to a power of two.  (The rounding of q_all itself does not
// depend on E and scales with |q_all|: the second term of l0_excl_bound covers it, and the figure that includes it is printed too.)  Meant to run under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_l0_bound_cpu.py
// builds and runs it both plainly and sanitized).
#include <math.h>
#include <stdio.h>

#include <algorithm>
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

// a small generator of its own: the same numbers on every platform
static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {  // in (-1, 1)
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

struct Problem {
  int p;
  double kappa;
  std::vector<double> H, c;
};
// H = Q diag(lambda) Q^T, lambda geometric from 1 down to 1 / kappa, Q from a Gram-Schmidt of a random matrix (long double,
// then rounded); c = H bhat for a random bhat of size `scale`
static Problem make(int p, double kappa, double scale) {
  std::vector<long double> Q((size_t)p * p);
  for (auto& v : Q) v = uniform();
  for (int pass = 0; pass < 2; ++pass)
    for (int j = 0; j < p; ++j) {
      for (int k = 0; k < j; ++k) {
        long double d = 0.0L;
        for (int i = 0; i < p; ++i) d += Q[(size_t)i * p + j] * Q[(size_t)i * p + k];
        for (int i = 0; i < p; ++i) Q[(size_t)i * p + j] -= d * Q[(size_t)i * p + k];
      }
      long double nn = 0.0L;
      for (int i = 0; i < p; ++i) nn += Q[(size_t)i * p + j] * Q[(size_t)i * p + j];
      nn = sqrtl(nn);
      for (int i = 0; i < p; ++i) Q[(size_t)i * p + j] /= nn;
    }
  Problem R{p, kappa, std::vector<double>((size_t)p * p), std::vector<double>((size_t)p)};
  for (int a = 0; a < p; ++a)
    for (int b = 0; b <= a; ++b) {
      long double t = 0.0L;
      for (int k = 0; k < p; ++k) t += Q[(size_t)a * p + k] * Q[(size_t)b * p + k] * powl((long double)kappa, -(long double)k / (p - 1));
      R.H[(size_t)a * p + b] = R.H[(size_t)b * p + a] = (double)t;
    }
  std::vector<double> bhat((size_t)p);
  for (double& v : bhat) v = scale * uniform();
  for (int a = 0; a < p; ++a) {
    long double t = 0.0L;
    for (int b = 0; b < p; ++b) t += (long double)R.H[(size_t)a * p + b] * bhat[(size_t)b];
    R.c[(size_t)a] = (double)t;
  }
  return R;
}

// q on the columns `cols`: -1/2 c_S^T H_SS^-1 c_S by a Cholesky in long double
static long double truth(const Problem& P, const std::vector<int>& cols) {
  const int m = (int)cols.size();
  std::vector<long double> L((size_t)m * m, 0.0L), w((size_t)m);
  long double ss = 0.0L;
  for (int i = 0; i < m; ++i) {
    for (int j = 0; j <= i; ++j) {
      long double t = P.H[(size_t)cols[(size_t)i] * P.p + cols[(size_t)j]];
      for (int k = 0; k < j; ++k) t -= L[(size_t)i * m + k] * L[(size_t)j * m + k];
      L[(size_t)i * m + j] = i == j ? sqrtl(t) : t / L[(size_t)j * m + j];
    }
    long double t = P.c[(size_t)cols[(size_t)i]];
    for (int k = 0; k < i; ++k) t -= L[(size_t)i * m + k] * w[(size_t)k];
    w[(size_t)i] = t / L[(size_t)i * m + i];
    ss += w[(size_t)i] * w[(size_t)i];
  }
  return -0.5L * ss;
}

static double worst_overshoot = 0.0, worst_kappa = 0.0, worst_with_q_all = 0.0;
static int worst_p = 0;
static long long bounds_checked = 0, fell_back = 0;

// One exclusion order on one problem: after every column the guarded bound is below the truth (check 1), the increment is
// within 1e-6 of the true one while kappa <= 1e6 (check 2: delta is L0_XB_C kappa_1 2^-53 <= 256 * 33 kappa 2^-53 < 1e-6 there at up to 33 columns,
// and the second term is 1e-10 of |q_all| + 1/2 ssx), the bound never falls along the path (check 4), and a factor that
// skipped one column or holds only CAP2 rows is never above the full one's unguarded value and below the truth (check 5).
static void sweep(const Problem& P, const L0ExclPlan& plan) {
  const int p = P.p;
  const double q_all = l0_q_all(P.H.data(), P.c.data(), p);
  std::vector<int> every((size_t)p);
  for (int j = 0; j < p; ++j) every[(size_t)j] = j;
  const long double q_all_true = truth(P, every);
  std::vector<int> order((size_t)p);
  for (int j = 0; j < p; ++j) order[(size_t)j] = j;
  for (int j = p - 1; j > 0; --j) std::swap(order[(size_t)j], order[(size_t)((uniform() + 1.0) * 0.5 * (j + 1)) % (size_t)(j + 1)]);
  const int skip = order[(size_t)((uniform() + 1.0) * 0.5 * p) % (size_t)p];
  constexpr int CAP2 = 5;
  auto full = std::make_unique<L0ExclFactor>(plan.P.data(), plan.bhat.data(), p);
  auto skipped = std::make_unique<L0ExclFactor>(plan.P.data(), plan.bhat.data(), p);
  L0FactorT<CAP2> capped(plan.P.data(), plan.bhat.data(), p);
  std::vector<bool> out((size_t)p, false);
  double last = l0_excl_bound(q_all, 0.0, plan.delta);
  CHECK(last <= q_all);
  for (int step = 0; step < p - 1; ++step) {  // (one column always stays: the empty remainder has q = 0 exactly)
    const int j = order[(size_t)step];
    out[(size_t)j] = true;
    (void)full->push(j);
    if (j != skip) (void)skipped->push(j);
    (void)capped.push(j);
    std::vector<int> rest;
    for (int k = 0; k < p; ++k)
      if (!out[(size_t)k]) rest.push_back(k);
    const long double q_true = truth(P, rest);
    const double unguarded = q_all + 0.5 * full->ss, guarded = l0_excl_bound(q_all, full->ss, plan.delta);
    ++bounds_checked;
    if (full->ss > 0.0) {
      const double over = (double)((0.5L * full->ss - (q_true - q_all_true)) / (long double)(plan.kappa1 * 0x1p-53 * 0.5 * full->ss));
      const double over_all = (double)(((long double)unguarded - q_true) / (long double)(plan.kappa1 * 0x1p-53 * 0.5 * full->ss));
      worst_with_q_all = fmax(worst_with_q_all, over_all);
      if (over > worst_overshoot) {
        worst_overshoot = over;
        worst_kappa = P.kappa;
        worst_p = p;
      }
    }
    CHECK((long double)guarded <= q_true);  // check 1
    if (P.kappa <= 1e6) {                    // check 2
      const long double inc_true = q_true - (long double)q_all, inc = (long double)guarded - (long double)q_all;
      CHECK(fabsl(inc - inc_true) <= 1e-6L * inc_true + 1.01e-10L * (fabsl((long double)q_all) + inc_true));
    }
    CHECK(guarded >= last);  // check 4
    last = guarded;
    // check 5: a sub-collection of E only lowers the bound, and stays valid
    const double g_skip = l0_excl_bound(q_all, skipped->ss, plan.delta), g_cap = l0_excl_bound(q_all, capped.ss, plan.delta);
    CHECK(g_skip <= unguarded && g_cap <= unguarded);
    CHECK((long double)g_skip <= q_true && (long double)g_cap <= q_true);
    CHECK(capped.m <= CAP2);
  }
  CHECK(capped.m == CAP2 && capped.overflow);
}

static void test_sweep() {
  for (int p : {8, 33, 64})
    for (int dec = 1; dec <= 12; ++dec) {
      const double kappa = pow(10.0, dec);
      for (int rep = 0; rep < 3; ++rep) {
        const Problem P = make(p, kappa, pow(10.0, 3.0 * uniform()));
        const L0ExclPlan plan = l0_excl_plan(P.H.data(), P.c.data(), p);
        CHECK(plan.reason == 0 || (plan.reason == 2 && plan.delta >= 0.5));  // (check 3 in the wild: kappa_1 near 2^52 / L0_XB_C)
        if (plan.reason != 0) {
          ++fell_back;
          continue;
        }
        CHECK(plan.kappa1 >= 0.99 * kappa && plan.kappa1 <= 1.01 * p * kappa);  // (kappa_2 <= kappa_1 <= p kappa_2)
        CHECK(plan.delta == l0_excl_delta(plan.kappa1) && plan.delta < 0.5);
        // P is the inverse and bhat the minimiser: H P = I and H bhat = c to the conditioning
        double worst = 0.0;
        for (int a = 0; a < p; ++a)
          for (int b = 0; b < p; ++b) {
            long double t = 0.0L;
            for (int k = 0; k < p; ++k) t += (long double)P.H[(size_t)a * p + k] * plan.P[(size_t)k * p + b];
            worst = fmax(worst, fabs((double)t - (a == b ? 1.0 : 0.0)));
          }
        CHECK(worst <= 64.0 * plan.kappa1 * 0x1p-53);
        for (int order = 0; order < 4; ++order) sweep(P, plan);
      }
    }
}

// check 3: the fallback flag is raised once delta >= 1/2, and by an H that is not positive definite under the pivot rule
static void test_fallback() {
  for (double small : {1e-12, 1e-13, 1e-14, 1e-15, 1e-16}) {
    const std::vector<double> H = {1.0, 0.0, 0.0, small}, c = {1.0, small};
    const L0ExclPlan plan = l0_excl_plan(H.data(), c.data(), 2);
    CHECK(fabs(plan.kappa1 * small - 1.0) <= 1e-14);
    CHECK((plan.reason == 2) == (L0_XB_C * plan.kappa1 * 0x1p-53 >= 0.5));
    CHECK(plan.reason == 0 || plan.reason == 2);
  }
  CHECK(l0_excl_plan(std::vector<double>{1.0, 0.0, 0.0, 1e-16}.data(), std::vector<double>{1.0, 0.0}.data(), 2).reason == 2);
  CHECK(l0_excl_plan(std::vector<double>{1.0, 0.0, 0.0, 1e-3}.data(), std::vector<double>{1.0, 0.0}.data(), 2).reason == 0);
  // a duplicated column: not positive definite
  const std::vector<double> D = {2.0, 1.0, 2.0, 1.0, 3.0, 1.0, 2.0, 1.0, 2.0}, c3 = {1.0, 1.0, 1.0};
  const L0ExclPlan dup = l0_excl_plan(D.data(), c3.data(), 3);
  CHECK(dup.reason == 1 && dup.P.empty());
  // the guard itself: below the unguarded value, equal to q_all's own guard with nothing excluded
  CHECK(l0_excl_bound(-2.0, 0.0, 0.25) == -2.0 - 2e-10);
  CHECK(l0_excl_bound(-2.0, 1.0, 0.25) == -2.0 + 0.5 * 0.75 - 1e-10 * 2.5);
  static_assert(l0_excl_bound(-1.0, 2.0, 0.0) < 0.0 + 1e-300, "constexpr: the device code calls this very function");
  static_assert(L0_XCAP == 32 || L0_XCAP == 64, "the two capacities that were measured");
}

int main() {
  test_sweep();
  test_fallback();
  printf("worst overshoot of the unguarded increment 1/2 ssx: %.4g units of kappa_1 2^-53 1/2 ssx (p = %d, kappa = %.0e; %lld bounds, %lld "
         "problems fell back); with the rounding of q_all itself, which the 1e-10 term covers: %.4g; L0_XB_C = %g\n",
         worst_overshoot, worst_p, worst_kappa, bounds_checked, fell_back, worst_with_q_all, L0_XB_C);
  CHECK(L0_XB_C >= 16.0 * worst_overshoot);
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("l0_bound_host_test: ok\n");
  return 0;
}
