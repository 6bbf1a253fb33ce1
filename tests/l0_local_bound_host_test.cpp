// CPU test of what the local bound adds to csrc/l0_host.hpp (slm_solve_l0_local_bound in engine_l0.hip calls THESE functions and
// l0_local_bound_kernel shares their arithmetic): the coordinate step against a scan of its own objective, phi* against phi, the
// wave-ordered sum, the twin l0_bound_solve on cases of its own (a bound for every stopping reason, the certificate rebuilt from u
// alone, dead columns counted) and on the cases tests/test_l0_local_bound_cpu.py exports from the numpy restatement -- u, sweeps,
// status, bound and relaxed value BIT FOR BIT -- and every refusal of l0_bound_check in its order.  A stand-alone program, meant to
// run under AddressSanitizer and UndefinedBehaviorSanitizer (the test builds and runs it both plainly and sanitized).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <limits>
#include <vector>

#include "../sparse-lm_amd/csrc/l0_host.hpp"

using namespace slm;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("FAILED line %d: %s\n", __LINE__, #cond);               \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static double rnd(unsigned long long& s) {  // uniform in (-1, 1)
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (double)((s >> 11) & ((1ull << 53) - 1)) / (double)(1ull << 52) - 1.0;
}

// a Gram of n rows on p columns (AR(1) columns, correlation rho), and c = X^T y / n for a y built from three columns
static void draw(int n, int p, double rho, unsigned long long seed, std::vector<double>& G, std::vector<double>& c) {
  std::vector<double> X((size_t)n * p), y((size_t)n, 0.0);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < p; ++j) {
      const double z = rnd(seed);
      X[(size_t)i * p + j] = j == 0 ? z : rho * X[(size_t)i * p + j - 1] + sqrt(1.0 - rho * rho) * z;
    }
  for (int i = 0; i < n; ++i) y[(size_t)i] = X[(size_t)i * p] - X[(size_t)i * p + p / 2] + X[(size_t)i * p + p - 1] + 0.3 * rnd(seed);
  G.assign((size_t)p * p, 0.0);
  c.assign((size_t)p, 0.0);
  for (int a = 0; a < p; ++a) {
    for (int b = 0; b < p; ++b) {
      double s = 0.0;
      for (int i = 0; i < n; ++i) s += X[(size_t)i * p + a] * X[(size_t)i * p + b];
      G[(size_t)a * p + b] = s / n;
    }
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += X[(size_t)i * p + a] * y[(size_t)i];
    c[(size_t)a] = s / n;
  }
}

// L(u) from the definition: t = c - G u by plain products, no shared code but l0_lb_conj
static double bound_at(const std::vector<double>& G, const std::vector<double>& c, int p, double alpha, double eta, double M, const double* u) {
  double quad = 0.0, sum = 0.0;
  for (int j = 0; j < p; ++j) {
    double gu = 0.0;
    for (int k = 0; k < p; ++k) gu += G[(size_t)j * p + k] * u[k];
    quad += u[j] * gu;
    sum += l0_lb_conj(c[(size_t)j] - gu, alpha, eta, M);
  }
  return -0.5 * quad - sum;
}

static const double ETAS[3] = {0.0, 0.01, 1.0}, BIG_MS[2] = {0.7, 100.0}, ALPHAS[3] = {1e-3, 0.1, 0.5};

static void test_coordinate_and_conjugate() {
  for (double eta : ETAS)
    for (double M : BIG_MS)
      for (double alpha : ALPHAS) {
        const L0LbCell cell = l0_lb_cell(alpha, eta, M);
        CHECK(cell.lam >= 0.0 && cell.tauc <= M);
        // phi is continuous where its pieces meet, and phi(M) is the cost of a coordinate at the box
        if (cell.tauc < M) CHECK(fabs(cell.lam * cell.tauc - (eta * cell.tauc * cell.tauc + alpha)) <= 1e-14 * (alpha + 1.0));
        for (double a : {0.3, 1.0, 4.0})
          for (int k = -40; k <= 40; ++k) {
            const double s = 0.11 * k * (k % 3 == 0 ? 3.0 : 1.0);
            const double b = l0_lb_coord(s, a, eta, cell.lam, cell.tauc, M);
            CHECK(fabs(b) <= M && (b == 0.0 || (b > 0.0) == (s > 0.0)));
            CHECK(l0_lb_coord(-s, a, eta, cell.lam, cell.tauc, M) == -b);
            // no point of a fine scan of the box lies below it
            const double at_b = 0.5 * a * b * b - s * b + l0_lb_phi(b, alpha, eta, cell.lam, cell.tauc);
            for (int g = -2000; g <= 2000; ++g) {
              const double x = M * g / 2000.0;
              CHECK(at_b <= 0.5 * a * x * x - s * x + l0_lb_phi(x, alpha, eta, cell.lam, cell.tauc) + 1e-12 * (1.0 + fabs(at_b)));
            }
          }
        // Fenchel-Young: t b - phi(b) <= phi*(t) on the box, with equality reached on a fine scan
        for (int k = -30; k <= 30; ++k) {
          const double t = 0.07 * k * (eta > 0.0 ? 1.0 + 2.0 * eta * M : 1.0);
          const double conj = l0_lb_conj(t, alpha, eta, M);
          double best = 0.0;
          for (int g = -4000; g <= 4000; ++g) {
            const double x = M * g / 4000.0;
            best = fmax(best, t * x - l0_lb_phi(x, alpha, eta, cell.lam, cell.tauc));
          }
          CHECK(best <= conj + 1e-12 * (1.0 + conj));
          CHECK(conj - best <= 1e-3 * (1.0 + conj));  // (the scan's step: eta (M / 8000)^2 at most, 1.6e-4 at eta = 1, M = 100)
        }
      }
  CHECK(!l0_lb_changed(std::numeric_limits<double>::quiet_NaN(), 1.0) && l0_lb_changed(1.0, 2.0) && !l0_lb_changed(0.0, -0.0));
  CHECK(l0_lb_closed(1.0, 1.0 - 1e-10, 0.1, 1e-9) && !l0_lb_closed(1.0, 1.0 - 1e-8, 0.1, 1e-9) && !l0_lb_closed(1.0, 0.5, 0.1, 0.0));
}

static void test_wave_sum() {
  unsigned long long seed = 7;
  double lanes[64], plain = 0.0;
  for (int i = 0; i < 64; ++i) {
    lanes[i] = rnd(seed);
    plain += lanes[i];
  }
  CHECK(fabs(l0_lb_wave_sum(lanes) - plain) <= 1e-14);
  // the butterfly's own order on a case where order shows: pairs (i, i ^ 32) first
  for (int i = 0; i < 64; ++i) lanes[i] = 0.0;
  lanes[0] = 1.0;
  lanes[32] = 1e-16;
  lanes[1] = -1.0;
  lanes[33] = 1e-16;
  CHECK(l0_lb_wave_sum(lanes) == (1.0 + 1e-16) + (-1.0 + 1e-16));
}

static void test_twin() {
  unsigned long long seed = 99;
  for (int p : {1, 7, 63, 64, 65, 130}) {
    std::vector<double> G, c;
    draw(40, p, 0.7, 1000 + (unsigned long long)p, G, c);
    std::vector<double> u((size_t)p), u1((size_t)p), start((size_t)p), zero((size_t)p, 0.0);
    for (double eta : ETAS)
      for (double M : BIG_MS)
        for (double alpha : {1e-3, 0.1}) {
          const L0LbResult R = l0_bound_solve(G.data(), (size_t)p, c.data(), p, alpha, eta, M, nullptr, 400, 1e-9, u.data());
          CHECK(R.sweeps >= 1 && R.sweeps <= 400 && (R.status == 0 || (R.status == L0_LS_SWEEPS_OUT && R.sweeps == 400)));
          // the certificate: L at the returned u by plain products (or L(0) where that is higher), and never above the relaxation
          const double at_u = bound_at(G, c, p, alpha, eta, M, u.data()), at_0 = bound_at(G, c, p, alpha, eta, M, zero.data());
          double quad = 0.0;
          for (int j = 0; j < p; ++j)
            for (int k = 0; k < p; ++k) quad += 0.5 * u[(size_t)j] * G[(size_t)j * p + k] * u[(size_t)k];
          const double tol = 1e-10 * fmax(fmax(fabs(R.lower), alpha), quad);
          CHECK(fabs(R.lower - fmax(at_u, at_0)) <= tol);
          CHECK(R.lower <= R.primal + tol && R.lower <= tol);  // (F(0) = 0 is feasible)
          if (R.status == 0) CHECK(R.primal - R.lower <= 2e-9 * fmax(fabs(R.primal), alpha));
          for (int j = 0; j < p; ++j) CHECK(fabs(u[(size_t)j]) <= M);
          // one sweep is a bound too, and the status says that the relaxation is open (unless one sweep closed it to the last bit)
          const L0LbResult R1 = l0_bound_solve(G.data(), (size_t)p, c.data(), p, alpha, eta, M, nullptr, 1, 0.0, u1.data());
          CHECK(R1.sweeps == 1 && R1.lower <= R.primal + tol);
          CHECK(R1.status == L0_LS_SWEEPS_OUT || R1.primal - R1.lower <= tol);
          CHECK(fabs(R1.lower - fmax(bound_at(G, c, p, alpha, eta, M, u1.data()), at_0)) <= tol);
          // a start outside the box is clipped into it; where both runs close the relaxation they meet
          for (int j = 0; j < p; ++j) start[(size_t)j] = 3.0 * M * rnd(seed);
          const L0LbResult R2 = l0_bound_solve(G.data(), (size_t)p, c.data(), p, alpha, eta, M, start.data(), 400, 1e-9, u1.data());
          CHECK(R2.lower >= at_0 - tol);
          if (R.status == 0 && R2.status == 0) CHECK(fabs(R2.lower - R.lower) <= 1e-8 * fmax(fabs(R.primal), alpha));
        }
  }
  // a dead column (zero diagonal, a made-up c there) keeps u = 0 and is still counted in the sum
  {
    const int p = 5;
    std::vector<double> G, c;
    draw(30, p, 0.5, 5, G, c);
    for (int k = 0; k < p; ++k) G[(size_t)2 * p + k] = G[(size_t)k * p + 2] = 0.0;
    c[2] = 0.9;
    std::vector<double> u((size_t)p), start((size_t)p, 0.25);
    const double alpha = 0.05, eta = 0.1, M = 2.0;
    const L0LbResult R = l0_bound_solve(G.data(), (size_t)p, c.data(), p, alpha, eta, M, start.data(), 200, 1e-9, u.data());
    CHECK(u[2] == 0.0);
    CHECK(fabs(R.lower - bound_at(G, c, p, alpha, eta, M, u.data())) <= 1e-12);
    std::vector<double> G4, c4, u4(4);
    for (int a = 0; a < p; ++a) {
      if (a == 2) continue;
      c4.push_back(c[(size_t)a]);
      for (int b = 0; b < p; ++b)
        if (b != 2) G4.push_back(G[(size_t)a * p + b]);
    }
    const L0LbResult R4 = l0_bound_solve(G4.data(), 4, c4.data(), 4, alpha, eta, M, nullptr, 200, 1e-9, u4.data());
    CHECK(fabs((R4.lower - l0_lb_conj(0.9, alpha, eta, M)) - R.lower) <= 1e-8);  // the column's term: it cannot be fitted, it is paid for
  }
  // alpha = 0: the relaxation IS the box-constrained ridge problem, so the bound is its optimum
  {
    const int p = 6;
    std::vector<double> G, c, u((size_t)p);
    draw(30, p, 0.5, 11, G, c);
    const double eta = 0.05, M = 0.4;
    const L0LbResult R = l0_bound_solve(G.data(), (size_t)p, c.data(), p, 0.0, eta, M, nullptr, 2000, 1e-12, u.data());
    CHECK(R.status == 0);
    double F = 0.0;
    for (int j = 0; j < p; ++j) {
      F += eta * u[(size_t)j] * u[(size_t)j] - c[(size_t)j] * u[(size_t)j];
      for (int k = 0; k < p; ++k) F += 0.5 * u[(size_t)j] * G[(size_t)j * p + k] * u[(size_t)k];
    }
    CHECK(fabs(F - R.lower) <= 1e-10 * fabs(F));
  }
}

static void test_check() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  double al[3] = {0.1, 0.2, 0.3}, et[3] = {0.0, 0.1, 1.0}, st[6] = {0, 0, 0, 0, 0, 0};
  long long which = -1;
  CHECK(l0_bound_check(3, al, et, 1.0, st, 2, 1e-9, true, false, &which) == L0_LB_OK);
  CHECK(l0_bound_check(3, al, et, 0.0, nullptr, 1024, 0.0, true, false) == L0_LB_OK);
  CHECK(l0_bound_check(3, nullptr, et, 1.0, st, 2, 1e-9, true, false) == L0_LB_NULL);
  CHECK(l0_bound_check(3, al, nullptr, 1.0, st, 2, 1e-9, true, false) == L0_LB_NULL);
  CHECK(l0_bound_check(0, al, et, -1.0, st, 2000, -1.0, false, true) == L0_LB_CELLS);  // the order: the first refusal wins
  CHECK(l0_bound_check(L0_LS_MAX_PROBLEMS + 1, al, et, -1.0, st, 2000, -1.0, false, true) == L0_LB_PROBLEMS);
  CHECK(l0_bound_check(3, al, et, -1.0, st, 2000, -1.0, false, true) == L0_LB_BIG_M);
  CHECK(l0_bound_check(3, al, et, nan, st, 2, 1e-9, true, false) == L0_LB_BIG_M);
  al[1] = -0.1;
  et[0] = nan;
  CHECK(l0_bound_check(3, al, et, 1.0, st, 2000, -1.0, false, true, &which) == L0_LB_ETA && which == 0);
  et[0] = 0.0;
  CHECK(l0_bound_check(3, al, et, 1.0, st, 2000, -1.0, false, true, &which) == L0_LB_ALPHA && which == 1);
  al[1] = inf;
  CHECK(l0_bound_check(3, al, et, 1.0, st, 2, 1e-9, true, false, &which) == L0_LB_ALPHA && which == 1);
  al[1] = 0.2;
  et[2] = -1.0;
  CHECK(l0_bound_check(3, al, et, 1.0, st, 2, 1e-9, true, false, &which) == L0_LB_ETA && which == 2);
  et[2] = 1.0;
  CHECK(l0_bound_check(3, al, et, 1.0, st, 2000, -1e-300, false, true) == L0_LB_GAP_TOL);
  CHECK(l0_bound_check(3, al, et, 1.0, st, 2, nan, true, false) == L0_LB_GAP_TOL);
  st[4] = nan;
  CHECK(l0_bound_check(3, al, et, 1.0, st, 1025, 1e-9, false, true) == L0_LB_WIDTH);
  CHECK(l0_bound_check(3, al, et, 1.0, st, 2, 1e-9, false, true, &which) == L0_LB_START && which == 4);
  st[4] = -inf;
  CHECK(l0_bound_check(3, al, et, 1.0, st, 2, 1e-9, true, false, &which) == L0_LB_START && which == 4);
  st[4] = 1e300;  // (outside the box: clipped, not refused)
  CHECK(l0_bound_check(3, al, et, 1.0, st, 2, 1e-9, false, true) == L0_LB_GROUPS);
  CHECK(l0_bound_check(3, al, et, 1.0, st, 2, 1e-9, true, true) == L0_LB_SHARDED);
  CHECK(l0_bound_check(3, al, et, 1.0, st, 2, 1e-9, true, false) == L0_LB_OK);
}

// The exported cases: per case a line `p alpha eta M has_start max_sweeps gap_tol sweeps status lower primal`, then p rows of G, c,
// the start where there is one, and the restatement's u.
static int test_exported(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) {
    printf("cannot open %s\n", path);
    ++failures;
    return 0;
  }
  int count = 0, p = 0, has_start = 0, max_sweeps = 0, sweeps = 0, status = 0;
  double alpha = 0.0, eta = 0.0, M = 0.0, gap_tol = 0.0, lower = 0.0, primal = 0.0;
  while (fscanf(f, "%d %lf %lf %lf %d %d %lf %d %d %lf %lf", &p, &alpha, &eta, &M, &has_start, &max_sweeps, &gap_tol, &sweeps, &status, &lower,
                &primal) == 11) {
    std::vector<double> G((size_t)p * p), c((size_t)p), start((size_t)p), want((size_t)p), u((size_t)p);
    bool ok = true;
    for (double& v : G) ok = ok && fscanf(f, "%lf", &v) == 1;
    for (double& v : c) ok = ok && fscanf(f, "%lf", &v) == 1;
    for (double& v : start) ok = ok && (!has_start || fscanf(f, "%lf", &v) == 1);
    for (double& v : want) ok = ok && fscanf(f, "%lf", &v) == 1;
    CHECK(ok);
    if (!ok) break;
    const L0LbResult R = l0_bound_solve(G.data(), (size_t)p, c.data(), p, alpha, eta, M, has_start ? start.data() : nullptr, max_sweeps, gap_tol,
                                        u.data());
    bool same = R.sweeps == sweeps && R.status == status && R.lower == lower && R.primal == primal;
    for (int j = 0; j < p; ++j) same = same && u[(size_t)j] == want[(size_t)j];
    if (!same) {
      printf("case %d (p %d alpha %g eta %g M %g start %d): sweeps %d / %d status %d / %d lower %.17g / %.17g primal %.17g / %.17g\n", count, p,
             alpha, eta, M, has_start, R.sweeps, sweeps, R.status, status, R.lower, lower, R.primal, primal);
      ++failures;
    }
    ++count;
  }
  fclose(f);
  return count;
}

int main(int argc, char** argv) {
  test_coordinate_and_conjugate();
  test_wave_sum();
  test_twin();
  test_check();
  if (argc > 1) printf("exported: %d cases\n", test_exported(argv[1]));
  if (failures) {
    printf("l0_local_bound_host_test: %d FAILED\n", failures);
    return 1;
  }
  printf("l0_local_bound_host_test: ok\n");
  return 0;
}
