// CPU test of the wide mode of csrc/l0_host.hpp -- the host side of slm_solve_l0_wide and slm_solve_l0_profile_wide: q_all on
// 100 columns (a factor of more than 64 rows, two dependent columns among them) against a long-double Cholesky; the greedy
// seed, which stops at 64 independent columns; the two-word masks with the order of the 128-bit integer; l0_support_of on a
// support whose columns all lie beyond index 64; and the capacity rule.  Meant to run under AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_l0_wide_cpu.py builds and runs it both plainly and sanitized).
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

// a small generator of its own: the same numbers on every platform
static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static double uniform() {  // in (-1, 1)
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) / 9007199254740992.0 * 2.0 - 1.0;
}

// X: n x p with the columns `dep` (each the sum of the two columns before it) dependent; H = X^T X / n, c = X^T y / n
struct Problem {
  int n, p;
  std::vector<double> X, y, H, c;
};
static Problem make(int n, int p, const std::vector<int>& dep) {
  Problem P{n, p, std::vector<double>((size_t)n * p), std::vector<double>((size_t)n), std::vector<double>((size_t)p * p), std::vector<double>((size_t)p)};
  for (double& v : P.X) v = uniform();
  for (int j : dep)
    for (int i = 0; i < n; ++i) P.X[(size_t)i * p + j] = P.X[(size_t)i * p + j - 1] + P.X[(size_t)i * p + j - 2];
  for (int i = 0; i < n; ++i) {
    double t = 0.3 * uniform();
    for (int j = 0; j < p; j += 7) t += (1.0 + 0.1 * j) * P.X[(size_t)i * p + j];
    P.y[(size_t)i] = t;
  }
  for (int a = 0; a < p; ++a) {
    long double s = 0.0L;
    for (int i = 0; i < n; ++i) s += (long double)P.X[(size_t)i * p + a] * P.y[(size_t)i];
    P.c[(size_t)a] = (double)(s / n);
    for (int b = 0; b < p; ++b) {
      long double t = 0.0L;
      for (int i = 0; i < n; ++i) t += (long double)P.X[(size_t)i * p + a] * P.X[(size_t)i * p + b];
      P.H[(size_t)a * p + b] = (double)(t / n);
    }
  }
  return P;
}

// -1/2 c_S^T H_SS^-1 c_S on the columns `cols` (independent) by a Cholesky in long double
static double reference_value(const Problem& P, const std::vector<int>& cols) {
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
  return (double)(-0.5L * ss);
}

static void test_masks() {
  L0Mask128 a = l0m_none<L0Mask128>();
  CHECK(a.lo == 0 && a.hi == 0);
  for (int g : {0, 1, 63, 64, 65, 127}) {
    CHECK(!l0m_test(a, g));
    l0m_set(a, g);
    CHECK(l0m_test(a, g));
  }
  CHECK(a.lo == (0x8000000000000003ull) && a.hi == (0x8000000000000003ull));
  l0m_clear(a, 64);
  l0m_clear(a, 63);
  CHECK(a.lo == 3ull && a.hi == 0x8000000000000002ull && !l0m_test(a, 64) && !l0m_test(a, 63) && l0m_test(a, 65));
  // the bits below g, on both sides of the word boundary
  CHECK(l0m_below<L0Mask128>(0).lo == 0 && l0m_below<L0Mask128>(0).hi == 0);
  CHECK(l0m_below<L0Mask128>(1).lo == 1 && l0m_below<L0Mask128>(63).lo == (~0ull >> 1) && l0m_below<L0Mask128>(63).hi == 0);
  CHECK(l0m_below<L0Mask128>(64).lo == ~0ull && l0m_below<L0Mask128>(64).hi == 0);
  CHECK(l0m_below<L0Mask128>(65).lo == ~0ull && l0m_below<L0Mask128>(65).hi == 1);
  CHECK(l0m_below<L0Mask128>(127).hi == (~0ull >> 1) && l0m_below<L0Mask128>(128).hi == ~0ull && l0m_below<L0Mask128>(128).lo == ~0ull);
  for (int g : {0, 1, 17, 63, 64}) CHECK(l0m_below<unsigned long long>(g) == l0m_below<L0Mask128>(g).lo);
  // the order of the 128-bit integer: the high word first, then the low one
  const L0Mask128 low_big{~0ull, 0ull}, high_small{0ull, 1ull}, high_small2{5ull, 1ull};
  CHECK(l0m_less(low_big, high_small) && !l0m_less(high_small, low_big));
  CHECK(l0m_less(high_small, high_small2) && !l0m_less(high_small2, high_small) && !l0m_less(high_small, high_small));
  CHECK(l0m_less(l0m_none<L0Mask128>(), l0m_ones<L0Mask128>()) && !l0m_less(l0m_ones<L0Mask128>(), l0m_ones<L0Mask128>()));
  CHECK(l0m_less(3ull, 4ull) && !l0m_less(4ull, 4ull));
  // a needs something that b lacks -- in either word
  L0Mask128 need = l0m_none<L0Mask128>(), have = l0m_none<L0Mask128>();
  l0m_set(need, 3);
  l0m_set(need, 70);
  l0m_set(have, 3);
  CHECK(l0m_any_outside(need, have));  // (an engine that ignored the high word would say no)
  l0m_set(have, 70);
  l0m_set(have, 100);
  CHECK(!l0m_any_outside(need, have) && l0m_any_outside(have, need));
  CHECK(!l0m_any_outside(l0m_and(need, l0m_below<L0Mask128>(70)), l0m_below<L0Mask128>(4)));  // only bit 3 lies below 70
  L0Mask128 u = need;
  l0m_or(u, L0Mask128{1ull << 9, 1ull << 9});
  CHECK(l0m_test(u, 9) && l0m_test(u, 73) && l0m_test(u, 3) && l0m_test(u, 70));
  CHECK(l0m_any_outside(5ull, 4ull) && !l0m_any_outside(4ull, 5ull) && l0m_and(6ull, 3ull) == 2ull);
}

static void test_q_all_on_100_columns() {
  const std::vector<int> dep = {40, 90};  // each the sum of the two columns before it
  const Problem P = make(240, 100, dep);
  std::vector<int> indep;
  for (int j = 0; j < 100; ++j)
    if (j != 40 && j != 90) indep.push_back(j);
  const double want = reference_value(P, indep), got = l0_q_all(P.H.data(), P.c.data(), 100);
  CHECK(fabs(got - want) <= 1e-11 * fabs(want));
  // the narrow branch of the same function is the 64-row factor
  const Problem Q = make(120, 30, {});
  std::vector<int> all30;
  for (int j = 0; j < 30; ++j) all30.push_back(j);
  L0Factor f(Q.H.data(), Q.c.data(), 30);
  for (int j = 0; j < 30; ++j) CHECK(f.push(j));
  CHECK(l0_q_all(Q.H.data(), Q.c.data(), 30) == -0.5 * f.ss && !f.overflow);
  CHECK(fabs(-0.5 * f.ss - reference_value(Q, all30)) <= 1e-12 * fabs(f.ss));
  // the factor with a capacity: 100 rows take 98 independent columns, 64 rows refuse the 65th and say so
  L0FactorT<L0_WIDE_PMAX> big(P.H.data(), P.c.data(), 100);
  for (int j = 0; j < 100; ++j) CHECK(big.push(j) == (j != 40 && j != 90));
  CHECK(big.m == 98 && !big.overflow);
  L0Factor small(P.H.data(), P.c.data(), 100);
  int taken = 0;
  for (int j = 0; j < 70; ++j) taken += small.push(j) ? 1 : 0;
  CHECK(taken == 64 && small.m == 64 && small.overflow);  // (column 40 is dependent: 64 rows are full after column 64)
  const double ss64 = small.ss;
  small.pop_to(10);
  CHECK(!small.overflow && small.m == 10 && small.ss < ss64);
}

static void test_support_beyond_column_64() {
  const Problem P = make(240, 100, {90});
  std::vector<int> gstart;  // 25 groups of four columns
  for (int g = 0; g <= 25; ++g) gstart.push_back(4 * g);
  L0Mask128 mask = l0m_none<L0Mask128>();
  l0m_set(mask, 17);  // columns 68 .. 71
  l0m_set(mask, 22);  // columns 88 .. 91, column 90 dependent
  l0m_set(mask, 24);  // columns 96 .. 99
  std::vector<double> beta(100, 1.0);
  bool over = true;
  const double v = l0_support_of(P.H.data(), P.c.data(), 100, gstart, mask, HUGE_VAL, true, beta.data(), &over);
  const std::vector<int> cols = {68, 69, 70, 71, 88, 89, 91, 96, 97, 98, 99};
  CHECK(!over && fabs(v - reference_value(P, cols)) <= 1e-12 * fabs(v));
  int nonzero = 0;
  for (int j = 0; j < 100; ++j) nonzero += beta[(size_t)j] != 0.0 ? 1 : 0;
  CHECK(nonzero == 11 && beta[90] == 0.0 && beta[0] == 0.0 && beta[67] == 0.0 && beta[68] != 0.0);
  // the value is the objective of the coefficients: 1/2 b^T H b - c^T b
  double at = 0.0;
  for (int a : cols) {
    double t = 0.0;
    for (int b : cols) t += P.H[(size_t)a * 100 + b] * beta[(size_t)b];
    at += beta[(size_t)a] * (0.5 * t - P.c[(size_t)a]);
  }
  CHECK(fabs(at - v) <= 1e-11 * fabs(v));
  // inside a binding box the coefficients stay inside it and the value rises
  double top = 0.0;
  for (int a : cols) top = fmax(top, fabs(beta[(size_t)a]));
  std::vector<double> boxed(100);
  const double vb = l0_support_of(P.H.data(), P.c.data(), 100, gstart, mask, 0.5 * top, true, boxed.data());
  CHECK(vb > v);
  for (int j = 0; j < 100; ++j) CHECK(fabs(boxed[(size_t)j]) <= 0.5 * top);
  // one word and two words agree where both apply
  std::vector<double> b1(100), b2(100);
  const double v1 = l0_support(P.H.data(), P.c.data(), 100, gstart, (1ull << 3) | (1ull << 20), HUGE_VAL, true, b1.data());
  L0Mask128 m2 = l0m_none<L0Mask128>();
  l0m_set(m2, 3);
  l0m_set(m2, 20);
  CHECK(v1 == l0_support_of(P.H.data(), P.c.data(), 100, gstart, m2, HUGE_VAL, true, b2.data()) && b1 == b2);
  // more than 64 independent columns: reported
  (void)l0_support_of(P.H.data(), P.c.data(), 100, gstart, l0m_below<L0Mask128>(25), HUGE_VAL, false, b2.data(), &over);
  CHECK(over);
}

static void test_greedy_stops_at_capacity() {
  const Problem P = make(240, 100, {});
  std::vector<int> gstart;  // ten groups of ten columns: six fit the 64 rows, a seventh does not
  for (int g = 0; g <= 10; ++g) gstart.push_back(10 * g);
  const std::vector<L0Mask128> none(10, l0m_none<L0Mask128>());
  std::vector<double> beta(100);
  int visits = 0, largest = 0;
  bool any_over = false;
  double last = 0.0;
  l0_greedy(P.H.data(), P.c.data(), 100, gstart, none, 10,
            [&](L0Mask128 mask) {
              bool over = false;
              const double v = l0_support_of(P.H.data(), P.c.data(), 100, gstart, mask, HUGE_VAL, false, beta.data(), &over);
              any_over = any_over || over;
              return v;
            },
            [&](int size, L0Mask128 mask, double value) {
              int bits = 0;
              for (int g = 0; g < 10; ++g) bits += l0m_test(mask, g) ? 1 : 0;
              CHECK(bits == size && value < last);
              last = value;
              largest = size > largest ? size : largest;
              ++visits;
            });
  CHECK(visits == 6 && largest == 6 && !any_over);  // (neither a seventh group nor the support of every group)
  // with a hierarchy: the seed only ever holds admissible supports -- group 0 needs group 9
  std::vector<L0Mask128> need(10, l0m_none<L0Mask128>());
  l0m_set(need[0], 9);
  l0_greedy(P.H.data(), P.c.data(), 100, gstart, need, 3, [&](L0Mask128) { return 0.0; },
            [&](int, L0Mask128 mask, double) { CHECK(!l0m_test(mask, 0) || l0m_test(mask, 9)); });
  // narrow masks, a problem that fits: every size and the support of every group
  const Problem Q = make(120, 12, {});
  std::vector<int> gs;
  for (int g = 0; g <= 6; ++g) gs.push_back(2 * g);
  const std::vector<unsigned long long> none6(6, 0ull);
  int sizes = 0;
  unsigned long long final_mask = 0;
  l0_greedy(Q.H.data(), Q.c.data(), 12, gs, none6, 6, [&](unsigned long long) { return 0.0; },
            [&](int, unsigned long long mask, double) {
              ++sizes;
              final_mask = mask;
            });
  CHECK(sizes == 7 && final_mask == 63ull);
}

static void test_capacity_rule() {
  // no refusal: proven whatever the objective; a refusal at c_min = 8 groups (cut = 9): proven iff objective <= q_all + 9 alpha
  CHECK(l0_capacity_proven(-1.0, -5.0, 0.1, 0));
  CHECK(l0_capacity_bound(-5.0, 0.1, 9) == -5.0 + 0.1 * 9.0);
  CHECK(!l0_capacity_proven(-4.0, -5.0, 0.1, 9) && l0_capacity_proven(-4.1, -5.0, 0.1, 9) && l0_capacity_proven(-4.5, -5.0, 0.1, 9));
  CHECK(!l0_capacity_proven(-4.9, -5.0, 0.0, 1));  // alpha = 0: only an incumbent that has reached q_all is proven
  CHECK(l0_capacity_proven(-5.0, -5.0, 0.0, 1));
}

int main() {
  test_masks();
  test_q_all_on_100_columns();
  test_support_beyond_column_64();
  test_greedy_stops_at_capacity();
  test_capacity_rule();
  if (failures) {
    fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  printf("l0_wide_host_test: ok\n");
  return 0;
}
