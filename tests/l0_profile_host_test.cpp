// CPU test of the profile mode of csrc/l0_host.hpp -- the host side of slm_solve_l0_profile: the two questions the table of
// per-size bests answers (l0_profile_best_subset, l0_profile_regularized), the envelope E the pruning rule compares against
// (l0_profile_term / l0_profile_join / l0_profile_envelope, the functions the kernel folds across its lanes) and the rule
// itself (l0_profile_cut) -- meant to run under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_l0_profile_cpu.py
// builds and runs it both plainly and sanitized).  The rule's soundness is checked by a host depth-first enumeration of a
// 10-column problem that applies it, against the same enumeration without it, at several alpha >= alpha_min.
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

static const double INF = HUGE_VAL;

static void test_table_questions() {
  // strictly decreasing: the bound binds at every K'
  const double dec[5] = {0.0, -3.0, -5.0, -6.0, -6.5};
  for (int K = 0; K <= 4; ++K) CHECK(l0_profile_best_subset(dec, K) == K);
  // values[k] + alpha k: gains are 3, 2, 1, 0.5
  CHECK(l0_profile_regularized(dec, 4, 0.0) == 4);
  CHECK(l0_profile_regularized(dec, 4, 0.75) == 3);
  CHECK(l0_profile_regularized(dec, 4, 1.5) == 2);
  CHECK(l0_profile_regularized(dec, 4, 2.5) == 1);
  CHECK(l0_profile_regularized(dec, 4, 3.5) == 0);
  CHECK(l0_profile_regularized(dec, 2, 0.0) == 2);  // K cuts the table
  // ties go to the smaller k: sizes 2 and 3 tie in value; at alpha = 1 sizes 1 and 2 tie in value + alpha k (both exact)
  const double tie[5] = {0.0, -4.0, -5.0, -5.0, -4.0};
  CHECK(l0_profile_best_subset(tie, 4) == 2 && l0_profile_best_subset(tie, 3) == 2 && l0_profile_best_subset(tie, 1) == 1);
  CHECK(l0_profile_regularized(tie, 4, 0.0) == 2);
  CHECK(l0_profile_regularized(tie, 4, 1.0) == 1);
  CHECK(l0_profile_regularized(tie, 4, 4.0) == 0);  // size 1 ties with the empty support
  // +inf entries are never chosen, wherever they stand; a table of nothing but +inf answers the empty support
  const double holes[6] = {0.0, INF, -6.0, INF, -7.0, INF};
  CHECK(l0_profile_best_subset(holes, 1) == 0 && l0_profile_best_subset(holes, 3) == 2 && l0_profile_best_subset(holes, 5) == 4);
  CHECK(l0_profile_regularized(holes, 5, 0.25) == 4 && l0_profile_regularized(holes, 5, 1.0) == 2 && l0_profile_regularized(holes, 5, 100.0) == 0);
  const double none[4] = {0.0, INF, INF, INF};
  CHECK(l0_profile_best_subset(none, 3) == 0 && l0_profile_regularized(none, 3, 0.0) == 0 && l0_profile_regularized(none, 3, 1.0) == 0);
  // nothing lowers the value: the empty support
  const double up[3] = {0.0, 0.0, 0.0};
  CHECK(l0_profile_best_subset(up, 2) == 0 && l0_profile_regularized(up, 2, 0.0) == 0);
}

static void test_envelope() {
  // against a direct minimum, for every prefix length, with +inf entries in the table
  const double q[8] = {-1.0, INF, -2.5, -2.4, INF, -9.0, -9.5, 3.0};
  for (double am : {0.0, 0.3, 1.0, 2.0, 50.0}) {
    for (int c = 0; c <= 8; ++c) {
      double want = 0.0;
      for (int k = 1; k <= c; ++k) want = fmin(want, q[k - 1] + am * k);
      CHECK(l0_profile_envelope(q, c, am) == want);
      // the fold the kernel runs: an inclusive scan of join over term, then join with 0
      double v = INF;
      for (int k = 1; k <= c; ++k) v = l0_profile_join(v, l0_profile_term(q[k - 1], k, am));
      CHECK(l0_profile_join(0.0, v) == want);
    }
  }
  CHECK(l0_profile_envelope(q, 0, 1.0) == 0.0);
  CHECK(l0_profile_join(1.0, NAN) == 1.0);  // a NaN never enters
  // the cut: q_all + alpha_min (cnt + 1) >= E(cnt); equality cuts
  CHECK(l0_profile_cut(-5.0, 1.0, 2, -2.0) && !l0_profile_cut(-5.0, 1.0, 2, -1.0) && l0_profile_cut(-5.0, 1.0, 2, -3.0));
  CHECK(l0_profile_cut(-0.5, 1.0, 0, 0.0));  // alpha_min above what all columns gain: cut at the root
  CHECK(!l0_profile_cut(-5.0, 0.0, 3, -4.9) && l0_profile_cut(-5.0, 0.0, 3, -5.0));
}

// ---- the pruning rule on a 10-column problem --------------------------------------------------------------------------------
constexpr int P = 10;

static void problem(double* H /* [P*P] */, double* c /* [P] */) {
  double A[14][P], y[14];
  unsigned v = 977u;
  auto next = [&]() {
    v = v * 1103515245u + 12345u;
    return (double)((v >> 16) & 0x3ff) / 512.0 - 1.0;
  };
  for (int i = 0; i < 14; ++i)
    for (int j = 0; j < P; ++j) A[i][j] = next();
  for (int i = 0; i < 14; ++i) y[i] = 2.0 * A[i][1] - 1.5 * A[i][4] + 0.7 * A[i][8] + 0.3 * next();
  for (int i = 0; i < P; ++i) {
    for (int j = 0; j < P; ++j) {
      double t = 0.0;
      for (int k = 0; k < 14; ++k) t += A[k][i] * A[k][j];
      H[i * P + j] = t / 14.0;
    }
    double t = 0.0;
    for (int k = 0; k < 14; ++k) t += A[k][i] * y[k];
    c[i] = t / 14.0;
  }
}

struct Table {
  double q[P + 1];
  unsigned long long mask[P + 1];
  long nodes = 0;
};

// Depth-first include / exclude over the columns in order, as the kernel walks them; prune: apply the rule with the table
// filled so far as the incumbents.
static void dfs(L0Factor& f, int depth, int cnt, unsigned long long incl, int K, double q_all, double alpha_min, bool prune, Table& t) {
  if (depth >= P || cnt >= K) return;
  if (prune && l0_profile_cut(q_all, alpha_min, cnt, l0_profile_envelope(t.q + 1, cnt, alpha_min))) return;
  const int m0 = f.m;
  ++t.nodes;
  if (f.push(depth)) {
    const double val = -0.5 * f.ss;
    const unsigned long long mk = incl | (1ull << depth);
    if (val < t.q[cnt + 1] || (val == t.q[cnt + 1] && mk < t.mask[cnt + 1])) {
      t.q[cnt + 1] = val;
      t.mask[cnt + 1] = mk;
    }
    dfs(f, depth + 1, cnt + 1, mk, K, q_all, alpha_min, prune, t);
  }
  f.pop_to(m0);
  dfs(f, depth + 1, cnt, incl, K, q_all, alpha_min, prune, t);
}

static Table enumerate(const double* H, const double* c, int K, double alpha_min, bool prune) {
  Table t;
  for (int k = 0; k <= P; ++k) {
    t.q[k] = k == 0 ? 0.0 : INF;
    t.mask[k] = k == 0 ? 0ull : ~0ull;
  }
  L0Factor all(H, c, P);
  for (int j = 0; j < P; ++j) (void)all.push(j);
  L0Factor f(H, c, P);
  dfs(f, 0, 0, 0ull, K, -0.5 * all.ss, alpha_min, prune, t);
  return t;
}

static void test_pruning_rule_is_sound() {
  double H[P * P], c[P];
  problem(H, c);
  for (int K : {P, 4}) {
    const Table full = enumerate(H, c, K, 0.0, false);
    long expect = 0;  // every support of at most K columns is one include attempt
    for (int k = 1; k <= K; ++k) {
      long b = 1;
      for (int i = 0; i < k; ++i) b = b * (P - i) / (i + 1);
      expect += b;
    }
    CHECK(full.nodes == expect);
    for (int k = 1; k <= K; ++k) CHECK(std::isfinite(full.q[k]) && __builtin_popcountll(full.mask[k]) == k);
    for (int k = 2; k <= K; ++k) CHECK(full.q[k] < full.q[k - 1]);  // (independent columns: a larger best support is better)
    // alpha_min = 0 prunes nothing before the one support that reaches q_all: the same table
    const Table zero = enumerate(H, c, K, 0.0, true);
    for (int k = 0; k <= K; ++k) CHECK(zero.q[k] == full.q[k] && zero.mask[k] == full.mask[k]);
    // alpha_min > 0: fewer nodes, and at every alpha >= alpha_min the same optimum, value and support
    const double scale = -full.q[K];
    for (double rel : {1e-3, 1e-2, 0.05, 0.2, 0.6}) {
      const double am = rel * scale;
      const Table cutt = enumerate(H, c, K, am, true);
      CHECK(cutt.nodes <= full.nodes);
      if (rel >= 0.05) CHECK(cutt.nodes < full.nodes);
      for (int k = 1; k <= K; ++k) CHECK(cutt.q[k] >= full.q[k]);  // entries are values of real supports
      for (double up : {1.0, 1.0 + 1e-9, 1.7, 4.0, 30.0, 1e4}) {
        const double alpha = am * up;
        const int a = l0_profile_regularized(full.q, K, alpha), b = l0_profile_regularized(cutt.q, K, alpha);
        CHECK(a == b && full.q[a] == cutt.q[b] && full.mask[a] == cutt.mask[b]);
      }
    }
    // alpha_min above what all columns gain: cut at the root, nothing visited, the table is empty but for size 0
    L0Factor all(H, c, P);
    for (int j = 0; j < P; ++j) (void)all.push(j);
    const double above = 1.01 * 0.5 * all.ss;  // (-q_all)
    const Table root = enumerate(H, c, K, above, true);
    CHECK(root.nodes == 0 && l0_profile_regularized(root.q, K, above) == 0);
    for (int k = 1; k <= K; ++k) CHECK(root.q[k] == INF);
  }
}

int main() {
  test_table_questions();
  test_envelope();
  test_pruning_rule_is_sound();
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("l0_profile_host_test: ok\n");
  return 0;
}
