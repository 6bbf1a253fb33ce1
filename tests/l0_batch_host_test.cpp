// CPU test of what the batched l0 profile adds to csrc/l0_host.hpp (slm_solve_l0_profile_batch in engine_l0.hip calls THESE
// functions): the layout of `count` problems in one block -- offsets disjoint, count = 1 identical to l0_layout, the rule for
// the workgroups per problem -- and the elimination of an intercept column from a Gram, against centring in long double.
// Meant to run under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_l0_cv_cpu.py builds and runs it both plainly
// and sanitized).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../sparse-lm_amd/csrc/l0_host.hpp"

using namespace slm;
typedef unsigned long long u64;

static int failures = 0;
#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) {                                                            \
      fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__); \
      ++failures;                                                             \
    }                                                                         \
  } while (0)

// the kernel's constants as l0_kernels.hpp has them
static const int PROFILE_CTL = 10 + 64, PREFIX = 16, BLOCK_WAVES = 4, SLOTS = 64;

// ---- the layout ---------------------------------------------------------------------------------------------------------------
static bool same(const L0Layout& a, const L0Layout& b) {
  return a.d == b.d && a.blocks == b.blocks && a.waves == b.waves && a.slots == b.slots && a.mask_words == b.mask_words && a.off_bv == b.off_bv &&
         a.off_bm == b.off_bm && a.off_H == b.off_H && a.off_c == b.off_c && a.off_need == b.off_need && a.off_gs == b.off_gs && a.words == b.words;
}
static void check_layout(int count, int p, int ng, int cus) {
  const L0BatchLayout B = l0_batch_layout(count, p, ng, cus, 1, SLOTS, PROFILE_CTL, PREFIX, BLOCK_WAVES);
  const L0Layout& y = B.one;
  // blocks_b = clamp(ceil(2^d / waves per workgroup), 1, max(1, floor(2 cus / count)))
  const int d = ng < PREFIX ? ng : PREFIX;
  long long want = ((1ll << d) + BLOCK_WAVES - 1) / BLOCK_WAVES, cap = 2ll * cus / count;
  if (cap < 1) cap = 1;
  if (want > cap) want = cap;
  if (want < 1) want = 1;
  if (y.blocks != (int)want) fprintf(stderr, "count %d p %d ng %d cus %d: %d workgroups per problem, expected %lld\n", count, p, ng, cus, y.blocks, want);
  CHECK(y.d == d && y.blocks == (int)want && y.waves == y.blocks * BLOCK_WAVES && B.grid() == count * y.blocks);
  // the whole grid is resident at once: at most two workgroups per CU -- unless there are more problems than that, one each
  CHECK(B.grid() <= 2 * cus || y.blocks == 1);
  // every copy is a whole single-problem layout; the copies tile the block back to back
  std::vector<size_t> at = {0, y.off_bv, y.off_bm, y.off_H, y.off_c, y.off_need, y.off_gs};
  std::vector<size_t> size = {(size_t)PROFILE_CTL, (size_t)y.waves * SLOTS, (size_t)y.waves * SLOTS, (size_t)p * p, (size_t)p, (size_t)ng, (size_t)ng + 1};
  size_t end = 0;
  for (size_t i = 0; i < at.size(); ++i) {
    CHECK(at[i] == end);
    end += size[i];
  }
  CHECK(end == y.words && B.stride == y.words && B.words == (size_t)count * B.stride && B.count == count);
  std::vector<int> owner(B.words, -1);
  for (int b = 0; b < count; ++b) {
    CHECK(B.at(b) == (size_t)b * B.stride);
    for (size_t i = 0; i < at.size(); ++i)
      for (size_t e = 0; e < size[i]; ++e) {
        const size_t word = B.at(b) + at[i] + e;
        CHECK(word < B.words);
        if (word < B.words) {
          CHECK(owner[word] == -1);  // disjoint: no word belongs to two sections or two problems
          owner[word] = b;
        }
      }
  }
  for (size_t wd = 0; wd < B.words; ++wd) CHECK(owner[wd] >= 0);  // ... and no gap
  if (count == 1) CHECK(same(y, l0_layout(p, ng, cus, 1, SLOTS, PROFILE_CTL, PREFIX, BLOCK_WAVES)));
}

// the single layout of every mode is still what it was: l0_layout is the cap of two workgroups per CU
static void check_single_is_the_capped_one() {
  for (int cus : {1, 8, 256})
    for (int p : {1, 5, 17, 64})
      for (int mw : {1, 2})
        for (int slots : {1, 64}) {
          const L0Layout a = l0_layout(p, p, cus, mw, slots, slots == 64 ? PROFILE_CTL : 10, PREFIX, BLOCK_WAVES);
          const L0Layout b = l0_layout_capped(p, p, 2ll * cus, mw, slots, slots == 64 ? PROFILE_CTL : 10, PREFIX, BLOCK_WAVES);
          CHECK(same(a, b));
          long long blocks = ((1ll << (p < PREFIX ? p : PREFIX)) + BLOCK_WAVES - 1) / BLOCK_WAVES;
          if (blocks > 2ll * cus) blocks = 2ll * cus;
          CHECK(a.blocks == (int)blocks);
        }
}

// ---- the elimination ----------------------------------------------------------------------------------------------------------
static double unit(u64& state) {  // a fixed stream in (-1, 1)
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return (double)((state >> 11) & ((1ull << 52) - 1)) / (double)(1ull << 51) - 1.0;
}

// The Gram of [X | 1] under weights w (sum n), eliminated, against the Gram of the columns centred by their weighted means in
// long double.  The bound is a priori: an entry of the Gram is a sum of n products and the elimination adds a product, a
// quotient and a subtraction, so its error is at most (n + 4) 2^-53 times the magnitude M_ab = sum_i w_i |x_ia| |x_ib| / n of
// what was summed (>= |g_a g_b| / G11 by Cauchy-Schwarz), doubled for the product that is subtracted.  Relative to the CENTRED
// entry that is the cancellation the header documents: it grows with (shift / spread)^2, and `lost` is how much of it shows.
static void check_elimination(int n, int q, double shift, double lost_min, double lost_max) {
  const int p = q + 1;
  const long double unit_err = 2.0L * (n + 4) * 0x1p-53L;
  u64 st = 12345u + (u64)n * 31u + (u64)q;
  std::vector<double> X((size_t)n * p), y((size_t)n), w((size_t)n);
  double wsum = 0.0;
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < q; ++j) X[(size_t)i * p + j] = unit(st) * (1.0 + 0.01 * j) + shift;
    X[(size_t)i * p + q] = 1.0;
    y[(size_t)i] = 3.0 * unit(st) + 0.5 * shift;
    w[(size_t)i] = i % 7 == 3 ? 0.0 : 0.5 + fabs(unit(st));  // (a fold's mask leaves rows out)
    wsum += w[(size_t)i];
  }
  for (int i = 0; i < n; ++i) w[(size_t)i] *= (double)n / wsum;
  std::vector<double> G((size_t)p * p, 0.0), c((size_t)p, 0.0);
  double yy = 0.0;
  for (int i = 0; i < n; ++i) {
    for (int a = 0; a < p; ++a) {
      c[(size_t)a] += w[(size_t)i] * X[(size_t)i * p + a] * y[(size_t)i] / n;
      for (int b = 0; b <= a; ++b) G[(size_t)a * p + b] += w[(size_t)i] * X[(size_t)i * p + a] * X[(size_t)i * p + b] / n;
    }
    yy += w[(size_t)i] * y[(size_t)i] * y[(size_t)i] / n;
  }
  for (int a = 0; a < p; ++a)  // (the engine's Grams are mirrored triangles: symmetric to the bit)
    for (int b = 0; b < a; ++b) G[(size_t)b * p + a] = G[(size_t)a * p + b];
  std::vector<double> Gs((size_t)q * q), cs((size_t)q), xmean((size_t)q);
  double yys = 0.0, ymean = 0.0;
  CHECK(l0_eliminate_last(G.data(), c.data(), p, yy, Gs.data(), cs.data(), &yys, xmean.data(), &ymean));
  // centring in long double
  std::vector<long double> xm((size_t)q, 0.0L);
  long double ym = 0.0L, ws = 0.0L;
  for (int i = 0; i < n; ++i) {
    ws += w[(size_t)i];
    ym += (long double)w[(size_t)i] * y[(size_t)i];
    for (int j = 0; j < q; ++j) xm[(size_t)j] += (long double)w[(size_t)i] * X[(size_t)i * p + j];
  }
  ym /= ws;
  for (int j = 0; j < q; ++j) xm[(size_t)j] /= ws;
  CHECK(fabsl(ymean - ym) <= unit_err * (1.0L + fabsl(ym)));
  long double yyc = 0.0L, yym = 0.0L;
  for (int i = 0; i < n; ++i) {
    yyc += (long double)w[(size_t)i] * (y[(size_t)i] - ym) * (y[(size_t)i] - ym) / n;
    yym += (long double)w[(size_t)i] * y[(size_t)i] * y[(size_t)i] / n;
  }
  CHECK(fabsl(yys - yyc) <= unit_err * yym);
  long double worst = 0.0L, lost = 0.0L;  // of the a-priori bound; of the centred entries' own magnitude
  for (int a = 0; a < q; ++a) {
    CHECK(fabsl(xmean[(size_t)a] - xm[(size_t)a]) <= unit_err * (1.0L + fabsl(xm[(size_t)a])));
    long double ca = 0.0L, mag_c = 0.0L;
    for (int i = 0; i < n; ++i) {
      ca += (long double)w[(size_t)i] * (X[(size_t)i * p + a] - xm[(size_t)a]) * (y[(size_t)i] - ym) / n;
      mag_c += (long double)w[(size_t)i] * fabsl((long double)X[(size_t)i * p + a] * y[(size_t)i]) / n;
    }
    worst = fmaxl(worst, fabsl(cs[(size_t)a] - ca) / (unit_err * mag_c));
    for (int b = 0; b < q; ++b) {
      long double g = 0.0L, mag = 0.0L, centred = 0.0L;
      for (int i = 0; i < n; ++i) {
        const long double t = (long double)w[(size_t)i] * (X[(size_t)i * p + a] - xm[(size_t)a]) * (X[(size_t)i * p + b] - xm[(size_t)b]) / n;
        g += t;
        centred += fabsl(t);
        mag += (long double)w[(size_t)i] * fabsl((long double)X[(size_t)i * p + a] * X[(size_t)i * p + b]) / n;
      }
      worst = fmaxl(worst, fabsl(Gs[(size_t)a * q + b] - g) / (unit_err * mag));
      lost = fmaxl(lost, fabsl(Gs[(size_t)a * q + b] - g) / centred);
      CHECK(Gs[(size_t)a * q + b] == Gs[(size_t)b * q + a]);  // symmetric to the bit
    }
  }
  printf("elimination n = %d, q = %d, shift %g: worst error %.3f of the a-priori bound; %.3e of the centred entries' magnitude\n", n, q, shift,
         (double)worst, (double)lost);
  CHECK(worst <= 1.0L);
  CHECK((double)lost >= lost_min && (double)lost <= lost_max);
}

static void check_elimination_refuses_an_empty_row_set() {
  const double G[4] = {1.0, 0.0, 0.0, 0.0}, c[2] = {1.0, 0.0};
  double Gs[1], cs[1], yys, xmean[1], ymean;
  CHECK(!l0_eliminate_last(G, c, 2, 1.0, Gs, cs, &yys, xmean, &ymean));
}

int main() {
  for (int count : {1, 6, 16})
    for (int cus : {1, 256})
      for (int p : {1, 3, 12, 20, 64}) {
        check_layout(count, p, p, cus);
        if (p >= 4) check_layout(count, p, p / 2, cus);  // grouped: fewer groups than columns
      }
  check_layout(5, 24, 12, 8);
  check_single_is_the_capped_one();
  // means of the order of the spread: the centred Gram keeps all but the last digit or two
  check_elimination(50, 12, 0.0, 0.0, 1e-13);
  check_elimination(40, 63, 1.0, 0.0, 1e-13);
  // the documented cancellation: |mean| = 1e4 spreads loses about (1e4)^2 = 1e8 units of 2^-53 -- half the digits, and it shows
  check_elimination(50, 6, 1e4, 1e-11, 1e-5);
  check_elimination_refuses_an_empty_row_set();
  if (failures) {
    fprintf(stderr, "l0_batch_host_test: %d failure(s)\n", failures);
    return 1;
  }
  printf("l0_batch_host_test: ok\n");
  return 0;
}
