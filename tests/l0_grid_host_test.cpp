// CPU test of what the l0 profile grid adds to csrc/l0_host.hpp (slm_solve_l0_profile_grid in engine_l0.hip calls THESE
// functions): the problem index over (row set, eta), the argument checks, and the layout of up to L0_GRID_MAX problems in one
// block -- copies disjoint, the control words (the per-problem eta word among them) inside each copy, the grid's size on a
// large and on a small device.  Meant to run under AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_l0_grid_cv_cpu.py
// builds and runs it both plainly and sanitized).
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

// the kernel's constants as l0_kernels.hpp has them: eleven control words (q_all in word 9, the l1 weight in word 10), then 64 incumbents
static const int QALL_WORD = 9, ETA_WORD = 10, CTL_WORDS = 11, PROFILE_CTL = CTL_WORDS + 64, PREFIX = 16, BLOCK_WAVES = 4, SLOTS = 64;

// ---- the layout at many problems --------------------------------------------------------------------------------------------
static void check_layout(int count, int n_eta, int p, int ng, int cus) {
  const int problems = count * n_eta;
  const L0BatchLayout B = l0_grid_layout(count, n_eta, p, ng, cus, SLOTS, PROFILE_CTL, PREFIX, BLOCK_WAVES);
  const L0Layout& y = B.one;
  const int d = ng < PREFIX ? ng : PREFIX;
  long long want = ((1ll << d) + BLOCK_WAVES - 1) / BLOCK_WAVES, cap = 2ll * cus / problems;
  if (cap < 1) cap = 1;
  if (want > cap) want = cap;
  CHECK(B.count == problems && y.d == d && y.blocks == (int)want && y.waves == y.blocks * BLOCK_WAVES && B.grid() == problems * y.blocks);
  CHECK(B.grid() <= 2 * cus || y.blocks == 1);  // resident at once, or one workgroup per problem running in waves
  CHECK(B.stride == y.words && B.words == (size_t)problems * B.stride);
  // the control words, the eta word among them, lie inside the copy and before every other section
  CHECK((size_t)ETA_WORD < (size_t)CTL_WORDS && (size_t)QALL_WORD < (size_t)CTL_WORDS && (size_t)PROFILE_CTL == y.off_bv && y.off_bv < B.stride);
  // sections in order, back to back, the last one ending at the stride
  const size_t at[7] = {0, y.off_bv, y.off_bm, y.off_H, y.off_c, y.off_need, y.off_gs};
  const size_t size[7] = {(size_t)PROFILE_CTL, (size_t)y.waves * SLOTS, (size_t)y.waves * SLOTS, (size_t)p * p, (size_t)p, (size_t)ng, (size_t)ng + 1};
  size_t end = 0;
  for (int i = 0; i < 7; ++i) {
    CHECK(at[i] == end);
    end += size[i];
  }
  CHECK(end == B.stride);
  // the copies do not overlap and leave no gap: every word of the block has exactly one owner
  std::vector<unsigned char> owned(B.words, 0);
  for (int b = 0; b < problems; ++b) {
    CHECK(B.at(b) == (size_t)b * B.stride && B.at(b) + B.stride <= B.words);
    CHECK(B.at(b) + ETA_WORD < B.at(b) + B.stride);
    for (size_t e = 0; e < B.stride && B.at(b) + e < B.words; ++e) {
      CHECK(owned[B.at(b) + e] == 0);
      owned[B.at(b) + e] = 1;
    }
  }
  for (size_t wd = 0; wd < B.words; ++wd) CHECK(owned[wd] == 1);
  // the host image of such a block takes a write of every problem's two words without leaving it (ASan watches)
  std::vector<unsigned long long> h(B.words, 0ull);
  for (int b = 0; b < problems; ++b) {
    const double q = -1.0 - b, eta = 0.5 * b;
    memcpy(h.data() + B.at(b) + QALL_WORD, &q, sizeof(double));
    memcpy(h.data() + B.at(b) + ETA_WORD, &eta, sizeof(double));
  }
  for (int b = 0; b < problems; ++b) {
    double q, eta;
    memcpy(&q, h.data() + B.at(b) + QALL_WORD, sizeof(double));
    memcpy(&eta, h.data() + B.at(b) + ETA_WORD, sizeof(double));
    CHECK(q == -1.0 - b && eta == 0.5 * b);
  }
}

static void check_grid_sizes() {
  // 256 CUs: never more than 2 CUs workgroups, whatever the number of problems up to the cap
  for (int problems : {1, 18, 96, 128}) {
    const L0BatchLayout B = l0_batch_layout(problems, 20, 20, 256, 1, SLOTS, PROFILE_CTL, PREFIX, BLOCK_WAVES);
    CHECK(B.grid() <= 2 * 256);
    CHECK(B.one.blocks == 2 * 256 / problems);  // (2^16 tickets want more than any share: the share decides)
  }
  // 64 CUs: the full grid still fits, one workgroup per problem
  {
    const L0BatchLayout B = l0_batch_layout(L0_GRID_MAX, 20, 20, 64, 1, SLOTS, PROFILE_CTL, PREFIX, BLOCK_WAVES);
    CHECK(B.one.blocks == 1 && B.grid() == L0_GRID_MAX && B.grid() <= 2 * 64);
  }
  // 32 CUs: one workgroup per problem; 96 and 128 problems exceed 2 CUs = 64 and run in waves, 18 keep three each
  for (int problems : {96, 128}) {
    const L0BatchLayout B = l0_batch_layout(problems, 20, 20, 32, 1, SLOTS, PROFILE_CTL, PREFIX, BLOCK_WAVES);
    CHECK(B.one.blocks == 1 && B.grid() == problems && B.grid() > 2 * 32);
  }
  CHECK(l0_batch_layout(18, 20, 20, 32, 1, SLOTS, PROFILE_CTL, PREFIX, BLOCK_WAVES).one.blocks == 3);
  CHECK(l0_batch_layout(1, 20, 20, 32, 1, SLOTS, PROFILE_CTL, PREFIX, BLOCK_WAVES).one.blocks == 64);
}

// ---- the problem index --------------------------------------------------------------------------------------------------------
static void check_index() {
  for (int count : {1, 6, 16})
    for (int n_eta : {1, 3, 8}) {
      std::vector<int> seen((size_t)count * n_eta, 0);
      for (int r = 0; r < count; ++r)
        for (int e = 0; e < n_eta; ++e) {
          const int b = l0_grid_index(r, e, n_eta);
          CHECK(b >= 0 && b < count * n_eta);
          CHECK(l0_grid_row_set(b, n_eta) == r && l0_grid_eta(b, n_eta) == e);
          if (b >= 0 && b < count * n_eta) ++seen[(size_t)b];
          if (e > 0) CHECK(b == l0_grid_index(r, e - 1, n_eta) + 1);  // a row set's problems lie side by side, etas innermost
        }
      for (int v : seen) CHECK(v == 1);
    }
  static_assert(l0_grid_index(2, 1, 3) == 7 && l0_grid_row_set(7, 3) == 2 && l0_grid_eta(7, 3) == 1, "row sets outermost");
}

// ---- the argument checks --------------------------------------------------------------------------------------------------------
static void check_refusals() {
  const double ok[3] = {0.0, 0.5, 2.0};
  int which = -1;
  CHECK(l0_grid_check(6, 3, ok, 0, false) == L0_GRID_OK);
  CHECK(l0_grid_check(6, 3, ok, 0, true) == L0_GRID_OK);   // a ridge grid takes T
  CHECK(l0_grid_check(6, 3, ok, 1, false) == L0_GRID_OK);
  CHECK(l0_grid_check(1, 1, ok, 1, false) == L0_GRID_OK);
  CHECK(l0_grid_check(0, 3, ok, 0, false) == L0_GRID_COUNT);
  CHECK(l0_grid_check(17, 1, ok, 0, false) == L0_GRID_COUNT);
  CHECK(l0_grid_check(-1, 3, ok, 0, false) == L0_GRID_COUNT);
  CHECK(l0_grid_check(6, 0, ok, 0, false) == L0_GRID_N_ETA);
  CHECK(l0_grid_check(6, -4, ok, 0, false) == L0_GRID_N_ETA);
  CHECK(l0_grid_check(6, 3, nullptr, 0, false) == L0_GRID_NULL);
  CHECK(l0_grid_check(6, 3, ok, 2, false) == L0_GRID_KIND);
  CHECK(l0_grid_check(6, 3, ok, -1, false) == L0_GRID_KIND);
  CHECK(l0_grid_check(6, 3, ok, 1, true) == L0_GRID_T_WITH_L1);
  const double neg[3] = {0.1, -0.5, 2.0}, nan_[3] = {0.1, 0.5, NAN}, inf_[3] = {INFINITY, 0.5, 1.0};
  CHECK(l0_grid_check(6, 3, neg, 0, false, &which) == L0_GRID_ETA && which == 1);
  CHECK(l0_grid_check(6, 3, nan_, 1, false, &which) == L0_GRID_ETA && which == 2);
  CHECK(l0_grid_check(6, 3, inf_, 0, false, &which) == L0_GRID_ETA && which == 0);
  // the cap: 16 x 8 = 128 is in, 3 x 43 = 129 and 16 x 9 = 144 are out -- decided before etas is read (a one-entry array, ASan watches)
  std::vector<double> eight(8, 0.25);
  const double one[1] = {0.25};
  CHECK(L0_GRID_MAX == 128 && L0_GRID_ROW_SETS == 16);
  CHECK(l0_grid_check(16, 8, eight.data(), 1, false) == L0_GRID_OK);
  CHECK(l0_grid_check(3, 43, one, 1, false) == L0_GRID_PROBLEMS);
  CHECK(l0_grid_check(16, 9, one, 0, false) == L0_GRID_PROBLEMS);
  CHECK(l0_grid_check(2, 0x7fffffff, one, 0, false) == L0_GRID_PROBLEMS);  // (no overflow: the product is taken in 64 bits)
}

int main() {
  for (int problems : {1, 18, 96, 128})
    for (int cus : {32, 256})
      for (int p : {1, 12, 20, 64}) {
        const int n_eta = problems == 1 ? 1 : (problems == 18 ? 3 : (problems == 96 ? 6 : 8)), count = problems / n_eta;
        check_layout(count, n_eta, p, p, cus);
        if (p >= 4) check_layout(count, n_eta, p, p / 2, cus);  // grouped: fewer groups than columns
      }
  check_grid_sizes();
  check_index();
  check_refusals();
  if (failures) {
    fprintf(stderr, "l0_grid_host_test: %d failure(s)\n", failures);
    return 1;
  }
  printf("l0_grid_host_test: ok\n");
  return 0;
}
