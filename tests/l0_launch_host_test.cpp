// CPU test of what every exact-l0 entry's launch shares (the end of csrc/l0_host.hpp; engine_l0.hip calls THESE functions): the
// layout of the device block for every mode, the winner among the waves' results under the tie rule, and the way back from
// search order to the caller's groups and columns.  Meant to run under AddressSanitizer and UndefinedBehaviorSanitizer
// (tests/test_l0_launch_cpu.py builds and runs it both plainly and sanitized).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <numeric>
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

// the kernel's constants as l0_kernels.hpp has them (the layout takes them as arguments: any values must tile)
static const int CTL = 10, PROFILE_CTL = 10 + 64, PREFIX = 16, BLOCK_WAVES = 4;

// ---- the layout ---------------------------------------------------------------------------------------------------------------
struct Mode {
  const char* name;
  int mask_words, slots, ctl;
  int m;      // >= 0: the constrained sections A, lo, hi, blo, bhi follow
  bool excl;  // the exclusion bound's P and P c follow
};
static void check_layout(const Mode& md, int p, int cus) {
  const int ng = p;
  L0Layout y = l0_layout(p, ng, cus, md.mask_words, md.slots, md.ctl, PREFIX, BLOCK_WAVES);
  // the grid: 2^d tickets, one per wave while they last, at least one workgroup, at most two per CU
  const int d = ng < PREFIX ? ng : PREFIX;
  long long blocks = ((1ll << d) + BLOCK_WAVES - 1) / BLOCK_WAVES;
  if (blocks > 2ll * cus) blocks = 2ll * cus;
  if (blocks < 1) blocks = 1;
  CHECK(y.d == d && y.blocks == (int)blocks && y.waves == (int)blocks * BLOCK_WAVES);
  CHECK(y.slots == md.slots && y.mask_words == md.mask_words);
  // the sections in the documented order, each where the one before it ends
  std::vector<size_t> at = {0, y.off_bv, y.off_bm, y.off_H, y.off_c, y.off_need, y.off_gs};
  std::vector<size_t> size = {(size_t)md.ctl, (size_t)y.waves * md.slots, (size_t)md.mask_words * y.waves * md.slots, (size_t)p * p, (size_t)p,
                              (size_t)md.mask_words * ng, (size_t)ng + 1};
  if (md.m >= 0)
    for (size_t n : {(size_t)md.m * p, (size_t)md.m, (size_t)md.m, (size_t)p, (size_t)p}) {
      at.push_back(y.append(n));
      size.push_back(n);
    }
  if (md.excl)
    for (size_t n : {(size_t)p * p, (size_t)p}) {
      at.push_back(y.append(n));
      size.push_back(n);
    }
  size_t end = 0;
  for (size_t i = 0; i < at.size(); ++i) {
    if (at[i] != end) fprintf(stderr, "%s p = %d cus = %d: section %zu at %zu, expected %zu\n", md.name, p, cus, i, at[i], end);
    CHECK(at[i] == end);  // disjoint, in order, no gap
    end += size[i];
  }
  CHECK(end == y.words);  // ... and they tile [0, words)
}

// l0_fill_image writes H, c, need and the group starts where the layout says and nothing else
static void check_image() {
  const int p = 5, ng = 3;
  L0Layout y = l0_layout(p, ng, 2, 2, 1, CTL, PREFIX, BLOCK_WAVES);
  const size_t tail = y.append(4);
  std::vector<double> H((size_t)p * p), c((size_t)p);
  for (size_t i = 0; i < H.size(); ++i) H[i] = 1.0 + (double)i;
  for (size_t i = 0; i < c.size(); ++i) c[i] = -1.0 - (double)i;
  std::vector<L0Mask128> needo = {{0, 0}, {1, 0}, {3, 1ull << 63}};
  std::vector<int> gstart = {0, 2, 3, 5};
  std::vector<u64> h(y.words, 0xabull);
  l0_fill_image(y, H.data(), c.data(), p, needo, gstart, h.data());
  CHECK(memcmp(&h[y.off_H], H.data(), sizeof(double) * H.size()) == 0 && memcmp(&h[y.off_c], c.data(), sizeof(double) * c.size()) == 0);
  CHECK(h[y.off_need + 2] == 1 && h[y.off_need + 3] == 0 && h[y.off_need + 4] == 3 && h[y.off_need + 5] == 1ull << 63);
  for (int g = 0; g <= ng; ++g) CHECK(h[y.off_gs + (size_t)g] == (u64)gstart[(size_t)g]);
  for (size_t i = 0; i < y.off_H; ++i) CHECK(h[i] == 0xab);
  for (size_t i = tail; i < y.words; ++i) CHECK(h[i] == 0xab);
}

// ---- the winner ---------------------------------------------------------------------------------------------------------------
static u64 bits(double v) {
  u64 b;
  memcpy(&b, &v, 8);
  return b;
}
// a block as read back: `waves` x `stride` values at off_bv, as many masks at off_bm
template <class Mask>
struct Field {
  int waves, stride;
  size_t off_bv, off_bm;
  std::vector<u64> h;
  Field(int waves_, int stride_) : waves(waves_), stride(stride_), off_bv(3), off_bm(3 + (size_t)waves_ * stride_) {
    const size_t n = (size_t)waves * stride, mw = sizeof(Mask) / 8;
    h.assign(off_bm + mw * n, 0);
    const Mask ones = l0m_ones<Mask>();  // what a wave that found nothing leaves
    for (size_t i = 0; i < n; ++i) {
      h[off_bv + i] = bits(HUGE_VAL);
      memcpy(&h[off_bm + mw * i], &ones, sizeof(Mask));
    }
  }
  void set(int wave, int slot, double v, Mask mk) {
    const size_t i = (size_t)wave * stride + slot;
    h[off_bv + i] = bits(v);
    memcpy(&h[off_bm + (sizeof(Mask) / 8) * i], &mk, sizeof(Mask));
  }
  void winner(int slot, double& v, Mask& mk) const { l0_winner(h.data(), off_bv, off_bm, waves, stride, slot, v, mk); }
};

static void check_winner() {
  {  // one word: the lower value; on a bitwise tie the lower support, whoever holds it
    Field<u64> f(8, 1);
    f.set(2, 0, -1.5, 0x30);
    f.set(5, 0, -1.5, 0x28);
    f.set(6, 0, -1.0, 0x01);
    double v = 0.0;
    u64 mk = 0;
    f.winner(0, v, mk);
    CHECK(v == -1.5 && mk == 0x28);
    v = -1.5, mk = 0x29;  // the seed wins the tie against a higher mask ...
    Field<u64> g(8, 1);
    g.set(3, 0, -1.5, 0x30);
    g.winner(0, v, mk);
    CHECK(v == -1.5 && mk == 0x29);
    v = -1.5, mk = 0x31;  // ... and loses it against a lower one
    g.winner(0, v, mk);
    CHECK(v == -1.5 && mk == 0x30);
    v = -2.0, mk = 0x7;  // a seed below every wave stays
    g.winner(0, v, mk);
    CHECK(v == -2.0 && mk == 0x7);
  }
  {  // nothing found anywhere: the seed stays, a finite one and the +inf, all-ones seed of an infeasible empty support alike
    Field<u64> f(4, 1);
    double v = 0.0;
    u64 mk = 0;
    f.winner(0, v, mk);
    CHECK(v == 0.0 && mk == 0);
    v = HUGE_VAL, mk = ~0ull;
    f.winner(0, v, mk);
    CHECK(v == HUGE_VAL && mk == ~0ull);
    f.set(1, 0, HUGE_VAL, 0x5);  // +inf is "nothing held", never a tie: the mask that comes with it is not taken
    f.winner(0, v, mk);
    CHECK(v == HUGE_VAL && mk == ~0ull);
    CHECK(!l0_better(HUGE_VAL, (u64)1, HUGE_VAL, ~0ull) && l0_better(1.0, ~0ull, HUGE_VAL, (u64)0));
    CHECK(!l0_better(NAN, (u64)0, 1.0, (u64)1) && !l0_better(1.0, (u64)0, NAN, (u64)1));
  }
  {  // two words: the order of the 128-bit integer, the high word first
    Field<L0Mask128> f(4, 1);
    f.set(0, 0, -3.0, L0Mask128{0x1, 0x2});
    f.set(1, 0, -3.0, L0Mask128{~0ull, 0x1});  // a larger low word, a smaller high one: the lower support
    f.set(3, 0, -3.0, L0Mask128{0x0, 0x2});
    double v = 0.0;
    L0Mask128 mk{0, 0};
    f.winner(0, v, mk);
    CHECK(v == -3.0 && mk.lo == ~0ull && mk.hi == 0x1);
    v = -3.0, mk = L0Mask128{0x5, 0x0};  // a seed with an empty high word is lower still
    f.winner(0, v, mk);
    CHECK(mk.lo == 0x5 && mk.hi == 0x0);
  }
  {  // profile mode: size k reads entry k - 1 of each wave's 64, and no other
    Field<u64> f(3, 64);
    for (int wv = 0; wv < 3; ++wv)
      for (int k = 1; k <= 64; ++k) f.set(wv, k - 1, -(double)k - 0.25 * ((wv + k) % 3), ((u64)(wv + 1) << 8) | (u64)k);
    for (int k = 1; k <= 64; ++k) {
      double v = HUGE_VAL;
      u64 mk = ~0ull;
      f.winner(k - 1, v, mk);
      int best = 0;
      for (int wv = 1; wv < 3; ++wv)
        if ((wv + k) % 3 > (best + k) % 3) best = wv;
      CHECK(v == -(double)k - 0.25 * ((best + k) % 3) && mk == (((u64)(best + 1) << 8) | (u64)k));
    }
    Field<L0Mask128> w(2, 64);
    w.set(1, 63, -7.0, L0Mask128{0x9, 0x8});
    double v = HUGE_VAL;
    L0Mask128 mk = l0m_ones<L0Mask128>();
    w.winner(63, v, mk);
    CHECK(v == -7.0 && mk.lo == 0x9 && mk.hi == 0x8);
    v = HUGE_VAL, mk = l0m_ones<L0Mask128>();
    w.winner(62, v, mk);
    CHECK(v == HUGE_VAL && mk.lo == ~0ull && mk.hi == ~0ull);
  }
}

// ---- back to the caller's order -----------------------------------------------------------------------------------------------
template <class Mask>
static void check_mapping(int ng) {
  // a search order that is no identity: group (7 k + 3) mod ng at position k (7 and ng coprime); two columns per group,
  // the caller's columns of group g being g and ng + g
  std::vector<int> gorder((size_t)ng), gpos((size_t)ng), cols;
  for (int k = 0; k < ng; ++k) {
    gorder[(size_t)k] = (7 * k + 3) % ng;
    gpos[(size_t)gorder[(size_t)k]] = k;
    cols.push_back(gorder[(size_t)k]);
    cols.push_back(ng + gorder[(size_t)k]);
  }
  Mask search = l0m_none<Mask>();
  int held = 0;
  for (int k = 0; k < ng; k += 3) {
    l0m_set(search, k);
    ++held;
  }
  int count = -1;
  const Mask caller = l0_caller_mask(search, gorder, &count);
  CHECK(count == held);
  for (int g = 0; g < ng; ++g) CHECK(l0m_test(caller, g) == l0m_test(search, gpos[(size_t)g]));
  // ... and back through the inverse order: a round trip
  const Mask again = l0_caller_mask(caller, gpos);
  CHECK(!l0m_less(again, search) && !l0m_less(search, again));
  CHECK(!l0m_any_outside(caller, l0m_below<Mask>(ng)));
  // coefficients: position i goes to column cols[i], every column once
  const int p = 2 * ng;
  std::vector<double> beta_s((size_t)p), beta((size_t)p, NAN);
  for (int i = 0; i < p; ++i) beta_s[(size_t)i] = 1.0 + (double)i;
  l0_scatter(beta_s.data(), cols, beta.data());
  for (int i = 0; i < p; ++i) CHECK(beta[(size_t)cols[(size_t)i]] == beta_s[(size_t)i]);
  for (int g = 0; g < ng; ++g) CHECK(beta[(size_t)g] == 1.0 + 2.0 * gpos[(size_t)g] && beta[(size_t)(ng + g)] == 2.0 + 2.0 * gpos[(size_t)g]);
}

// the loss from the Gram against the residual it stands for
static void check_loss() {
  const int n = 9, p = 4;
  std::vector<double> X((size_t)n * p), yv((size_t)n), G((size_t)p * p, 0.0), c((size_t)p, 0.0), beta = {0.5, 0.0, -1.25, 2.0};
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < p; ++j) X[(size_t)i * p + j] = (double)((i * 7 + j * 3) % 5) - 2.0;
    yv[(size_t)i] = (double)(i % 4) - 1.5;
  }
  double yy = 0.0, direct = 0.0;
  for (int i = 0; i < n; ++i) {
    yy += yv[(size_t)i] * yv[(size_t)i] / n;
    double r = -yv[(size_t)i];
    for (int j = 0; j < p; ++j) {
      r += X[(size_t)i * p + j] * beta[(size_t)j];
      c[(size_t)j] += X[(size_t)i * p + j] * yv[(size_t)i] / n;
      for (int k = 0; k < p; ++k) G[(size_t)j * p + k] += X[(size_t)i * p + j] * X[(size_t)i * p + k] / n;
    }
    direct += r * r / (2.0 * n);
  }
  CHECK(fabs(l0_gram_loss(G.data(), c.data(), p, yy, beta.data()) - direct) <= 1e-13 * (1.0 + direct));
  std::vector<double> zero((size_t)p, 0.0);
  CHECK(l0_gram_loss(G.data(), c.data(), p, yy, zero.data()) == 0.5 * yy);
}

int main() {
  const Mode modes[] = {{"narrow", 1, 1, CTL, -1, false},           {"wide", 2, 1, CTL, -1, false},
                        {"profile", 1, 64, PROFILE_CTL, -1, false}, {"profile wide", 2, 64, PROFILE_CTL, -1, false},
                        {"constrained, m = 0", 1, 1, CTL, 0, false}, {"constrained, m = 64", 1, 1, CTL, 64, false},
                        {"exclusion bound", 1, 1, CTL, -1, true},    {"exclusion bound wide", 2, 1, CTL, -1, true}};
  for (const Mode& md : modes)
    for (int p : {1, 64, 128})
      for (int cus : {1, 256}) check_layout(md, p, cus);
  // the grid at the edges of its clamp: one ticket, fewer tickets than a workgroup's waves, and the ticket prefix
  CHECK(l0_layout(0, 0, 256, 1, 1, CTL, PREFIX, BLOCK_WAVES).blocks == 1 && l0_layout(1, 1, 256, 1, 1, CTL, PREFIX, BLOCK_WAVES).blocks == 1);
  CHECK(l0_layout(3, 3, 256, 1, 1, CTL, PREFIX, BLOCK_WAVES).blocks == 2 && l0_layout(12, 12, 256, 1, 1, CTL, PREFIX, BLOCK_WAVES).blocks == 512);
  CHECK(l0_layout(20, 20, 256, 1, 1, CTL, PREFIX, BLOCK_WAVES).d == PREFIX && l0_layout(20, 20, 1, 1, 1, CTL, PREFIX, BLOCK_WAVES).waves == 8);
  check_image();
  check_winner();
  check_mapping<u64>(5);
  check_mapping<u64>(64);
  check_mapping<L0Mask128>(65);
  check_mapping<L0Mask128>(128);
  check_loss();
  if (failures) {
    fprintf(stderr, "l0_launch_host_test: %d failure(s)\n", failures);
    return 1;
  }
  printf("l0_launch_host_test: ok\n");
  return 0;
}
