// CPU test of csrc/host_logic.hpp -- the engine's device-free bookkeeping --, of csrc/tail_logic.hpp -- the scalar state
// machine of the tail kernels, the very functions the device runs -- and of csrc/l0_host.hpp -- the host side of the exact
// l0 search: the growing factor, the boxed descent, a support's value and coefficients -- meant to run under AddressSanitizer and
// UndefinedBehaviorSanitizer (tools/sanitize.sh; tests/test_host_logic_cpu.py builds and runs it plainly in the CPU suite).
// Every check is against an independent statement of what the function must do; a randomised pool run models the
// allocator with malloc/free so that a double release or a leak is the sanitizers' to find.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <random>
#include <set>
#include <string>

#include "../sparse-lm_amd/csrc/host_logic.hpp"
#include "../sparse-lm_amd/csrc/tail_logic.hpp"
#include "../sparse-lm_amd/csrc/l0_host.hpp"

using namespace slm_host;
using namespace slm;

static int failures = 0;
#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) {                                                            \
      fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__); \
      ++failures;                                                             \
    }                                                                         \
  } while (0)

static void test_pool() {
  PoolLedger book;
  std::mt19937_64 rng(1);
  const size_t sizes[] = {64u << 20, 200u << 20, 1000u << 20, 4000ull << 20};
  const size_t cap = 6000ull << 20;
  std::vector<std::pair<void*, std::pair<int, size_t>>> mine;  // blocks the "engine" holds
  std::set<void*> released;
  size_t driver_allocs = 0, reused = 0;
  for (int step = 0; step < 20000; ++step) {
    const bool alloc = mine.empty() || (rng() % 100 < 55 && mine.size() < 40);
    if (alloc) {
      const int dev = (int)(rng() % 2);
      const size_t bytes = sizes[rng() % 4];
      void* p = book.take(dev, bytes);
      if (!p) {
        p = malloc(16);  // (stands for hipMalloc of `bytes`)
        ++driver_allocs;
        book.adopt(p, dev, bytes);
      } else {
        ++reused;
      }
      for (auto& m : mine) CHECK(m.first != p);  // never handed out twice
      mine.push_back({p, {dev, bytes}});
    } else {
      const size_t i = rng() % mine.size();
      void* p = mine[i].first;
      mine.erase(mine.begin() + (long)i);
      std::vector<void*> evict;
      const bool kept = book.give_back(p, cap, true, &evict);
      for (void* q : evict) {
        CHECK(q != p);
        free(q);
      }
      if (!kept) free(p);
      CHECK(book.idle_bytes <= cap);
      size_t sum = 0;
      for (auto& e : book.idle) sum += e.bytes;
      CHECK(sum == book.idle_bytes);
    }
    CHECK(book.live.size() == mine.size());
  }
  CHECK(reused > 1000 && driver_allocs > 10);
  // a block that is not the pool's, pooling off, a block over the cap
  {
    std::vector<void*> evict;
    int dummy;
    CHECK(!book.give_back(&dummy, cap, true, &evict) && evict.empty());
    void* p = malloc(16);
    book.adopt(p, 0, 64u << 20);
    CHECK(!book.give_back(p, cap, false, &evict));
    free(p);
    p = malloc(16);
    book.adopt(p, 0, cap + 1);
    CHECK(!book.give_back(p, cap, true, &evict));
    free(p);
  }
  // retire a device: nothing while one of its blocks is in use, everything once none is
  for (auto& m : mine) {
    std::vector<void*> evict;
    if (!book.give_back(m.first, cap, true, &evict)) free(m.first);
    for (void* q : evict) free(q);
  }
  mine.clear();
  void* busy = malloc(16);
  book.adopt(busy, 1, 64u << 20);
  CHECK(book.retire_device(1).empty());
  {
    std::vector<void*> evict;
    if (!book.give_back(busy, cap, true, &evict)) free(busy);
    for (void* q : evict) free(q);
  }
  for (void* q : book.retire_device(1)) free(q);
  for (auto& e : book.idle) CHECK(e.dev == 0);
  for (void* q : book.flush()) free(q);
  CHECK(book.idle.empty() && book.idle_bytes == 0 && book.live.empty());
}

static void test_row_sets() {
  double w0[4], w1[4];
  const void* rw[16] = {w0, w0, nullptr, w1, w0, nullptr, w1, w1, w0, nullptr, nullptr, w1, w0, w0, w1, nullptr};
  int64_t ne[16];
  for (int l = 0; l < 16; ++l) ne[l] = rw[l] == w0 ? 80 : (rw[l] == w1 ? 80 : 0);
  ne[13] = 70;  // same weights, another scaling: a set of its own
  int set_of[16], set_lane[16];
  const int n = row_sets(16, rw, ne, set_of, set_lane);
  CHECK(n == 4);
  for (int l = 0; l < 16; ++l) {
    CHECK(set_of[l] >= 0 && set_of[l] < n);
    const int rep = set_lane[set_of[l]];
    CHECK(rep <= l && rw[rep] == rw[l] && ne[rep] == ne[l]);
    for (int m = 0; m < 16; ++m) CHECK((set_of[m] == set_of[l]) == (rw[m] == rw[l] && ne[m] == ne[l]));
  }
  for (int s = 0; s + 1 < n; ++s) CHECK(set_lane[s] < set_lane[s + 1]);  // in order of their first lane
  CHECK(row_sets(1, rw, ne, set_of, set_lane) == 1 && set_of[0] == 0 && set_lane[0] == 0);
}

static void test_interleaved() {
  for (int B = 1; B <= 32; ++B)  // (a shared path runs on up to thirty-two lanes)
    for (int64_t total = B; total <= 200; ++total)
      for (int tail = 0; tail < 3; ++tail) {  // (2: the slack of a three-pass path to the deepest lanes of the first band)
        std::vector<int> seen((size_t)total, 0);
        int64_t most = 0;
        for (int l = 0; l < B; ++l) {
          const LaneWalk w = interleaved_walk(l, B, total, tail != 0, tail == 2);
          int64_t mine = 0;
          for (int k = w.first; k < w.n_points; k += w.stride) {
            seen[(size_t)k] += 1;
            ++mine;
          }
          if (w.tail_pt >= 0) {
            CHECK(w.tail_pt >= w.n_points && w.tail_pt < total);
            seen[(size_t)w.tail_pt] += 1;
            ++mine;
          }
          CHECK(mine == interleaved_points(w));
          most = std::max(most, mine);
        }
        for (int64_t k = 0; k < total; ++k) CHECK(seen[(size_t)k] == 1);  // every point exactly once
        CHECK(most == (total + B - 1) / B);                               // and no lane walks more than its share
      }
  {  // 50 points on eighteen lanes: lanes 16 and 17 own points 16 and 17 alone, lane l < 16 owns l, 18 + l and 34 + l
    const LaneWalk a = interleaved_walk(16, 18, 50, true, true), b = interleaved_walk(3, 18, 50, true, true);
    CHECK(a.first == 16 && a.n_points == 18 && a.tail_pt == -1 && interleaved_points(a) == 1);
    CHECK(b.first == 3 && b.n_points == 34 && b.stride == 18 && b.tail_pt == 37 && interleaved_points(b) == 3);
  }
  const LaneWalk w = interleaved_walk(15, 16, 50, true);  // the headline: 48 regular points, 48 and 49 go to lanes 14, 15
  CHECK(w.n_points == 48 && w.tail_pt == 49 && interleaved_walk(14, 16, 50, true).tail_pt == 48 && interleaved_walk(13, 16, 50, true).tail_pt == -1);
}

static void test_auto_lanes() {
  // (points, cap, working-set solve over a large X, lanes beyond twenty allowed)
  // interleaved lanes: sixteen unless eighteen or twenty save a pass; never more than the kernels serve
  CHECK(auto_path_lanes(50, 32, true, false) == 18 && auto_path_lanes(50, 32, false, false) == 16 && auto_path_lanes(50, 16, true, false) == 16);
  CHECK(auto_path_lanes(100, 32, true, false) == 20 && auto_path_lanes(32, 32, true, false) == 16 && auto_path_lanes(36, 32, true, false) == 18);
  CHECK(auto_path_lanes(40, 32, true, false) == 20 && auto_path_lanes(41, 32, true, false) == 16 && auto_path_lanes(7, 32, true, false) == 7);
  CHECK(auto_path_lanes(1, 4, false, false) == 1 && auto_path_lanes(9, 4, false, true) == 4 && auto_path_lanes(0, 32, true, true) == 1);
  // contiguous ranges: up to thirty-two -- 50 points in two passes of twenty-five
  CHECK(auto_path_lanes(50, 32, true, true) == 25 && auto_path_lanes(60, 32, true, true) == 30 && auto_path_lanes(36, 32, true, true) == 18);
  CHECK(auto_path_lanes(64, 32, true, true) == 32 && auto_path_lanes(100, 32, true, true) == 25 && auto_path_lanes(17, 32, true, true) == 17);
  for (int64_t k = 1; k <= 400; ++k)
    for (int cap : {1, 4, 6, 16, 32})
      for (int big = 0; big < 2; ++big)
        for (int wide = 0; wide < 2; ++wide) {
          const int b = auto_path_lanes(k, cap, big != 0, wide != 0);
          const int64_t narrow = std::min<int64_t>(std::min(cap, 16), k);
          CHECK(b >= 1 && b <= cap && b <= k && b <= (wide ? 32 : 20));
          CHECK((k + b - 1) / b <= (k + narrow - 1) / narrow);  // never more passes than sixteen lanes take
          if (!big) CHECK(b == narrow);
        }
}

static void test_grid() {
  for (int cus : {1, 64, 256, 304})
    for (int64_t ld : {16, 512, 528, 5008, 10240, 16384})
      for (int64_t n : {1, 7, 8, 9, 1000, 5008, 100000, 1000003}) {
        const int most = xtr_row_blocks_most(cus, ld, 512);
        CHECK(most >= 1);
        for (int64_t want : {(int64_t)0, (int64_t)1, (int64_t)(most / 2), (int64_t)most}) {
          const XtrGrid g = xtr_grid(n, ld, 512, want);
          CHECK(g.xb * 512 >= ld && (g.xb - 1) * 512 < ld);
          CHECK(g.rows % 8 == 0 && g.rows >= 8);
          CHECK((int64_t)g.yb * g.rows >= n && (int64_t)(g.yb - 1) * g.rows < n);  // the blocks cover the rows, none is empty
          CHECK(g.yb <= std::max<int64_t>(1, want));
        }
      }
}

struct Entry { double fp1, fp2, n_eff; };
static void test_find_and_tiles() {
  std::vector<Entry> e = {{1.0, 2.0, 80.0}, {1.0, 2.0, 70.0}, {3.0, 2.0, 80.0}};
  CHECK(find_by_fingerprint(e, 1.0, 2.0, 70.0) == 1 && find_by_fingerprint(e, 3.0, 2.0, 80.0) == 2);
  CHECK(find_by_fingerprint(e, 1.0, 2.5, 80.0) == -1 && find_by_fingerprint(std::vector<Entry>(), 0, 0, 0) == -1);
  int t = 0;
  for (int I = 0; I < 300; ++I)
    for (int J = 0; J <= I; ++J, ++t) {
      int a, b, c, d;
      triangle_tile(t, &a, &b);
      triangle_tile_fast(t, &c, &d);
      CHECK(a == I && b == J && c == I && d == J);
    }
  CHECK(triangle_tiles(300) == t);
  for (int tt : {(1 << 24) - 1, 1 << 24, 8256 * 16 - 1, 33550336}) {  // far beyond any triangle the engine builds
    int a, b, c, d;
    triangle_tile(tt, &a, &b);
    triangle_tile_fast(tt, &c, &d);
    CHECK(a == c && b == d && a * (a + 1) / 2 + b == tt && b <= a);
  }
  CHECK(model_gram_cap(5008, 3.0e9, 16) == 16 && model_gram_cap(10000, 3.0e9, 16) == 7 && model_gram_cap(16384, 3.0e9, 16) == 2 &&
        model_gram_cap(100000, 3.0e9, 16) == 1);
}

// explicit sixteen-lane paths of 33 to 47 points under slack_deep (advisor, round 5): 48 slots, the slack goes to the lanes
// that hold the deepest points of the first band -- they own that one point -- and every point is owned exactly once
static void test_interleaved_sixteen_lanes() {
  for (int total = 33; total <= 47; ++total) {
    std::vector<int> owner(total, -1);
    const int64_t e = (48 - total) / 2, F = 16 - e;
    for (int lane = 0; lane < 16; ++lane) {
      const LaneWalk w = interleaved_walk(lane, 16, total, true, true);
      std::vector<int> pts;
      for (int q = w.first; q < w.n_points; q += w.stride) pts.push_back(q);
      if (w.tail_pt >= 0) pts.push_back(w.tail_pt);
      CHECK((int64_t)pts.size() == interleaved_points(w));
      if (e >= 1) {
        if (lane >= F) CHECK(pts.size() == 1 && pts[0] == lane);  // the deepest points of the first band: one point each
        else CHECK(pts.size() >= 2 && pts[0] == lane && pts[1] == 16 + lane);
      }
      for (int q : pts) {
        CHECK(q >= 0 && q < total && owner[q] == -1);
        if (q >= 0 && q < total) owner[q] = lane;
      }
    }
    for (int q = 0; q < total; ++q) CHECK(owner[q] >= 0);
    if (total == 40) {  // (the advisor's example: e = 4, lanes 12..15 own a single point; lanes 0..11 own l, 16 + l, 28 + l)
      CHECK(interleaved_walk(12, 16, 40, true, true).tail_pt == -1 && interleaved_walk(12, 16, 40, true, true).n_points == 16);
      CHECK(interleaved_walk(0, 16, 40, true, true).tail_pt == 28 && interleaved_walk(11, 16, 40, true, true).tail_pt == 39);
    }
  }
}

// what normal use runs with: nothing set
static void check_defaults(const Knobs& d) {
  CHECK(d.split && d.on_chip && d.interleave && d.carry && d.ws_carry);
  CHECK(d.ws == -1 && d.mg == -1 && d.grad_ring == -1 && d.rowdot_ring == -1 && d.auto_lanes == 0 && d.trace == 0);
  CHECK(d.ws_theta == 0.85 && d.ws_append == 48 && d.ws_kinit == 0 && d.ws_fill == 0.0);
  CHECK(d.sample_start && d.sample_min_rows == 65536 && d.sample_div == 4);
  CHECK(d.device_pool_gb < 0.0 && !d.allow_any_arch && d.xtr_wgs_per_cu == 1.0 && d.handover);
  CHECK(!d.eval_fused && d.power_iters == 0 && d.grad_cfg[0] == 0);
  CHECK(d.light_pass && d.gram_owner && d.lag_handover && d.ws_miss_factor == 4 && d.ws_miss_div == 8);  // (round 6)
}

// the SLM_* knobs: read once into a struct (round-5 verdict, item 5) -- defaults, every kind of field, clamping, reload
static void test_knobs() {
  std::map<std::string, std::string> env;
  auto get = [&](const char* name) -> const char* {
    auto it = env.find(name);
    return it == env.end() ? nullptr : it->second.c_str();
  };
  check_defaults(Knobs::from(get));
  // the settings that were knobs once keep the values they defaulted to
  CHECK(kSketchPowerIters == 1 && kSketchRowDiv == 32 && kWsLookahead == 2 && kWsPowerIters == 10);
  // the retired variables, each at its former non-default value: read by nothing
  for (const char* name : {"SLM_XTR_EXTRAS", "SLM_ROWDOT32", "SLM_MG_SYRK"}) env[name] = "0";
  for (const char* name : {"SLM_NO_RESID32", "SLM_NO_SLACK_DEEP", "SLM_NO_DIRECT", "SLM_NO_L_SKETCH", "SLM_NO_SKETCH_CACHE",
                           "SLM_NO_MG_KEEP", "SLM_NO_SMALL_STAGE", "SLM_NO_WIDE_LANES", "SLM_SAMPLE_START_ALL", "SLM_COV_ALL_ROWS",
                           "SLM_ON_CHIP_NO_FALLBACK", "SLM_PROFILE_UNIT", "SLM_NO_DEVICE_POOL"})
    env[name] = "1";
  env["SLM_L_SKETCH_ITERS"] = "3"; env["SLM_L_SKETCH_DIV"] = "16"; env["SLM_WS_LOOKAHEAD"] = "4";
  env["SLM_WS_POWER_ITERS"] = "20"; env["SLM_GRAD_BLOCKS_PER_CU"] = "2";
  check_defaults(Knobs::from(get));
  env.clear();
  env["SLM_WS"] = "0"; env["SLM_MG"] = "2"; env["SLM_TRACE"] = "3"; env["SLM_TRACE_POLL"] = "1"; env["SLM_SPLIT"] = "0";
  env["SLM_GRAD_CONFIG"] = "8,5,2"; env["SLM_WS_THETA"] = "0.7"; env["SLM_WS_APPEND"] = "9999"; env["SLM_WS_KINIT"] = "3";
  env["SLM_SAMPLE_DIV"] = "0"; env["SLM_SAMPLE_START_MIN_ROWS"] = "10"; env["SLM_XTR_WGS_PER_CU"] = "7"; env["SLM_NO_CARRY"] = "";
  env["SLM_DEVICE_POOL_GB"] = "-3"; env["SLM_ROWDOT_RING"] = "1"; env["SLM_GRAD_RING"] = "0"; env["SLM_AUTO_LANES"] = "20";
  env["SLM_WS_FILL"] = "5"; env["SLM_POWER_ITERS"] = "1"; env["SLM_ON_CHIP"] = "0";
  env["SLM_NO_LIGHT_PASS"] = "1"; env["SLM_NO_GRAM_OWNER"] = ""; env["SLM_NO_LAG_HANDOVER"] = "1"; env["SLM_WS_MISS_DIV"] = "0"; env["SLM_WS_MISS_FACTOR"] = "99";
  Knobs k = Knobs::from(get);
  CHECK(!k.light_pass && !k.gram_owner && !k.lag_handover && k.ws_miss_div == 1 && k.ws_miss_factor == 8);
  CHECK(k.ws == 0 && k.mg == 2 && k.trace == 3 && k.trace_poll && !k.split && !k.on_chip);
  CHECK(k.grad_cfg[0] == 8 && k.grad_cfg[1] == 5 && k.grad_cfg[2] == 2 && k.ws_theta == 0.7);
  CHECK(k.ws_append == 512 && k.ws_kinit == 16 && k.sample_div == 1 && k.sample_min_rows == 64);  // clamped to their ranges
  CHECK(k.xtr_wgs_per_cu == 1.0);  // (outside (0, 2]: ignored)
  CHECK(!k.carry && k.ws_carry && k.device_pool_gb == 0.0 && k.rowdot_ring == 1 && k.grad_ring == 0 && k.auto_lanes == 20);
  CHECK(k.ws_fill == 1.0 && k.power_iters == 2);
  env["SLM_WS"] = "1"; env["SLM_MG"] = "0"; env["SLM_TRACE"] = "yes"; env["SLM_WS_THETA"] = "1.5"; env.erase("SLM_SPLIT");
  k = Knobs::from(get);  // a second read follows the environment (slm_reload_knobs)
  CHECK(k.ws == 1 && k.mg == 0 && k.trace == 1 && k.ws_theta == 0.85 && k.split);
}


// ---- csrc/tail_logic.hpp --------------------------------------------------------------------------------------------
// A lane in the middle of a point: L = 4, ak = 2, Lhat = 3, one accepted value (10) in the ring, pen_z = 0.5, loss_z = 1.
// The numbers are small dyadic ones wherever a check is an equality, so that no rounding is involved.
static const double kFloor = 16.0 * 2.220446049250313e-16;  // kRoundFloor: a copy, the HIP header that defines it (tail_kernels.hpp) cannot be
                                                            // included here; the checks below need a floor, not this value
static TailSnap tail_snap(int mode, double loss_z = 1.0, bool provisional = false) {
  TailSnap c{};
  c.point = 1; c.n_points = 4; c.pt_lo = 0; c.stride = 1; c.tail_pt = -1;
  c.iter = 3; c.max_iter = 1000; c.total_iter = 10; c.flags = 0;
  c.mode = mode; c.have_base = 1; c.rejects = 0; c.n_hist = 1;
  c.t = 2.0; c.L = 4.0; c.tol = 1e-6; c.ak = 2.0; c.Lhat = 3.0; c.pen_z = 0.5; c.mu = 0.0; c.mu_rq = 0.0; c.loss_base = 7.0;
  c.hist[0] = 10.0;
  for (int k = 1; k < BB_HIST; ++k) c.hist[k] = 1000.0;  // (beyond n_hist: stale, never to be looked at)
  tail_snap_call(c, loss_z, provisional, kFloor);
  return c;
}

static void test_tail_snapshot() {
  TailSnap c = tail_snap(1, 8.0);
  CHECK(!c.hit_max && !c.cold && !c.provisional && c.loss_z == 8.0 && c.bnorm_floor == 1e-10 * sqrt(2.0 * 8.0 / 4.0));
  c.Lhat = 16.0; c.flags = SLM_FLAG_COLD_START; c.max_iter = c.iter + 1;
  tail_snap_call(c, -1.0, true, kFloor);  // (a loss below zero counts as zero; the larger of L and Lhat scales the floor)
  CHECK(c.hit_max && c.cold && c.provisional && c.bnorm_floor == 0.0);
  c.max_iter = c.iter + 2;
  tail_snap_call(c, 8.0, false, kFloor);
  CHECK(!c.hit_max && c.bnorm_floor == 1e-10 * sqrt(2.0 * 8.0 / 16.0));
  const TailNext n = tail_next(c);
  CHECK(n.mode == c.mode && n.have_base == c.have_base && n.rejects == c.rejects && n.n_hist == c.n_hist && n.t == c.t && n.L == c.L &&
        n.ak == c.ak && n.Lhat == c.Lhat && n.pen_z == c.pen_z && n.mu_rq == c.mu_rq && n.loss_base == c.loss_base);
  CHECK(n.stored && !n.finalize && !n.conv && !n.nonfinite && !n.did_restart && !n.l_bad && !n.fallback);
}

static void test_bb_decide() {
  {  // first call of a point: the start point is the base whatever the ring held, its penalty is s[4]
    TailSnap c = tail_snap(1);
    c.have_base = 0; c.n_hist = 3;
    TailNext n = tail_next(c);
    const double s[6] = {1.0, 1.0, 1.0, 0.0, 0.25, 4.0};
    CHECK(bb_decide(c, n, s));
    CHECK(n.n_hist == 1 && n.hist[0] == 1.25 && n.have_base == 1 && n.loss_base == 1.0 && n.stored && !n.nonfinite && !n.fallback);
    CHECK(n.ak == 2.0 && n.Lhat == 3.0 && n.rejects == 0 && n.mu_rq == 0.0);
  }
  // accept and reject against a ring of 1, BB_HIST - 1 and BB_HIST entries: the reference is the largest VALID entry
  // (top), the candidate must lie below it by sigma/2 ak ||dz||^2 = 1e-4
  for (int nh : {1, BB_HIST - 1, BB_HIST})
    for (int accept_it = 0; accept_it < 2; ++accept_it)
      for (int top_at = 0; top_at < nh; top_at += (nh > 1 ? nh - 1 : 1)) {  // the largest entry first, or last
        const double top = 20.0;
        TailSnap c = tail_snap(1, accept_it ? top - 1.5 : top - 0.5);  // F(z) = loss_z + pen_z = top - 1 | top
        c.n_hist = nh; c.mu_rq = 1.5;
        for (int k = 0; k < nh; ++k) c.hist[k] = 10.0 + k;
        c.hist[top_at] = top;
        TailNext n = tail_next(c);
        const double s[6] = {1.0, 2.0, 9.0, 0.0, 99.0, 4.0};
        const bool accept = bb_decide(c, n, s);
        CHECK(accept == (accept_it != 0) && n.stored == accept && !n.nonfinite && !n.fallback);
        if (accept) {
          CHECK(n.Lhat == 3.0 && n.ak == 2.0 && n.mu_rq == 1.5 && n.rejects == 0 && n.have_base == 1 && n.loss_base == c.loss_z);
          if (nh < BB_HIST) {
            CHECK(n.n_hist == nh + 1 && n.hist[nh] == top - 1.0);
            for (int k = 0; k < nh; ++k) CHECK(n.hist[k] == c.hist[k]);
          } else {  // full: the oldest value leaves
            CHECK(n.n_hist == BB_HIST && n.hist[BB_HIST - 1] == top - 1.0);
            for (int k = 0; k + 1 < BB_HIST; ++k) CHECK(n.hist[k] == c.hist[k + 1]);
          }
        } else {
          CHECK(n.ak == 4.0 && n.rejects == 1 && n.n_hist == nh && n.Lhat == 3.0 && n.mu_rq == 1.5 && n.loss_base == 7.0);
          for (int k = 0; k < BB_HIST; ++k) CHECK(n.hist[k] == c.hist[k]);
        }
      }
  {  // the margin itself: just below the reference is not enough
    TailSnap c = tail_snap(1, 10.0 - 0.5 - 0.5e-4);
    TailNext n = tail_next(c);
    const double s[6] = {1.0, 2.0, 9.0, 0.0, 0.0, 4.0};
    CHECK(!bb_decide(c, n, s));
    c = tail_snap(1, 10.0 - 0.5 - 2e-4);
    n = tail_next(c);
    CHECK(bb_decide(c, n, s));
  }
  // ak: the quotient <dz,dg>/<dz,dz>, Lhat where that is not positive, unchanged for a zero step; clamped to
  // [1e-6, 1e6] Lhat; a larger curvature ||dg||/||dz|| raises Lhat; the first quotient of a point starts mu_rq
  struct { double s0, s1, s2, ak, Lhat, mu_rq; } cases[] = {
      {1.0, 2.0, 9.0, 2.0, 3.0, 2.0},        {1.0, 2.0, 25.0, 2.0, 5.0, 2.0},           {1.0, 1e-9, 9.0, 1e-6 * 3.0, 3.0, 1e-6 * 3.0},
      {1.0, 1e8, 9.0, 1e6 * 3.0, 3.0, 1e6 * 3.0}, {1.0, -1.0, 9.0, 3.0, 3.0, 0.0}, {0.0, 0.0, 0.0, 2.0, 3.0, 0.0}};
  for (const auto& k : cases) {
    const TailSnap c = tail_snap(1, 0.0);
    TailNext n = tail_next(c);
    const double s[6] = {k.s0, k.s1, k.s2, 0.0, 0.0, 4.0};
    CHECK(bb_decide(c, n, s));
    CHECK(n.ak == k.ak && n.Lhat == k.Lhat && n.mu_rq == k.mu_rq);
  }
  {  // a rejected step doubles ak, up to 1e6 Lhat
    TailSnap c = tail_snap(1, 100.0);
    c.ak = 2e6;
    TailNext n = tail_next(c);
    const double s[6] = {1.0, 2.0, 9.0, 0.0, 0.0, 4.0};
    CHECK(!bb_decide(c, n, s) && n.ak == 1e6 * 3.0);
  }
  // mu_rq is left alone when the step is at the rounding level of the iterate (first) or of the gradient (second)
  for (int which = 0; which < 2; ++which) {
    TailSnap c = tail_snap(1, 0.0);
    c.mu_rq = 0.75;
    TailNext n = tail_next(c);
    const double s[6] = {which ? 1.0 : 1e-30, which ? 1.0 : 1e-30, which ? 1e-10 : 1e-30, 0.0, 0.0, 1e12};
    CHECK(bb_decide(c, n, s) && n.mu_rq == 0.75 && n.ak == 1.0);
  }
  // fallback: at exactly BB_REJECT_LIMIT rejects, and when the call is iteration BB_POINT_LIMIT + 1 of its point
  for (int rej = 0; rej < BB_REJECT_LIMIT; ++rej)
    for (int accept_it = 0; accept_it < 2; ++accept_it) {
      TailSnap c = tail_snap(1, accept_it ? 0.0 : 100.0);
      c.rejects = rej;
      TailNext n = tail_next(c);
      const double s[6] = {1.0, 2.0, 25.0, 0.0, 0.0, 4.0};
      CHECK(bb_decide(c, n, s) == (accept_it != 0));
      CHECK(n.fallback == (!accept_it && rej == BB_REJECT_LIMIT - 1));
      if (n.fallback) {
        bb_fallback(c, n);
        CHECK(n.mode == 0 && n.t == 1.0 && n.L == 4.0 && !n.finalize && n.rejects == BB_REJECT_LIMIT);
      }
    }
  for (int it : {BB_POINT_LIMIT - 1, BB_POINT_LIMIT}) {
    TailSnap c = tail_snap(1, 0.0);
    c.iter = it;
    c.max_iter = BB_POINT_LIMIT + 1;
    tail_snap_call(c, 0.0, false, kFloor);
    TailNext n = tail_next(c);
    const double s[6] = {1.0, 2.0, 25.0, 0.0, 0.0, 4.0};
    CHECK(bb_decide(c, n, s) && n.fallback == (it == BB_POINT_LIMIT));
    if (n.fallback) {  // FISTA takes the largest curvature seen; a point out of iterations is reported as it stands
      bb_fallback(c, n);
      CHECK(n.mode == 0 && n.t == 1.0 && n.L == 5.0 && c.hit_max && n.finalize && tail_status(n) == SLM_ERR_NOT_CONVERGED);
    }
  }
  {  // a non-finite gradient or objective: no fallback, the point ends in bb_stop
    TailSnap c = tail_snap(1, 100.0);
    c.rejects = BB_REJECT_LIMIT - 1;
    TailNext n = tail_next(c);
    const double s[6] = {1.0, 2.0, 9.0, 1.0, 0.0, 4.0};
    CHECK(!bb_decide(c, n, s) && n.nonfinite && !n.fallback);
    c = tail_snap(1, INFINITY);
    n = tail_next(c);
    const double s2[6] = {1.0, 2.0, 9.0, 0.0, 0.0, 4.0};
    bb_decide(c, n, s2);
    CHECK(n.nonfinite && !n.fallback);
  }
}

static void test_bb_stop() {
  const double s[6] = {1.0, 2.0, 9.0, 0.0, 0.0, 4.0};
  auto run = [&](TailSnap c, const double (&q)[4]) {
    TailNext n = tail_next(c);
    CHECK(bb_decide(c, n, s));
    bb_stop(c, n, s, q);
    return n;
  };
  const double far[4] = {1.0, 1.0, 0.125, 0.0}, there[4] = {0.0, 1.0, 0.125, 0.0};
  TailNext n = run(tail_snap(1, 0.0), far);
  CHECK(!n.conv && !n.finalize && !n.nonfinite && n.pen_z == 0.125 && n.resid == 1.0 && n.bnorm == 1.0 && n.kkt == 2.0 && n.mu_eff == 2.0);
  {  // mu: the smallest of ak, Lhat, the point's quotients and the model solver's estimate, floored at kMuFloor Lhat
    TailSnap c = tail_snap(1, 0.0);
    c.mu_rq = 1.5;
    CHECK(run(c, far).mu_eff == 1.5);
    c.mu = 0.5;
    CHECK(run(c, far).mu_eff == 0.5);
    c.mu = 1e-9;
    CHECK(run(c, far).mu_eff == kMuFloor * 3.0);
    c = tail_snap(1, 0.0);
    c.ak = 8.0;  // (a step shorter than 1 / Lhat: the residual is reported at the scale of Lhat)
    const double s0[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 4.0};
    TailNext m = tail_next(c);
    CHECK(bb_decide(c, m, s0) && m.ak == 8.0);
    bb_stop(c, m, s0, far);
    CHECK(m.resid == 8.0 / 3.0 && m.kkt == 8.0 && m.mu_eff == 3.0);
  }
  n = run(tail_snap(1, 0.0), there);
  CHECK(n.conv && n.finalize && tail_status(n) == SLM_OK && n.kkt == 0.0);
  n = run(tail_snap(1, 0.0, true), there);  // an estimated gradient accepts no point
  CHECK(!n.conv && !n.finalize);
  {  // the rule itself: kkt <= tol * ||c|| * mu, one ulp either side (q[1] = 1, mu = ak = 2: the bound is 2 tol)
    TailSnap c = tail_snap(1, 0.0);
    c.tol = 0.25;
    const double in[4] = {0.0625, 1.0, 0.0, 0.0}, out[4] = {0.0625 * (1.0 + 1e-15), 1.0, 0.0, 0.0};
    CHECK(run(c, in).conv && !run(c, out).conv);
    const double tiny[4] = {0.0625, 1e-40, 0.0, 0.0};  // ||c|| below the floor: the floor stands in
    CHECK(c.bnorm_floor == 0.0 && !run(c, tiny).conv);
    c.hist[0] = 1e21;
    tail_snap_call(c, 8e20, false, kFloor);  // (rms residual / sqrt(L) = sqrt(2 * 8e20 / 4): the floor is 1e-10 of it)
    CHECK(c.bnorm_floor == 2.0 && run(c, tiny).conv);
  }
  {
    TailSnap c = tail_snap(1, 0.0);
    c.max_iter = c.iter + 1;
    tail_snap_call(c, 0.0, false, kFloor);
    n = run(c, far);
    CHECK(!n.conv && n.finalize && tail_status(n) == SLM_ERR_NOT_CONVERGED);
  }
  const double bad1[4] = {1.0, 1.0, 0.0, 1.0}, bad2[4] = {INFINITY, 1.0, 0.0, 0.0}, bad3[4] = {0.0, NAN, 0.0, 0.0};
  for (const auto* q : {&bad1, &bad2, &bad3}) {
    n = run(tail_snap(1, 0.0), *q);
    const TailRoute r = tail_route(tail_snap(1, 0.0), n, true);
    CHECK(n.nonfinite && n.finalize && tail_status(n) == SLM_ERR_NON_FINITE && !r.range_end && !r.goes_idle && !r.secant);
  }
}

static void test_fista_decide() {
  //                 ||b+-z||^2 ||b+||^2 restart ||dg||^2 ||dz||^2 ||z||^2 bad ||g||^2 <dg,dz>
  const double plain[9] = {1.0, 1.0, -1.0, 4.0, 1.0, 1.0, 0.0, 4.0, 2.0};
  TailSnap c = tail_snap(0);
  TailNext n = tail_next(c);
  fista_decide(c, n, plain);
  const double t17 = 0.5 * (1.0 + sqrt(17.0));
  CHECK(!n.l_bad && !n.did_restart && !n.conv && !n.finalize && n.L == 4.0 && n.t == t17 && n.mom == 1.0 / t17);
  CHECK(n.resid == 1.0 && n.bnorm == 1.0 && n.kkt == 4.0 && n.mu_rq == 2.0 && n.mu_eff == 2.0 && n.loss_base == 1.0 && n.stored);
  c.mu = 0.5; c.mu_rq = 1.0;
  n = tail_next(c);
  fista_decide(c, n, plain);
  CHECK(n.mu_rq == 1.0 && n.mu_eff == 0.5);
  {  // the curvature guard: ||dg||/||dz|| = 10 > L raises L to 1.02 * 10, drops the momentum and forbids conv, even at a
     // fixed point of the step; exactly L does not trip it, and neither does the first call of a solve or a move of z at the rounding level
    const double bad[9] = {0.0, 1.0, -1.0, 100.0, 1.0, 1.0, 0.0, 4.0, 2.0};
    c = tail_snap(0);
    n = tail_next(c);
    fista_decide(c, n, bad);
    CHECK(n.l_bad && n.L == 1.02 * 10.0 && n.t == 1.0 && !n.conv && !n.finalize && n.kkt == 0.0);
    const double edge[9] = {0.0, 1.0, -1.0, 16.0, 1.0, 1.0, 0.0, 4.0, 2.0};
    n = tail_next(c);
    fista_decide(c, n, edge);
    CHECK(!n.l_bad && n.L == 4.0 && n.conv && n.finalize && tail_status(n) == SLM_OK);
    c.total_iter = 0;
    n = tail_next(c);
    fista_decide(c, n, bad);
    CHECK(!n.l_bad && n.L == 4.0 && n.mu_rq == 0.0);
    c = tail_snap(0);
    const double still[9] = {0.0, 1.0, -1.0, 100e-13, 1e-13, 1.0, 0.0, 4.0, 2.0};
    n = tail_next(c);
    fista_decide(c, n, still);
    CHECK(!n.l_bad && n.L == 4.0);
  }
  {  // restart when the step turns against the last move, unless the caller forbids it
    const double back[9] = {1.0, 1.0, 0.5, 4.0, 1.0, 1.0, 0.0, 4.0, 2.0};
    c = tail_snap(0);
    n = tail_next(c);
    fista_decide(c, n, back);
    CHECK(n.did_restart && n.mom == 0.0 && n.t == 0.5 * (1.0 + sqrt(5.0)));
    c.flags = SLM_FLAG_NO_RESTART;
    n = tail_next(c);
    fista_decide(c, n, back);
    CHECK(!n.did_restart && n.t == t17 && n.mom == 1.0 / t17);
  }
  const double there[9] = {0.0, 1.0, -1.0, 4.0, 1.0, 1.0, 0.0, 4.0, 2.0};
  c = tail_snap(0, 1.0, true);
  n = tail_next(c);
  fista_decide(c, n, there);
  CHECK(!n.conv && !n.finalize);
  c = tail_snap(0);
  c.max_iter = c.iter + 1;
  tail_snap_call(c, 1.0, false, kFloor);
  n = tail_next(c);
  fista_decide(c, n, plain);
  CHECK(!n.conv && n.finalize && tail_status(n) == SLM_ERR_NOT_CONVERGED);
  for (int which = 0; which < 4; ++which) {  // a non-finite count, sum or loss ends the point and the path
    double s[9];
    for (int k = 0; k < 9; ++k) s[k] = plain[k];
    if (which == 0) s[6] = 1.0;
    if (which == 1) s[0] = NAN;
    if (which == 2) s[1] = INFINITY;
    c = tail_snap(0, which == 3 ? NAN : 1.0);
    c.point = 3;  // (the last point of the range: it would otherwise end the range)
    n = tail_next(c);
    fista_decide(c, n, s);
    const TailRoute r = tail_route(c, n, false);
    CHECK(n.nonfinite && n.finalize && tail_status(n) == SLM_ERR_NON_FINITE && !r.range_end && !r.goes_idle);
  }
}

static void test_tail_route() {
  TailNext done = tail_next(tail_snap(1)), going = done;
  done.finalize = true;
  for (int steal = 0; steal < 2; ++steal) {
    TailSnap c = tail_snap(1);  // points 0..3, the lane stands on 1
    TailRoute r = tail_route(c, done, steal != 0);
    CHECK(r.secant && !r.range_end && !r.goes_idle && r.next_point == 2);
    r = tail_route(c, going, steal != 0);  // (an unfinished point moves nothing)
    CHECK(!r.secant && !r.range_end && !r.goes_idle);
    c.flags = SLM_FLAG_COLD_START;
    tail_snap_call(c, 1.0, false, kFloor);
    CHECK(!tail_route(c, done, steal != 0).secant);
    c = tail_snap(1);
    c.point = 0;  // the first point of the range has no predecessor for the secant ...
    CHECK(!tail_route(c, done, steal != 0).secant && tail_route(c, done, steal != 0).next_point == 1);
    c.point = 2; c.pt_lo = 2;  // ... nor has the first point of a range taken over
    CHECK(!tail_route(c, done, steal != 0).secant);
    c = tail_snap(1);
    c.point = 3;  // the last point, no tail point: the range ends; on a shared path the lane waits for work
    r = tail_route(c, done, steal != 0);
    CHECK(!r.secant && r.range_end && r.goes_idle == (steal != 0) && r.next_point == 4);
    r = tail_route(c, going, steal != 0);
    CHECK(!r.range_end && !r.goes_idle);
    c.tail_pt = 9;  // the last regular point with a tail point to visit: on to it
    r = tail_route(c, done, steal != 0);
    CHECK(!r.range_end && !r.goes_idle && r.next_point == 9);
    c.point = 9;  // the tail point itself (it lies beyond n_points): the range ends
    r = tail_route(c, done, steal != 0);
    CHECK(r.range_end && r.goes_idle == (steal != 0) && r.next_point == 10 && !r.secant);
    // interleaved lanes: every sixteenth point of 48, no secant through the neighbours' points
    c = tail_snap(1);
    c.n_points = 48; c.stride = 16; c.point = 21; c.pt_lo = 5; c.tail_pt = 49;
    r = tail_route(c, done, steal != 0);
    CHECK(!r.secant && !r.range_end && r.next_point == 37);
    c.point = 37;
    r = tail_route(c, done, steal != 0);
    CHECK(!r.range_end && r.next_point == 49);
    c.tail_pt = -1;
    r = tail_route(c, done, steal != 0);
    CHECK(r.range_end && r.next_point == 53);
    c.n_points = 54;  // (one more regular point)
    CHECK(!tail_route(c, done, steal != 0).range_end && tail_route(c, done, steal != 0).next_point == 53);
    c = tail_snap(1);
    c.stride = 0;  // (a control block that never set it walks point by point)
    CHECK(tail_route(c, done, steal != 0).next_point == 2 && tail_route(c, done, steal != 0).secant);
  }
}

// ---- csrc/l0_host.hpp -----------------------------------------------------------------------------------------------
// A 6 x 6 symmetric positive definite matrix with no structure to hide behind (entries from a fixed recurrence), and c.
static void l0_spd6(double* H /* [36] */, double* c /* [6] */) {
  double A[8][6];
  unsigned v = 12345u;
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

// Reference in long double: the Cholesky factor of H on `cols`, w = L^-1 c, beta = L^-T w.
static void l0_reference(const double* H, const double* c, int p, const int* cols, int m, long double L[6][6], long double* w, long double* beta) {
  for (int i = 0; i < m; ++i) {
    for (int j = 0; j <= i; ++j) {
      long double t = H[cols[i] * p + cols[j]];
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = i == j ? sqrtl(t) : t / L[j][j];
    }
    long double t = c[cols[i]];
    for (int k = 0; k < i; ++k) t -= L[i][k] * w[k];
    w[i] = t / L[i][i];
  }
  for (int k = m - 1; k >= 0; --k) {
    long double t = w[k];
    for (int r = k + 1; r < m; ++r) t -= L[r][k] * beta[r];
    beta[k] = t / L[k][k];
  }
}

static bool l0_near(double got, long double want, double rtol) { return fabsl((long double)got - want) <= rtol * fmaxl(1.0L, fabsl(want)); }

static void l0_check_factor(const L0Factor& f, const double* H, const double* c, const int* cols, int m) {
  long double L[6][6], w[6], beta[6], ss = 0.0L;
  l0_reference(H, c, 6, cols, m, L, w, beta);
  CHECK(f.m == m);
  double b[L0_PMAX];
  f.solve(b);
  for (int r = 0; r < m; ++r) {
    CHECK(f.col[r] == cols[r]);
    for (int k = 0; k <= r; ++k) CHECK(l0_near(f.L[r][k], L[r][k], 1e-13));
    CHECK(l0_near(f.w[r], w[r], 1e-13));
    CHECK(l0_near(b[r], beta[r], 1e-12));
    ss += w[r] * w[r];
  }
  CHECK(l0_near(f.ss, ss, 1e-13));
  // ... and the solution solves the normal equations of the block
  for (int r = 0; r < m; ++r) {
    long double t = -(long double)c[cols[r]];
    for (int k = 0; k < m; ++k) t += (long double)H[cols[r] * 6 + cols[k]] * b[k];
    CHECK(fabsl(t) <= 1e-12);
  }
}

static void test_l0_factor() {
  double H[36], c[6];
  l0_spd6(H, c);
  const int all[6] = {0, 1, 2, 3, 4, 5}, some[4] = {4, 1, 5, 2}, after_pop[4] = {0, 1, 2, 5};
  {
    L0Factor f(H, c, 6);
    double ss_at_3 = 0.0;
    for (int j = 0; j < 6; ++j) {
      CHECK(f.push(j));
      l0_check_factor(f, H, c, all, j + 1);  // every prefix of the columns
      if (j == 2) ss_at_3 = f.ss;
    }
    // backtracking: the column count goes down, ss is that of the remaining columns, and the factor grows again from there
    f.pop_to(3);
    CHECK(f.m == 3 && fabs(f.ss - ss_at_3) <= 4e-16 * ss_at_3);
    l0_check_factor(f, H, c, all, 3);
    CHECK(f.push(5));
    l0_check_factor(f, H, c, after_pop, 4);
    f.pop_to(0);
    CHECK(f.m == 0 && f.ss == 0.0);
  }
  {
    L0Factor f(H, c, 6);  // columns out of order: col[] carries the map
    for (int k = 0; k < 4; ++k) CHECK(f.push(some[k]));
    l0_check_factor(f, H, c, some, 4);
  }
  {
    // a dependent column is refused and leaves the factor as it was: x2 = x0 + x1 (the Gram of integer vectors, exact)
    const double X[4][3] = {{1, 2, 3}, {2, -1, 1}, {0, 3, 3}, {-1, 1, 0}};
    double G[9], g[3];
    for (int i = 0; i < 3; ++i) {
      g[i] = (double)(i + 1);
      for (int j = 0; j < 3; ++j) {
        G[i * 3 + j] = 0.0;
        for (int k = 0; k < 4; ++k) G[i * 3 + j] += X[k][i] * X[k][j];
      }
    }
    L0Factor f(G, g, 3);
    CHECK(f.push(0) && f.push(1));
    const double ss = f.ss, l10 = f.L[1][0], w1 = f.w[1];
    CHECK(!f.push(2));
    CHECK(f.m == 2 && f.ss == ss && f.L[1][0] == l10 && f.w[1] == w1 && f.col[0] == 0 && f.col[1] == 1);
    CHECK(!f.push(1));  // (so is a column that is already there)
    CHECK(f.m == 2 && f.ss == ss);
    // a zero column has nothing to bring either
    const double Z[4] = {1.0, 0.0, 0.0, 0.0}, z[2] = {1.0, 0.0};
    L0Factor fz(Z, z, 2);
    CHECK(!fz.push(1) && fz.m == 0 && fz.push(0) && !fz.push(1) && fz.m == 1);
  }
}

// min 1/2 b^T H b - c^T b over |b_j| <= 1 with H = tridiag(1, 2, 1) and c = (3.5, 1.75, 0): the minimiser is
// b = (1, 1/2, -1/4).  There H b - c = (-1, 0, 0): the first coordinate sits at its bound with the gradient pushing outwards,
// the other two are free with a zero gradient -- the KKT conditions of a strictly convex problem, so the point is THE
// minimiser; its value is 1/2 * 3.375 - 4.375 = -2.6875.  (The unconstrained minimiser is (1.75, 0, 0) with the value -3.0625: the box binds.)
static void test_l0_boxed() {
  const double H3[9] = {2, 1, 0, 1, 2, 1, 0, 1, 2}, c3[3] = {3.5, 1.75, 0.0};
  const double want[3] = {1.0, 0.5, -0.25}, value = -2.6875;
  const int cols3[3] = {0, 1, 2};
  for (int polish = 0; polish < 2; ++polish) {
    const double tol = polish ? 1e-14 : 1e-10;  // (the descent stops at a relative change of 1e-12 per sweep; the polish is exact)
    for (int start = 0; start < 2; ++start) {
      double b[3] = {0.0, 0.0, 0.0};
      if (start) {  // from the unconstrained minimiser, as l0_support calls it
        L0Factor f(H3, c3, 3);
        for (int j = 0; j < 3; ++j) CHECK(f.push(j));
        f.solve(b);
        CHECK(fabs(b[0] - 1.75) <= 1e-14 && fabs(b[1]) <= 1e-14 && fabs(b[2]) <= 1e-14);
      }
      const double v = l0_boxed(H3, c3, 3, cols3, 3, 1.0, polish != 0, b);
      CHECK(b[0] == 1.0);
      for (int k = 0; k < 3; ++k) CHECK(fabs(b[k] - want[k]) <= tol);
      CHECK(fabs(v - value) <= tol);
    }
    // the same block scattered over a 5 x 5 matrix whose other entries must not be read
    double H5[25], c5[5] = {1.75, 1e6, 0.0, -1e6, 3.5};
    const int cols5[3] = {4, 0, 2};
    for (int e = 0; e < 25; ++e) H5[e] = 1e6;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) H5[cols5[i] * 5 + cols5[j]] = H3[i * 3 + j];
    double b[3] = {0.0, 0.0, 0.0};
    const double v = l0_boxed(H5, c5, 5, cols5, 3, 1.0, polish != 0, b);
    for (int k = 0; k < 3; ++k) CHECK(fabs(b[k] - want[k]) <= tol);
    CHECK(fabs(v - value) <= tol);
    // a box nothing touches leaves the unconstrained minimiser; a box of zero leaves nothing
    double wide[3] = {0.0, 0.0, 0.0}, none[3] = {0.3, -0.2, 0.1};
    CHECK(fabs(l0_boxed(H3, c3, 3, cols3, 3, 100.0, polish != 0, wide) + 3.0625) <= 1e-9);
    CHECK(fabs(wide[0] - 1.75) <= 1e-9 && fabs(wide[1]) <= 1e-9 && fabs(wide[2]) <= 1e-9);
    CHECK(l0_boxed(H3, c3, 3, cols3, 3, 0.0, polish != 0, none) == 0.0 && none[0] == 0.0 && none[1] == 0.0 && none[2] == 0.0);
  }
  // through l0_support: three groups of one column, all included, big_M = 1
  double beta[3];
  const std::vector<int> gstart = {0, 1, 2, 3};
  CHECK(fabs(l0_support(H3, c3, 3, gstart, 7ull, 1.0, true, beta) - value) <= 1e-14);
  for (int k = 0; k < 3; ++k) CHECK(fabs(beta[k] - want[k]) <= 1e-14);
  // two of the three: b_1 is out of the support and stays at zero; min over (b_0, b_2) separates: b_0 = 1 (1.75 clipped), b_2 = 0
  CHECK(fabs(l0_support(H3, c3, 3, gstart, 5ull, 1.0, true, beta) - (1.0 - 3.5)) <= 1e-14);
  CHECK(beta[0] == 1.0 && beta[1] == 0.0 && beta[2] == 0.0);
}

static void test_l0_support_skips_dependent_columns() {
  // columns x0, x1 = 2 x0, x2, x3 in two groups {0, 1}, {2, 3}: the Gram of integer vectors, exact
  const double X[5][4] = {{1, 2, 0, 1}, {-1, -2, 2, 0}, {2, 4, 1, 1}, {0, 0, -1, 3}, {1, 2, 1, -1}};
  const double y[5] = {1.0, -2.0, 0.5, 3.0, -1.0};
  double G[16], g[4];
  for (int i = 0; i < 4; ++i) {
    g[i] = 0.0;
    for (int k = 0; k < 5; ++k) g[i] += X[k][i] * y[k];
    for (int j = 0; j < 4; ++j) {
      G[i * 4 + j] = 0.0;
      for (int k = 0; k < 5; ++k) G[i * 4 + j] += X[k][i] * X[k][j];
    }
  }
  const std::vector<int> gstart = {0, 2, 4};
  const double inf = HUGE_VAL;
  double beta[4];
  for (int polish = 0; polish < 2; ++polish) {
    // the first group alone: one column counts, the dependent one keeps a zero, the other group is all zero
    double v = l0_support(G, g, 4, gstart, 1ull, inf, polish != 0, beta);
    CHECK(fabs(beta[0] - g[0] / G[0]) <= 1e-15 && beta[1] == 0.0 && beta[2] == 0.0 && beta[3] == 0.0);
    CHECK(fabs(v + 0.5 * g[0] * g[0] / G[0]) <= 1e-14);
    // both groups: the solution on columns {0, 2, 3}, with the skipped column still at zero
    v = l0_support(G, g, 4, gstart, 3ull, inf, polish != 0, beta);
    const int cols[3] = {0, 2, 3};
    long double L[6][6], w[6], b[6], ss = 0.0L;
    l0_reference(G, g, 4, cols, 3, L, w, b);
    for (int k = 0; k < 3; ++k) ss += w[k] * w[k];
    CHECK(beta[1] == 0.0);
    for (int k = 0; k < 3; ++k) CHECK(l0_near(beta[cols[k]], b[k], 1e-13));
    CHECK(l0_near(v, -0.5L * ss, 1e-13));
    // ... also when the box binds on the kept columns
    double top = 0.0;
    for (int k = 0; k < 4; ++k) top = fmax(top, fabs(beta[k]));
    const double free_v = v;
    v = l0_support(G, g, 4, gstart, 3ull, 0.5 * top, polish != 0, beta);
    CHECK(beta[1] == 0.0 && v > free_v);
    for (int k = 0; k < 4; ++k) CHECK(fabs(beta[k]) <= 0.5 * top);
    // the empty support
    CHECK(l0_support(G, g, 4, gstart, 0ull, inf, polish != 0, beta) == 0.0);
    for (int k = 0; k < 4; ++k) CHECK(beta[k] == 0.0);
  }
}

int main() {
  test_pool();
  test_row_sets();
  test_interleaved();
  test_interleaved_sixteen_lanes();
  test_auto_lanes();
  test_grid();
  test_find_and_tiles();
  test_knobs();
  test_tail_snapshot();
  test_bb_decide();
  test_bb_stop();
  test_fista_decide();
  test_tail_route();
  test_l0_factor();
  test_l0_boxed();
  test_l0_support_skips_dependent_columns();
  if (failures) {
    fprintf(stderr, "host_logic_test: %d check(s) failed\n", failures);
    return 1;
  }
  printf("host_logic_test: ok\n");
  return 0;
}
