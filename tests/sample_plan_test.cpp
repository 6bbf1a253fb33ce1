// slm_host::sample_plan (csrc/host_logic.hpp): the grid of the opening's sample product on the fp32 image, walked block by
// block the way sample_xty_kernel walks it.  For every shape of tests/test_sample_f32_gpu.py at every divisor, the headline's
// quarter (25 000 x 5 000) and the wide shape (12 500 x 20 000), on 256 and 304 CUs: every (row, column) of the image is
// covered exactly once, no block is empty, every row of every block starts on 16 bytes.  Built with
// -fsanitize=address,undefined by tests/test_sample_plan_cpu.py.
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../sparse-lm_amd/csrc/host_logic.hpp"

static int failures = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      ++failures;                                 \
      printf("FAILED %s: ", #cond);               \
      printf(__VA_ARGS__);                        \
      printf("\n");                               \
    }                                             \
  } while (0)

static void check_shape(int64_t n_s, int64_t p, int cus) {
  using namespace slm_host;
  const int64_t ld32 = sample_ld32(p);
  CHECK(ld32 % 4 == 0 && ld32 >= p && ld32 < p + 4, "ld32 %lld for p %lld", (long long)ld32, (long long)p);
  const SamplePlan g = sample_plan(n_s, p, ld32, cus);
  CHECK(g.xb >= 1 && g.yb >= 1 && g.rows >= 1 && g.ld32 == ld32, "plan of (%lld, %lld, %d)", (long long)n_s, (long long)p, cus);
  // as many row blocks as fill the CUs, unless the rows give fewer
  CHECK((int64_t)g.xb * g.yb <= (int64_t)kSampleWgsPerCu * cus || g.yb == 1, "grid %d x %d on %d CUs", g.xb, g.yb, cus);
  std::vector<uint8_t> seen((size_t)(n_s * ld32), 0);
  for (int by = 0; by < g.yb; ++by) {
    const int64_t i0 = (int64_t)by * g.rows, i1 = i0 + g.rows < n_s ? i0 + g.rows : n_s;
    CHECK(i0 < i1, "row block %d of (%lld, %lld, %d) is empty", by, (long long)n_s, (long long)p, cus);
    for (int bx = 0; bx < g.xb; ++bx) {
      int64_t covered = 0;
      for (int t = 0; t < kSampleThreads; ++t) {
        const int64_t col = ((int64_t)bx * kSampleThreads + t) * 4;
        if (col >= ld32) continue;
        CHECK(col + 4 <= ld32, "thread %d of column block %d reads past the row", t, bx);
        for (int64_t i = i0; i < i1; ++i) {
          const int64_t byte = (i * ld32 + col) * (int64_t)sizeof(float);
          if (byte % 16 != 0) CHECK(false, "row %lld column %lld starts at byte %lld", (long long)i, (long long)col, (long long)byte);
          for (int c = 0; c < 4; ++c) ++seen[(size_t)(i * ld32 + col + c)];
        }
        covered += 4;
      }
      CHECK(covered > 0, "column block %d of (%lld, %lld, %d) is empty", bx, (long long)n_s, (long long)p, cus);
    }
  }
  int64_t wrong = 0;
  for (uint8_t v : seen) wrong += v != 1;
  CHECK(wrong == 0, "%lld entries of (%lld, %lld, %d) not covered exactly once", (long long)wrong, (long long)n_s, (long long)p, cus);
}

int main() {
  const int64_t shapes[][2] = {{256, 1}, {400, 3}, {1000, 7}, {4099, 130}, {10000, 513}, {6000, 4097}};
  const int divs[] = {1, 4, 64};
  const int cus[] = {256, 304};
  for (int c : cus) {
    for (const auto& s : shapes)
      for (int d : divs) check_shape(s[0] / d, s[1], c);
    check_shape(25000, 5000, c);
    check_shape(12500, 20000, c);
    check_shape(1, 1, c);
  }
  // the headline: about four workgroups per CU, all resident at once
  const slm_host::SamplePlan h = slm_host::sample_plan(25000, 5000, 5000, 256);
  CHECK(h.xb == 5 && h.yb * h.xb > 3 * 256 && h.yb * h.xb <= 4 * 256, "headline grid %d x %d", h.xb, h.yb);
  // 20 000 columns: no tile quantisation worth the name (the grid is within 2 % of four workgroups per CU)
  const slm_host::SamplePlan w = slm_host::sample_plan(12500, 20000, 20000, 256);
  CHECK(w.xb == 20 && w.yb * w.xb >= 1000 && w.yb * w.xb <= 1024, "wide grid %d x %d", w.xb, w.yb);
  // the knob of the fp64 route
  const char* on = "1";
  slm_host::Knobs k = slm_host::Knobs::from([&](const char* name) -> const char* { return std::string(name) == "SLM_SAMPLE_F64" ? on : nullptr; });
  CHECK(k.sample_f64, "SLM_SAMPLE_F64=1");
  k = slm_host::Knobs::from([](const char*) -> const char* { return nullptr; });
  CHECK(!k.sample_f64, "default");
  if (failures) {
    printf("sample_plan_test: %d failures\n", failures);
    return 1;
  }
  printf("sample_plan_test: ok\n");
  return 0;
}
