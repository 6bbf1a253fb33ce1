// slm_host::gather_row_blocks and slm_host::xty_part_rows (csrc/host_logic.hpp): the row blocks of the working set's gather
// and the rows of partial sums its X_W^T y variant writes, walked the way ws_gather_body walks them.  For the row counts of
// tests/test_opening_xty_gpu.py, the headline and the edges of the cap: every tile of 32 rows belongs to exactly one row
// block, no row block is empty (so every row of partials the apply reads has been written), the partials fit the buffer they
// go to -- written here into a buffer of exactly that size, which AddressSanitizer guards.  Built with
// -fsanitize=address,undefined by tests/test_gather_rows_cpu.py.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
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

// the Gram's partial block as engine_path.hip sizes it: most = max(1, min(cus, n / 64)) row blocks of 512 x 512 per row set
static int64_t part_doubles(int64_t n, int cus, int sets) {
  const int64_t most = std::max<int64_t>(1, std::min<int64_t>(cus, n / 64));
  return most * sets * 512 * 512;
}

static void walk(int64_t n, int blocks, int64_t buffer) {
  const int64_t tiles = (n + 31) / 32;
  CHECK(blocks >= 1 && blocks <= slm_host::kGatherRowBlocks && blocks <= tiles, "n %lld: %d row blocks for %lld tiles", (long long)n, blocks,
        (long long)tiles);
  std::vector<int> owner_count((size_t)tiles, 0);
  std::vector<double> part((size_t)buffer, 0.0);  // (exactly the buffer: a row of partials past it is a heap overflow)
  for (int b = 0; b < blocks; ++b) {
    int64_t walked = 0;
    for (int64_t rt = b; rt < tiles; rt += blocks) {
      ++owner_count[(size_t)rt];
      ++walked;
    }
    CHECK(walked > 0, "n %lld: row block %d of %d walks no tile", (long long)n, b, blocks);
    for (int k = 0; k < slm_host::kXtyPartStride; ++k) part[(size_t)b * slm_host::kXtyPartStride + k] += 1.0;
  }
  int64_t wrong = 0;
  for (int c : owner_count) wrong += c != 1;
  CHECK(wrong == 0, "n %lld: %lld tiles not walked exactly once", (long long)n, (long long)wrong);
}

int main() {
  using namespace slm_host;
  const int64_t rows[] = {1, 31, 32, 33, 95, 64, 127, 128, 4096, 32 * 1024 - 1, 32 * 1024, 32 * 1024 + 1, 33000, 100000, 4000000};
  const int cus[] = {1, 2, 3, 64, 256, 304};
  for (int64_t n : rows) {
    const int g = gather_row_blocks(n);
    CHECK(g == (int)std::min<int64_t>((n + 31) / 32, 1024), "gather_row_blocks(%lld) = %d", (long long)n, g);
    walk(n, g, (int64_t)g * kXtyPartStride);
    for (int c : cus)
      for (int sets : {1, 5}) {
        const int64_t buf = part_doubles(n, c, sets);
        const int r = xty_part_rows(n, buf);
        CHECK(r >= 1 && r <= g && (int64_t)r * kXtyPartStride <= buf, "xty_part_rows(%lld, %lld) = %d", (long long)n, (long long)buf, r);
        walk(n, r, buf);
        // from three row blocks of the Gram on, the buffer never cuts the grid: the gather with the sums is the plain one's
        if (buf >= 3 * 512 * 512) CHECK(r == g, "n %lld on %d CUs: %d row blocks, the plain gather has %d", (long long)n, c, r, g);
      }
  }
  CHECK(gather_row_blocks(0) == 1 && gather_row_blocks(-5) == 1, "an empty dataset still launches one row block");
  CHECK(xty_part_rows(100000, 0) == 1 && xty_part_rows(100000, kXtyPartStride * 7 + 1) == 7, "a short buffer cuts the rows");
  CHECK(xty_part_rows(100000, part_doubles(100000, 256, 1)) == 1024, "the headline: 1 024 rows of partials");
  if (failures) {
    printf("gather_rows_test: %d failures\n", failures);
    return 1;
  }
  printf("gather_rows_test: ok\n");
  return 0;
}
