// The CPU baseline of `tools/l1l0_local_timing.py`: l0_local_solve<false, true> of csrc/l0_host.hpp -- the twin of l0_local_l1_kernel --
// on the cells of one file, one after the other on one core.  The tool compiles this file with g++ -O2 and runs it.
// In: a file of  int64 p, ld, n_cells, swaps;  double yy, big_M;  G [p][ld];  c [p];  alphas [n_cells];  l1s [n_cells];  ridges [n_cells].
// Out: one line "cells N ms T changes C sweeps S swaps W", then one line "F" with every cell's objective.
#include <stdint.h>
#include <stdio.h>

#include <chrono>
#include <vector>

#include "../sparse-lm_amd/csrc/l0_host.hpp"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  int64_t head[4];
  double scal[2];
  if (fread(head, sizeof(int64_t), 4, fh) != 4 || fread(scal, sizeof(double), 2, fh) != 2) return 2;
  const int p = (int)head[0], cells = (int)head[2];
  const size_t ld = (size_t)head[1];
  if (p < 1 || p > slm::L0_LS_PMAX || ld < (size_t)p || cells < 1) return 2;
  std::vector<double> G((size_t)p * ld), c((size_t)p), alphas((size_t)cells), l1s((size_t)cells), ridges((size_t)cells), beta((size_t)p),
      F((size_t)cells);
  auto take = [&](std::vector<double>& v) { return fread(v.data(), sizeof(double), v.size(), fh) == v.size(); };
  if (!take(G) || !take(c) || !take(alphas) || !take(l1s) || !take(ridges)) return 2;
  fclose(fh);
  long long changes = 0, sweeps = 0, swaps = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (int e = 0; e < cells; ++e) {
    const slm::L0LsResult R = slm::l0_local_solve<false, true>(G.data(), ld, c.data(), p, alphas[(size_t)e], ridges[(size_t)e], scal[1], scal[0],
                                                               head[3] != 0, nullptr, beta.data(), l1s[(size_t)e]);
    F[(size_t)e] = R.F;
    changes += R.changes;
    sweeps += R.sweeps;
    swaps += R.swaps;
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("cells %d ms %.6f changes %lld sweeps %lld swaps %lld\nF", cells, ms, changes, sweeps, swaps);
  for (double v : F) printf(" %.17g", v);
  printf("\n");
  return 0;
}
