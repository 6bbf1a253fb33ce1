// The CPU baseline of `tools/l0_local_bound_timing.py`: l0_bound_solve of csrc/l0_host.hpp -- the twin of l0_local_bound_kernel -- on the
// cells of one file, one after the other on one core.  The tool compiles this file with g++ -O2 -ffp-contract=off and runs it.
// In: a file of  int64 p, ld, n_cells, max_sweeps;  double big_M, gap_tol;  G [p][ld];  c [p];  alphas [n_cells];  etas [n_cells].
// Out: one line "cells N ms T changes C sweeps S open O", then one line "L" with every cell's bound.
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
  const int p = (int)head[0], cells = (int)head[2], max_sweeps = (int)head[3];
  const size_t ld = (size_t)head[1];
  if (p < 1 || p > slm::L0_LS_PMAX || ld < (size_t)p || cells < 1 || max_sweeps < 1 || !(scal[0] > 0.0)) return 2;
  std::vector<double> G((size_t)p * ld), c((size_t)p), alphas((size_t)cells), etas((size_t)cells), u((size_t)p), L((size_t)cells);
  auto take = [&](std::vector<double>& v) { return fread(v.data(), sizeof(double), v.size(), fh) == v.size(); };
  if (!take(G) || !take(c) || !take(alphas) || !take(etas)) return 2;
  fclose(fh);
  long long changes = 0, sweeps = 0, open = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (int e = 0; e < cells; ++e) {
    const slm::L0LbResult R = slm::l0_bound_solve(G.data(), ld, c.data(), p, alphas[(size_t)e], etas[(size_t)e], scal[0], nullptr, max_sweeps,
                                                  scal[1], u.data());
    L[(size_t)e] = R.lower;
    changes += R.changes;
    sweeps += R.sweeps;
    open += R.status != 0;
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("cells %d ms %.6f changes %lld sweeps %lld open %lld\nL", cells, ms, changes, sweeps, open);
  for (double v : L) printf(" %.17g", v);
  printf("\n");
  return 0;
}
