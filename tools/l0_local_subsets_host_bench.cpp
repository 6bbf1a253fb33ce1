// The CPU baseline of `tools/l0_local_subsets_timing.py`: l0_local_solve<true> of csrc/l0_host.hpp -- the twin of the kernel's cardinality
// rule -- on the cells of one file, one after the other on one core.  The tool compiles this file with g++ -O2 and runs it.
// In: a file of  int64 p, ld, n_cells, swaps;  double yy, big_M;  G [p][ld];  c [p];  sizes [n_cells] (as doubles);  etas [n_cells].
// Out: one line "cells N ms T changes C sweeps S swaps W grows G drops D", then one line "Q" with every cell's objective.
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
  std::vector<double> G((size_t)p * ld), c((size_t)p), sizes((size_t)cells), etas((size_t)cells), beta((size_t)p), Q((size_t)cells);
  if (fread(G.data(), sizeof(double), G.size(), fh) != G.size() || fread(c.data(), sizeof(double), c.size(), fh) != c.size() ||
      fread(sizes.data(), sizeof(double), sizes.size(), fh) != sizes.size() || fread(etas.data(), sizeof(double), etas.size(), fh) != etas.size())
    return 2;
  fclose(fh);
  long long changes = 0, sweeps = 0, swaps = 0, grows = 0, drops = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (int e = 0; e < cells; ++e) {
    const slm::L0LsResult R = slm::l0_local_solve<true>(G.data(), ld, c.data(), p, (int)sizes[(size_t)e], etas[(size_t)e], scal[1], scal[0], head[3] != 0,
                                               nullptr, beta.data());
    Q[(size_t)e] = R.F;
    changes += R.changes;
    sweeps += R.sweeps;
    swaps += R.swaps;
    grows += R.grows;
    drops += R.drops;
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("cells %d ms %.6f changes %lld sweeps %lld swaps %lld grows %lld drops %lld\nQ", cells, ms, changes, sweeps, swaps, grows, drops);
  for (double v : Q) printf(" %.17g", v);
  printf("\n");
  return 0;
}
