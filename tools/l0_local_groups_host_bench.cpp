// The CPU baseline of `tools/l0_local_groups_timing.py`: l0_lg_solve of csrc/l0_host.hpp -- the twin of l0_local_group_kernel -- on
// the cells of one file, one after the other on one core.  The tool compiles this file with g++ -O2 and runs it.
// In: a file of  int64 p, ld, n_cells, swaps, ng, n_need;  double yy, big_M;  G [p][ld];  c [p];  alphas [n_cells];  etas [n_cells];
//     then as doubles: gstart [ng + 1], need_ptr [ng + 1], need_idx [n_need] (the DIRECT lists: closed here, outside the clock).
// Out: one line "cells N ms T changes C sweeps S swaps W trials R", then one line "F" with every cell's objective.
#include <stdint.h>
#include <stdio.h>

#include <chrono>
#include <vector>

#include "../sparse-lm_amd/csrc/l0_host.hpp"

static std::vector<int> ints(const std::vector<double>& v) { return std::vector<int>(v.begin(), v.end()); }

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  int64_t head[6];
  double scal[2];
  if (fread(head, sizeof(int64_t), 6, fh) != 6 || fread(scal, sizeof(double), 2, fh) != 2) return 2;
  const int p = (int)head[0], cells = (int)head[2], ng = (int)head[4], n_need = (int)head[5];
  const size_t ld = (size_t)head[1];
  if (p < 1 || p > slm::L0_LS_PMAX || ld < (size_t)p || cells < 1 || ng < 1 || ng > p || n_need < 0) return 2;
  std::vector<double> G((size_t)p * ld), c((size_t)p), alphas((size_t)cells), etas((size_t)cells), beta((size_t)p), F((size_t)cells);
  std::vector<double> gs((size_t)ng + 1), np((size_t)ng + 1), ni((size_t)n_need);
  auto take = [&](std::vector<double>& v) { return fread(v.data(), sizeof(double), v.size(), fh) == v.size(); };
  if (!take(G) || !take(c) || !take(alphas) || !take(etas) || !take(gs) || !take(np) || !take(ni)) return 2;
  fclose(fh);
  const std::vector<int> gstart = ints(gs), need_ptr = ints(np), need_idx = ints(ni);
  for (int k = 0; k < n_need; ++k)
    if (need_idx[(size_t)k] < 0 || need_idx[(size_t)k] >= ng) return 2;
  std::vector<int> cptr, cidx;
  slm::l0_lg_close(ng, need_ptr.data(), need_idx.data(), cptr, cidx);
  cidx.push_back(0);
  long long changes = 0, sweeps = 0, swaps = 0, trials = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (int e = 0; e < cells; ++e) {
    const slm::L0LgResult R = slm::l0_lg_solve(G.data(), ld, c.data(), p, ng, gstart.data(), cptr.data(), cidx.data(), alphas[(size_t)e],
                                               etas[(size_t)e], scal[1], scal[0], head[3] != 0, nullptr, beta.data());
    F[(size_t)e] = R.F;
    changes += R.changes;
    sweeps += R.sweeps;
    swaps += R.swaps;
    trials += R.trials;
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  printf("cells %d ms %.6f changes %lld sweeps %lld swaps %lld trials %lld\nF", cells, ms, changes, sweeps, swaps, trials);
  for (double v : F) printf(" %.17g", v);
  printf("\n");
  return 0;
}
