// The CPU baseline of `tools/l0_local_group_prove_timing.py`: l0_prove_tree of csrc/l0_host.hpp with a group map and the group node
// twin l0_group_node_solve as its callable -- the tree slm_solve_l0_local_group_prove grows, node for node -- on one core.  The
// tool compiles this file with g++ -O2 -ffp-contract=off and runs it.
// In: a file of  int64 p, n_cells, max_nodes, width, max_sweeps, has_incumbents, n_groups, n_need;  double big_M, rel_gap;
//     int64 gstart [n_groups + 1], need_ptr [n_groups + 1], need_idx [n_need];  G [p][p];  c [p];  alphas [n_cells];  etas [n_cells];
//     incumbents [n_cells][p] where has_incumbents.
// Out: one line "cells N ms T nodes K launches L most M optimal O".
#include <stdint.h>
#include <stdio.h>

#include <chrono>
#include <vector>

#include "../sparse-lm_amd/csrc/l0_host.hpp"

int main(int argc, char** argv) {
  using namespace slm;
  if (argc != 2) return 2;
  FILE* fh = fopen(argv[1], "rb");
  if (!fh) return 2;
  int64_t head[8];
  double scal[2];
  if (fread(head, sizeof(int64_t), 8, fh) != 8 || fread(scal, sizeof(double), 2, fh) != 2) return 2;
  const int p = (int)head[0], cells = (int)head[1], max_nodes = (int)head[2], width = (int)head[3], max_sweeps = (int)head[4], ng = (int)head[6];
  if (p < 1 || p > L0_LS_PMAX || cells < 1 || max_nodes < 1 || width < 1 || max_sweeps < 1 || ng < 1 || ng > p || head[7] < 0 || !(scal[0] > 0.0))
    return 2;
  std::vector<int64_t> wide((size_t)(2 * (ng + 1) + head[7]));
  if (fread(wide.data(), sizeof(int64_t), wide.size(), fh) != wide.size()) return 2;
  std::vector<int> gstart(wide.begin(), wide.begin() + ng + 1), need_ptr(wide.begin() + ng + 1, wide.begin() + 2 * (ng + 1)),
      need_idx(wide.begin() + 2 * (ng + 1), wide.end());
  if (gstart[0] != 0 || gstart[(size_t)ng] != p || need_ptr[0] != 0 || need_ptr[(size_t)ng] != (int)head[7]) return 2;
  for (int g = 0; g < ng; ++g)
    if (gstart[(size_t)g + 1] <= gstart[(size_t)g] || need_ptr[(size_t)g + 1] < need_ptr[(size_t)g]) return 2;
  for (int v : need_idx)
    if (v < 0 || v >= ng) return 2;
  std::vector<double> G((size_t)p * p), c((size_t)p), alphas((size_t)cells), etas((size_t)cells), inc(head[5] ? (size_t)cells * p : 0);
  auto take = [&](std::vector<double>& v) { return fread(v.data(), sizeof(double), v.size(), fh) == v.size(); };
  if (!take(G) || !take(c) || !take(alphas) || !take(etas) || !take(inc)) return 2;
  fclose(fh);
  std::vector<int> cptr, cidx, rptr, ridx;
  l0_lg_close(ng, need_ptr.data(), need_idx.data(), cptr, cidx);
  l0_gp_reverse(ng, cptr, cidx, rptr, ridx);
  L0GroupMap gm;
  gm.ng = ng; gm.gstart = gstart.data(); gm.cptr = cptr.data(); gm.cidx = cidx.data(); gm.rptr = rptr.data(); gm.ridx = ridx.data();
  std::vector<L0NodeCell> nc((size_t)cells);
  for (int e = 0; e < cells; ++e) nc[(size_t)e] = l0_node_cell(alphas[(size_t)e], etas[(size_t)e], scal[0]);
  std::vector<double> beta((size_t)cells * p), F((size_t)cells), L((size_t)cells);
  std::vector<int> nodes((size_t)cells), rounds((size_t)cells), status((size_t)cells);
  long long launches = 0, most = 0, total = 0, optimal = 0;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = l0_prove_tree(G.data(), (size_t)p, c.data(), p, cells, nc.data(), head[5] ? inc.data() : nullptr, scal[1], max_nodes, width,
                               [&](const L0NodeBatch& b) {
                                 ++launches;
                                 most = b.n > most ? b.n : most;
                                 return l0_group_node_batch_host(G.data(), (size_t)p, c.data(), p, nc.data(), gm, max_sweeps, scal[1] / 100.0, b);
                               },
                               beta.data(), F.data(), L.data(), nodes.data(), rounds.data(), status.data(), nullptr, &gm);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (rc != 0) return 3;
  for (int e = 0; e < cells; ++e) {
    total += nodes[(size_t)e];
    optimal += status[(size_t)e] == L0_PV_OPTIMAL;
  }
  printf("cells %d ms %.6f nodes %lld launches %lld most %lld optimal %lld\n", cells, ms, total, launches, most, optimal);
  return 0;
}
