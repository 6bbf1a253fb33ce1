// The CPU baseline of `tools/l0_local_prove_timing.py`: l0_prove_tree of csrc/l0_host.hpp with the node twin l0_node_solve as its
// callable -- the tree slm_solve_l0_local_prove grows, node for node -- on one core.  The tool compiles this file with
// g++ -O2 -ffp-contract=off and runs it.
// In: a file of  int64 p, ld, n_cells, max_nodes, width, max_sweeps, has_incumbents;  double big_M, rel_gap;  G [p][ld];  c [p];
//     alphas [n_cells];  etas [n_cells];  incumbents [n_cells][p] where has_incumbents.
// Out: one line "cells N ms T nodes K launches L most M optimal O", then "F", "L", "nodes" and "rounds" with every cell's value.
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
  int64_t head[7];
  double scal[2];
  if (fread(head, sizeof(int64_t), 7, fh) != 7 || fread(scal, sizeof(double), 2, fh) != 2) return 2;
  const int p = (int)head[0], cells = (int)head[2], max_nodes = (int)head[3], width = (int)head[4], max_sweeps = (int)head[5];
  const size_t ld = (size_t)head[1];
  if (p < 1 || p > L0_LS_PMAX || ld < (size_t)p || cells < 1 || max_nodes < 1 || width < 1 || max_sweeps < 1 || !(scal[0] > 0.0)) return 2;
  std::vector<double> G((size_t)p * ld), c((size_t)p), alphas((size_t)cells), etas((size_t)cells), inc(head[6] ? (size_t)cells * p : 0);
  auto take = [&](std::vector<double>& v) { return fread(v.data(), sizeof(double), v.size(), fh) == v.size(); };
  if (!take(G) || !take(c) || !take(alphas) || !take(etas) || !take(inc)) return 2;
  fclose(fh);
  std::vector<L0NodeCell> nc((size_t)cells);
  for (int e = 0; e < cells; ++e) nc[(size_t)e] = l0_node_cell(alphas[(size_t)e], etas[(size_t)e], scal[0]);
  std::vector<double> beta((size_t)cells * p), F((size_t)cells), L((size_t)cells);
  std::vector<int> nodes((size_t)cells), rounds((size_t)cells), status((size_t)cells);
  long long launches = 0, most = 0, total = 0, optimal = 0;
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = l0_prove_tree(G.data(), ld, c.data(), p, cells, nc.data(), head[6] ? inc.data() : nullptr, scal[1], max_nodes, width,
                               [&](const L0NodeBatch& b) {
                                 ++launches;
                                 most = b.n > most ? b.n : most;
                                 return l0_node_batch_host(G.data(), ld, c.data(), p, nc.data(), max_sweeps, scal[1] / 100.0, b);
                               },
                               beta.data(), F.data(), L.data(), nodes.data(), rounds.data(), status.data());
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (rc != 0) return 3;
  for (int e = 0; e < cells; ++e) {
    total += nodes[(size_t)e];
    optimal += status[(size_t)e] == L0_PV_OPTIMAL;
  }
  printf("cells %d ms %.6f nodes %lld launches %lld most %lld optimal %lld\nF", cells, ms, total, launches, most, optimal);
  for (double v : F) printf(" %.17g", v);
  printf("\nL");
  for (double v : L) printf(" %.17g", v);
  printf("\nnodes");
  for (int v : nodes) printf(" %d", v);
  printf("\nrounds");
  for (int v : rounds) printf(" %d", v);
  printf("\n");
  return 0;
}
