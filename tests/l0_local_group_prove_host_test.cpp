// The local proof with groups without a device (csrc/l0_host.hpp, "local proof with groups"): the group node twin
// l0_group_node_solve, the tree l0_prove_tree with a group map and the twin as its callable, and the argument checks -- meant to
// run under AddressSanitizer and UndefinedBehaviorSanitizer as a plain program.  Its input is a file of doubles that
// tests/test_l0_local_group_prove_cpu.py writes: node batches with the numpy restatement's answers, which the twin must meet BIT
// FOR BIT (and, where every group is one column and there is no hierarchy, l0_node_solve's bits), and trees with the
// restatement's nodes, rounds, coefficients and bounds, which the twin's tree must meet exactly.
//   g++ -std=c++17 -O1 -g -ffp-contract=off [-fsanitize=address,undefined] tests/l0_local_group_prove_host_test.cpp -o t && ./t cases.bin
#include "../sparse-lm_amd/csrc/l0_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace slm;

static int failures = 0;
#define CHECK(cond)                                               \
  do {                                                            \
    if (!(cond)) {                                                \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static bool same(double a, double b) { return memcmp(&a, &b, sizeof(a)) == 0; }  // the same bits: -0.0 is not +0.0

struct Reader {
  std::vector<double> v;
  size_t at = 0;
  double next() {
    if (at >= v.size()) {
      printf("FAILED: the case file ends early\n");
      exit(2);
    }
    return v[at++];
  }
  int next_int() { return (int)next(); }
  std::vector<double> block(size_t n) {
    std::vector<double> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = next();
    return out;
  }
  std::vector<int> ints(size_t n) {
    std::vector<int> out(n);
    for (size_t i = 0; i < n; ++i) out[i] = next_int();
    return out;
  }
};

static void words_of(const std::vector<double>& flags, unsigned long long* w) {
  for (int k = 0; k < L0_ND_WORDS; ++k) w[k] = 0;
  for (size_t j = 0; j < flags.size(); ++j)
    if (flags[j] != 0.0) w[j >> 6] |= 1ull << (j & 63);
}

// the groups of a case: ng, gstart, the direct need lists (CSR), and the map built from them
struct Groups {
  int ng = 0;
  std::vector<int> gstart, need_ptr, need_idx, cptr, cidx, rptr, ridx;
  L0GroupMap map;
  void read(Reader& in) {
    ng = in.next_int();
    gstart = in.ints((size_t)ng + 1);
    need_ptr = in.ints((size_t)ng + 1);
    need_idx = in.ints((size_t)need_ptr[(size_t)ng]);
    l0_lg_close(ng, need_ptr.data(), need_idx.data(), cptr, cidx);
    l0_gp_reverse(ng, cptr, cidx, rptr, ridx);
    map.ng = ng;
    map.gstart = gstart.data();
    map.cptr = cptr.data();
    map.cidx = cidx.data();
    map.rptr = rptr.data();
    map.ridx = ridx.data();
  }
  bool plain() const { return need_ptr[(size_t)ng] == 0 && gstart[(size_t)ng] == ng; }  // one column a group, no hierarchy
};

static int node_cases(Reader& in) {
  const int n_cases = in.next_int();
  int nodes_seen = 0;
  for (int k = 0; k < n_cases; ++k) {
    const int p = in.next_int(), n_cells = in.next_int();
    const double big_M = in.next();
    const int max_sweeps = in.next_int();
    const double gap_tol = in.next();
    const int n_nodes = in.next_int();
    Groups gr;
    gr.read(in);
    const std::vector<double> G = in.block((size_t)p * p), c = in.block((size_t)p), cells = in.block(2 * (size_t)n_cells);
    for (int i = 0; i < n_nodes; ++i) {
      const int cell = in.next_int(), has_start = in.next_int();
      const double parent = in.next();
      const std::vector<double> fin = in.block((size_t)gr.ng), fout = in.block((size_t)gr.ng);
      std::vector<double> start;
      if (has_start) start = in.block((size_t)p);
      const int sweeps = in.next_int(), status = in.next_int();
      const double lower = in.next(), primal = in.next(), upper = in.next();
      const std::vector<double> u_ref = in.block((size_t)p);
      unsigned long long wi[L0_ND_WORDS], wo[L0_ND_WORDS];
      words_of(fin, wi);
      words_of(fout, wo);
      const L0NodeCell nc = l0_node_cell(cells[2 * (size_t)cell], cells[2 * (size_t)cell + 1], big_M);
      std::vector<double> u((size_t)p);
      const L0NodeResult r = l0_group_node_solve(G.data(), (size_t)p, c.data(), p, nc, gr.map, wi, wo, has_start ? start.data() : nullptr,
                                                 max_sweeps, gap_tol, u.data());
      const double low = r.lower > parent ? r.lower : parent;
      bool ok = r.sweeps == sweeps && r.status == status && same(low, lower) && same(r.primal, primal) && same(r.upper, upper);
      for (int j = 0; j < p; ++j) ok = ok && same(u[(size_t)j], u_ref[(size_t)j]);
      if (!ok)
        printf("case %d node %d: sweeps %d/%d status %d/%d lower %.17g/%.17g primal %.17g/%.17g upper %.17g/%.17g\n", k, i, r.sweeps, sweeps,
               r.status, status, low, lower, r.primal, primal, r.upper, upper);
      CHECK(ok);
      if (gr.plain()) {  // singleton groups, no hierarchy: the column twin's bits
        std::vector<double> uc((size_t)p);
        const L0NodeResult q = l0_node_solve(G.data(), (size_t)p, c.data(), p, nc, wi, wo, has_start ? start.data() : nullptr, max_sweeps, gap_tol,
                                             uc.data());
        bool eq = q.sweeps == r.sweeps && q.status == r.status && same(q.lower, r.lower) && same(q.primal, r.primal) && same(q.upper, r.upper) &&
                  q.changes == r.changes;
        for (int j = 0; j < p; ++j) eq = eq && same(uc[(size_t)j], u[(size_t)j]);
        CHECK(eq);
      }
      {  // the batch wrapper is the same node
        const int cells_i[1] = {0};
        double bl, bp, bu;
        int bs[2];
        std::vector<double> u2((size_t)p);
        const L0NodeBatch b{1, cells_i, wi, wo, &parent, has_start ? start.data() : nullptr, &bl, &bp, &bu, u2.data(), bs};
        CHECK(l0_group_node_batch_host(G.data(), (size_t)p, c.data(), p, &nc, gr.map, max_sweeps, gap_tol, b) == 0);
        CHECK(same(bl, low) && same(bp, r.primal) && same(bu, r.upper) && bs[0] == r.sweeps && bs[1] == r.status);
      }
      ++nodes_seen;
    }
  }
  return nodes_seen;
}

static int tree_cases(Reader& in) {
  const int n_trees = in.next_int();
  int cells_seen = 0;
  for (int k = 0; k < n_trees; ++k) {
    const int p = in.next_int(), n_cells = in.next_int();
    const double big_M = in.next(), rel_gap = in.next();
    const int max_nodes = in.next_int(), width = in.next_int(), max_sweeps = in.next_int(), has_inc = in.next_int();
    Groups gr;
    gr.read(in);
    const std::vector<double> G = in.block((size_t)p * p), c = in.block((size_t)p), cells = in.block(2 * (size_t)n_cells);
    std::vector<double> inc;
    if (has_inc) inc = in.block((size_t)n_cells * p);
    std::vector<L0NodeCell> nc((size_t)n_cells);
    for (int e = 0; e < n_cells; ++e) nc[(size_t)e] = l0_node_cell(cells[2 * (size_t)e], cells[2 * (size_t)e + 1], big_M);
    std::vector<double> beta((size_t)n_cells * p), obj((size_t)n_cells), low((size_t)n_cells);
    std::vector<int> nodes((size_t)n_cells), rounds((size_t)n_cells), status((size_t)n_cells);
    const long long cap = 1 << 14;
    std::vector<int> lcell((size_t)cap);
    std::vector<unsigned long long> lin((size_t)cap * L0_ND_WORDS), lout((size_t)cap * L0_ND_WORDS);
    std::vector<double> lu((size_t)cap * p), llow((size_t)cap);
    L0ProveLeaves leaves;
    leaves.capacity = cap;
    leaves.cell = lcell.data(); leaves.in_mask = lin.data(); leaves.out_mask = lout.data(); leaves.u = lu.data(); leaves.lower = llow.data();
    long long most = 0;
    const int rc = l0_prove_tree(G.data(), (size_t)p, c.data(), p, n_cells, nc.data(), has_inc ? inc.data() : nullptr, rel_gap, max_nodes, width,
                                 [&](const L0NodeBatch& b) {
                                   most = b.n > most ? b.n : most;
                                   return l0_group_node_batch_host(G.data(), (size_t)p, c.data(), p, nc.data(), gr.map, max_sweeps, rel_gap / 100.0, b);
                                 },
                                 beta.data(), obj.data(), low.data(), nodes.data(), rounds.data(), status.data(), &leaves, &gr.map);
    CHECK(rc == 0 && most <= L0_ND_MAX_BATCH);
    std::vector<long long> cell_leaves((size_t)n_cells, 0);
    for (long long i = 0; i < std::min(leaves.count, cap); ++i) ++cell_leaves[(size_t)lcell[(size_t)i]];
    for (int e = 0; e < n_cells; ++e) {
      const int r_nodes = in.next_int(), r_rounds = in.next_int(), r_status = in.next_int();
      const double r_obj = in.next(), r_low = in.next();
      const int r_leaves = in.next_int();
      const std::vector<double> r_beta = in.block((size_t)p);
      bool ok = nodes[(size_t)e] == r_nodes && rounds[(size_t)e] == r_rounds && status[(size_t)e] == r_status && same(obj[(size_t)e], r_obj) &&
                same(low[(size_t)e], r_low) && cell_leaves[(size_t)e] == r_leaves;
      for (int j = 0; j < p; ++j) ok = ok && same(beta[(size_t)e * p + j], r_beta[(size_t)j]);
      if (!ok)
        printf("tree %d cell %d: nodes %d/%d rounds %d/%d status %d/%d objective %.17g/%.17g bound %.17g/%.17g leaves %lld/%d\n", k, e,
               nodes[(size_t)e], r_nodes, rounds[(size_t)e], r_rounds, status[(size_t)e], r_status, obj[(size_t)e], r_obj, low[(size_t)e], r_low,
               cell_leaves[(size_t)e], r_leaves);
      CHECK(ok);
      CHECK(low[(size_t)e] <= obj[(size_t)e]);
      ++cells_seen;
    }
  }
  return cells_seen;
}

static void test_checks() {
  const double al[2] = {0.1, 0.2}, et[2] = {0.0, 1.0};
  const int cell[2] = {0, 1};
  unsigned long long in[2 * L0_ND_WORDS] = {0}, out[2 * L0_ND_WORDS] = {0};
  const int gid[6] = {0, 0, 1, 1, 2, 2};           // three groups of two
  const int ptr[4] = {0, 0, 1, 2}, idx[2] = {0, 1};  // a chain: 1 needs 0, 2 needs 1
  int ng = -1;
  CHECK(l0_group_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 6, 1e-9, gid, ptr, idx, false, &ng).kind == L0_GP_OK && ng == 3);
  CHECK(l0_group_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 6, 1e-9, nullptr, nullptr, nullptr, false, &ng).kind == L0_GP_OK &&
        ng == 6);
  L0GpRefusal R = l0_group_nodes_check(2, al, et, -1.0, 2, cell, in, out, nullptr, nullptr, 6, 1e-9, gid, ptr, idx, false);
  CHECK(R.kind == L0_GP_FIRST && R.nd == L0_ND_BIG_M);
  const int torn[6] = {0, 1, 0, 1, 2, 2};
  R = l0_group_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 6, 1e-9, torn, ptr, idx, false);
  CHECK(R.kind == L0_GP_ORDER && R.which == 2);
  const int falls[4] = {0, 1, 0, 2};
  R = l0_group_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 6, 1e-9, gid, falls, idx, false);
  CHECK(R.kind == L0_GP_NEED_PTR && R.which == 2);
  const int far[2] = {0, 3};
  R = l0_group_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 6, 1e-9, gid, ptr, far, false);
  CHECK(R.kind == L0_GP_NEED_IDX && R.which == 1);
  R = l0_group_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 6, 1e-9, gid, ptr, nullptr, false);
  CHECK(R.kind == L0_GP_NEED_IDX);
  in[L0_ND_WORDS] = 8;  // node 1: group 3 of three
  R = l0_group_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 6, 1e-9, gid, ptr, idx, false);
  CHECK(R.kind == L0_GP_RANGE && R.which == 1);
  in[L0_ND_WORDS] = 4;  // node 1: group 2 IN without 1 and 0
  R = l0_group_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 6, 1e-9, gid, ptr, idx, false);
  CHECK(R.kind == L0_GP_UNCLOSED && R.which == 1);
  in[L0_ND_WORDS] = 7;
  CHECK(l0_group_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 6, 1e-9, gid, ptr, idx, false).kind == L0_GP_OK);
  in[L0_ND_WORDS] = 0;
  out[0] = 1;  // node 0: group 0 OUT while 1 and 2, which need it, are not
  R = l0_group_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 6, 1e-9, gid, ptr, idx, false);
  CHECK(R.kind == L0_GP_UNCLOSED && R.which == 0);
  out[0] = 7;
  CHECK(l0_group_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 6, 1e-9, gid, ptr, idx, false).kind == L0_GP_OK);
  CHECK(l0_group_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 6, 1e-9, gid, ptr, idx, true).kind == L0_GP_SHARDED);
  out[0] = 1;  // (without a hierarchy any masks are closed)
  CHECK(l0_group_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 6, 1e-9, gid, nullptr, nullptr, false).kind == L0_GP_OK);

  CHECK(l0_group_prove_check(2, al, et, 1.0, nullptr, 6, 1e-6, 100, 4, gid, ptr, idx, false, &ng).kind == L0_GP_OK && ng == 3);
  R = l0_group_prove_check(2, al, et, 1.0, nullptr, 6, 2.0, 100, 4, gid, ptr, idx, false);
  CHECK(R.kind == L0_GP_FIRST && R.pv == L0_PV_REL_GAP);
  CHECK(l0_group_prove_check(2, al, et, 1.0, nullptr, 6, 1e-6, 100, 4, torn, ptr, idx, false).kind == L0_GP_ORDER);
  CHECK(l0_group_prove_check(2, al, et, 1.0, nullptr, 6, 1e-6, 100, 4, gid, falls, idx, false).kind == L0_GP_NEED_PTR);
  CHECK(l0_group_prove_check(2, al, et, 1.0, nullptr, 6, 1e-6, 100, 4, gid, ptr, far, false).kind == L0_GP_NEED_IDX);
  CHECK(l0_group_prove_check(2, al, et, 1.0, nullptr, 6, 1e-6, 100, 4, gid, ptr, idx, true).kind == L0_GP_SHARDED);

  // the reverse of the closed lists, and a cycle
  std::vector<int> cptr, cidx, rptr, ridx;
  const int cyc_ptr[4] = {0, 1, 2, 2}, cyc_idx[2] = {1, 0};  // 0 and 1 need each other
  l0_lg_close(3, cyc_ptr, cyc_idx, cptr, cidx);
  l0_gp_reverse(3, cptr, cidx, rptr, ridx);
  CHECK(rptr == std::vector<int>({0, 1, 2, 2}) && ridx == std::vector<int>({1, 0}));
  L0GroupMap gm;
  const int gs[4] = {0, 2, 4, 6};
  gm.ng = 3; gm.gstart = gs; gm.cptr = cptr.data(); gm.cidx = cidx.data(); gm.rptr = rptr.data(); gm.ridx = ridx.data();
  unsigned long long m[L0_ND_WORDS] = {0};
  l0_gp_child(gm, 0, true, m);
  CHECK(m[0] == 3);
  m[0] = 0;
  l0_gp_child(gm, 1, false, m);
  CHECK(m[0] == 3);
}

int main(int argc, char** argv) {
  test_checks();
  if (argc > 1) {
    FILE* fh = fopen(argv[1], "rb");
    if (!fh) {
      printf("FAILED: cannot open %s\n", argv[1]);
      return 2;
    }
    Reader in;
    fseek(fh, 0, SEEK_END);
    const long bytes = ftell(fh);
    fseek(fh, 0, SEEK_SET);
    in.v.resize((size_t)bytes / sizeof(double));
    const size_t got = fread(in.v.data(), sizeof(double), in.v.size(), fh);
    fclose(fh);
    CHECK(got == in.v.size());
    const int nodes = node_cases(in);
    const int cells = tree_cases(in);
    CHECK(in.at == in.v.size());
    printf("exported: %d nodes, %d tree cells\n", nodes, cells);
  }
  if (failures) {
    printf("l0_local_group_prove_host_test: %d FAILED\n", failures);
    return 1;
  }
  printf("l0_local_group_prove_host_test: ok\n");
  return 0;
}
