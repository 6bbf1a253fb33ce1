// The local proof without a device (csrc/l0_host.hpp, "local proof"): the node twin l0_node_solve, the tree l0_prove_tree with
// the twin as its callable, and the argument checks l0_nodes_check and l0_prove_check -- meant to run under AddressSanitizer
// and UndefinedBehaviorSanitizer as a plain program.  Its input is a file of doubles that tests/test_l0_local_prove_cpu.py
// writes: node batches with the numpy restatement's answers, which the twin must meet BIT FOR BIT, and trees with the
// restatement's nodes, rounds, coefficients and bounds, which the twin's tree must meet exactly.
//   g++ -std=c++17 -O1 -g -ffp-contract=off [-fsanitize=address,undefined] tests/l0_local_prove_host_test.cpp -o t && ./t cases.bin
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
};

static void words_of(const std::vector<double>& flags, unsigned long long* w) {
  for (int k = 0; k < L0_ND_WORDS; ++k) w[k] = 0;
  for (size_t j = 0; j < flags.size(); ++j)
    if (flags[j] != 0.0) w[j >> 6] |= 1ull << (j & 63);
}

static int node_cases(Reader& in) {
  const int n_cases = in.next_int();
  int nodes_seen = 0;
  for (int k = 0; k < n_cases; ++k) {
    const int p = in.next_int(), n_cells = in.next_int();
    const double big_M = in.next();
    const int max_sweeps = in.next_int();
    const double gap_tol = in.next();
    const int n_nodes = in.next_int();
    const std::vector<double> G = in.block((size_t)p * p), c = in.block((size_t)p), cells = in.block(2 * (size_t)n_cells);
    for (int i = 0; i < n_nodes; ++i) {
      const int cell = in.next_int(), has_start = in.next_int();
      const double parent = in.next();
      const std::vector<double> fin = in.block((size_t)p), fout = in.block((size_t)p);
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
      const L0NodeResult r = l0_node_solve(G.data(), (size_t)p, c.data(), p, nc, wi, wo, has_start ? start.data() : nullptr, max_sweeps, gap_tol,
                                           u.data());
      const double low = r.lower > parent ? r.lower : parent;
      bool ok = r.sweeps == sweeps && r.status == status && same(low, lower) && same(r.primal, primal) && same(r.upper, upper);
      for (int j = 0; j < p; ++j) ok = ok && same(u[(size_t)j], u_ref[(size_t)j]);
      if (!ok)
        printf("case %d node %d: sweeps %d/%d status %d/%d lower %.17g/%.17g primal %.17g/%.17g upper %.17g/%.17g\n", k, i, r.sweeps, sweeps,
               r.status, status, low, lower, r.primal, primal, r.upper, upper);
      CHECK(ok);
      bool any = false;
      for (int w = 0; w < L0_ND_WORDS; ++w) any = any || wi[w] || wo[w];
      if (!any) {  // with both masks empty the twin returns l0_bound_solve's bits
        std::vector<double> ub((size_t)p);
        const L0LbResult b = l0_bound_solve(G.data(), (size_t)p, c.data(), p, nc.alpha, nc.eta, big_M, has_start ? start.data() : nullptr,
                                            max_sweeps, gap_tol, ub.data());
        bool eq = b.sweeps == r.sweeps && b.status == r.status && same(b.lower, r.lower) && same(b.primal, r.primal) && b.changes == r.changes;
        for (int j = 0; j < p; ++j) eq = eq && same(ub[(size_t)j], u[(size_t)j]);
        CHECK(eq);
      }
      // the batch wrapper is the same node
      {
        const int cells_i[1] = {0};
        double bl, bp, bu;
        int bs[2];
        std::vector<double> u2((size_t)p);
        const L0NodeBatch b{1, cells_i, wi, wo, &parent, has_start ? start.data() : nullptr, &bl, &bp, &bu, u2.data(), bs};
        CHECK(l0_node_batch_host(G.data(), (size_t)p, c.data(), p, &nc, max_sweeps, gap_tol, b) == 0);
        CHECK(same(bl, low) && same(bp, r.primal) && same(bu, r.upper) && bs[0] == r.sweeps && bs[1] == r.status);
        const L0NodeBatch b0{1, cells_i, wi, wo, nullptr, has_start ? start.data() : nullptr, &bl, &bp, &bu, u2.data(), bs};  // no parent's bound
        CHECK(l0_node_batch_host(G.data(), (size_t)p, c.data(), p, &nc, max_sweeps, gap_tol, b0) == 0 && same(bl, r.lower));
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
    long long launches = 0, most = 0;
    const int rc = l0_prove_tree(G.data(), (size_t)p, c.data(), p, n_cells, nc.data(), has_inc ? inc.data() : nullptr, rel_gap, max_nodes, width,
                                 [&](const L0NodeBatch& b) {
                                   ++launches;
                                   most = b.n > most ? b.n : most;
                                   return l0_node_batch_host(G.data(), (size_t)p, c.data(), p, nc.data(), max_sweeps, rel_gap / 100.0, b);
                                 },
                                 beta.data(), obj.data(), low.data(), nodes.data(), rounds.data(), status.data(), &leaves);
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
  long long which = -1;
  CHECK(l0_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 5, 1e-9, true, false) == L0_ND_OK);
  CHECK(l0_nodes_check(2, nullptr, et, 1.0, 2, cell, in, out, nullptr, nullptr, 5, 1e-9, true, false) == L0_ND_NULL);
  CHECK(l0_nodes_check(2, al, et, 1.0, 2, cell, nullptr, out, nullptr, nullptr, 5, 1e-9, true, false) == L0_ND_NULL);
  CHECK(l0_nodes_check(0, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 5, 1e-9, true, false) == L0_ND_CELLS);
  CHECK(l0_nodes_check(8193, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 5, 1e-9, true, false) == L0_ND_PROBLEMS);
  CHECK(l0_nodes_check(2, al, et, 1.0, 0, cell, in, out, nullptr, nullptr, 5, 1e-9, true, false) == L0_ND_NODES);
  CHECK(l0_nodes_check(2, al, et, 1.0, 8193, cell, in, out, nullptr, nullptr, 5, 1e-9, true, false) == L0_ND_BATCH);
  CHECK(l0_nodes_check(2, al, et, -1.0, 2, cell, in, out, nullptr, nullptr, 5, 1e-9, true, false) == L0_ND_BIG_M);
  const double bad[2] = {0.1, -1.0};
  CHECK(l0_nodes_check(2, bad, et, 1.0, 2, cell, in, out, nullptr, nullptr, 5, 1e-9, true, false, &which) == L0_ND_ALPHA && which == 1);
  CHECK(l0_nodes_check(2, al, bad, 1.0, 2, cell, in, out, nullptr, nullptr, 5, 1e-9, true, false, &which) == L0_ND_ETA && which == 1);
  CHECK(l0_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 5, -1.0, true, false) == L0_ND_GAP_TOL);
  CHECK(l0_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 1025, 1e-9, true, false) == L0_ND_WIDTH);
  const int far[2] = {0, 2};
  CHECK(l0_nodes_check(2, al, et, 1.0, 2, far, in, out, nullptr, nullptr, 5, 1e-9, true, false, &which) == L0_ND_CELL && which == 1);
  in[L0_ND_WORDS + 1] = 4;
  out[L0_ND_WORDS + 1] = 6;
  CHECK(l0_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 5, 1e-9, true, false, &which) == L0_ND_MASK && which == 1);
  out[L0_ND_WORDS + 1] = 2;
  double par[2] = {-INFINITY, NAN};
  CHECK(l0_nodes_check(2, al, et, 1.0, 2, cell, in, out, par, nullptr, 5, 1e-9, true, false, &which) == L0_ND_PARENT && which == 1);
  par[1] = INFINITY;
  CHECK(l0_nodes_check(2, al, et, 1.0, 2, cell, in, out, par, nullptr, 5, 1e-9, true, false, &which) == L0_ND_PARENT && which == 1);
  par[1] = -3.5;
  CHECK(l0_nodes_check(2, al, et, 1.0, 2, cell, in, out, par, nullptr, 5, 1e-9, true, false) == L0_ND_OK);
  double st[10] = {0.0};
  st[7] = INFINITY;
  CHECK(l0_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, st, 5, 1e-9, true, false, &which) == L0_ND_START && which == 7);
  CHECK(l0_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 5, 1e-9, false, false) == L0_ND_GROUPS);
  CHECK(l0_nodes_check(2, al, et, 1.0, 2, cell, in, out, nullptr, nullptr, 5, 1e-9, true, true) == L0_ND_SHARDED);

  CHECK(l0_prove_check(2, al, et, 1.0, nullptr, 5, 1e-6, 100, 4, true, false) == L0_PV_OK);
  CHECK(l0_prove_check(2, al, nullptr, 1.0, nullptr, 5, 1e-6, 100, 4, true, false) == L0_PV_NULL);
  CHECK(l0_prove_check(0, al, et, 1.0, nullptr, 5, 1e-6, 100, 4, true, false) == L0_PV_CELLS);
  CHECK(l0_prove_check(8193, al, et, 1.0, nullptr, 5, 1e-6, 100, 4, true, false) == L0_PV_PROBLEMS);
  CHECK(l0_prove_check(2, al, et, -1.0, nullptr, 5, 1e-6, 100, 4, true, false) == L0_PV_BIG_M);
  CHECK(l0_prove_check(2, bad, et, 1.0, nullptr, 5, 1e-6, 100, 4, true, false) == L0_PV_ALPHA);
  CHECK(l0_prove_check(2, al, bad, 1.0, nullptr, 5, 1e-6, 100, 4, true, false) == L0_PV_ETA);
  CHECK(l0_prove_check(2, al, et, 1.0, nullptr, 5, 1e-11, 100, 4, true, false) == L0_PV_REL_GAP);
  CHECK(l0_prove_check(2, al, et, 1.0, nullptr, 5, 1.5, 100, 4, true, false) == L0_PV_REL_GAP);
  CHECK(l0_prove_check(2, al, et, 1.0, nullptr, 5, NAN, 100, 4, true, false) == L0_PV_REL_GAP);
  CHECK(l0_prove_check(2, al, et, 1.0, nullptr, 5, 1e-6, 0, 4, true, false) == L0_PV_MAX_NODES);
  CHECK(l0_prove_check(2, al, et, 1.0, nullptr, 5, 1e-6, 100, 0, true, false) == L0_PV_TREE_WIDTH);
  CHECK(l0_prove_check(2, al, et, 1.0, nullptr, 1025, 1e-6, 100, 4, true, false) == L0_PV_WIDTH);
  double inc[10] = {0.0};
  inc[3] = 1.5;
  CHECK(l0_prove_check(2, al, et, 1.0, inc, 5, 1e-6, 100, 4, true, false, &which) == L0_PV_INCUMBENT && which == 3);
  inc[3] = NAN;
  CHECK(l0_prove_check(2, al, et, 1.0, inc, 5, 1e-6, 100, 4, true, false, &which) == L0_PV_INCUMBENT && which == 3);
  inc[3] = 1.0;
  CHECK(l0_prove_check(2, al, et, 1.0, inc, 5, 1e-6, 100, 4, true, false) == L0_PV_OK);
  CHECK(l0_prove_check(2, al, et, 1.0, nullptr, 5, 1e-6, 100, 4, false, false) == L0_PV_GROUPS);
  CHECK(l0_prove_check(2, al, et, 1.0, nullptr, 5, 1e-6, 100, 4, true, true) == L0_PV_SHARDED);
}

// a tree that runs out of nodes still reports a proven bound, and one node is the root alone
static void test_node_limit() {
  const int p = 6;
  std::vector<double> G((size_t)p * p), c((size_t)p);
  for (int i = 0; i < p; ++i) {
    c[(size_t)i] = 0.3 + 0.1 * i;
    for (int j = 0; j < p; ++j) G[(size_t)i * p + j] = i == j ? 1.0 : 0.6;
  }
  const L0NodeCell nc = l0_node_cell(0.02, 0.0, 100.0);
  for (int max_nodes : {1, 2, 3, 4096}) {
    std::vector<double> beta((size_t)p);
    double obj = 0.0, low = 0.0;
    int nodes = 0, rounds = 0, status = -1;
    CHECK(l0_prove_tree(G.data(), (size_t)p, c.data(), p, 1, &nc, nullptr, 1e-6, max_nodes, 1,
                        [&](const L0NodeBatch& b) { return l0_node_batch_host(G.data(), (size_t)p, c.data(), p, &nc, 10000, 1e-8, b); }, beta.data(),
                        &obj, &low, &nodes, &rounds, &status) == 0);
    CHECK(nodes <= max_nodes && low <= obj && (status == L0_PV_OPTIMAL || status == L0_PV_NODE_LIMIT));
    if (max_nodes <= 2) CHECK(nodes == 1 && rounds == 1);
    if (max_nodes == 4096) CHECK(status == L0_PV_OPTIMAL && obj - low <= 1e-6 * std::fmax(std::fabs(obj), nc.alpha));
    CHECK(std::fabs(l0_prove_value(G.data(), (size_t)p, c.data(), p, nc.alpha, nc.eta, beta.data()) - obj) <= 1e-12);
    printf("max_nodes %d: nodes %d rounds %d status %d objective %.9e bound %.9e\n", max_nodes, nodes, rounds, status, obj, low);
  }
}

int main(int argc, char** argv) {
  test_checks();
  test_node_limit();
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
    printf("l0_local_prove_host_test: %d FAILED\n", failures);
    return 1;
  }
  printf("l0_local_prove_host_test: ok\n");
  return 0;
}
