// The host side of slm_solve_l0_local_groups without a device (csrc/l0_host.hpp, "local groups"): l0_lg_close, l0_lg_closure,
// l0_lg_check and the kernel's twin l0_lg_solve.  The twin runs on the cases that tests/test_l0_local_groups_cpu.py exports
// from the numpy restatement (argv[1]); every case was taken with a decision margin >= 1e-6, so supports, counts and the
// closure must be identical and F equal to 1e-10 relative.  Built with g++, plainly and with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <type_traits>
#include <vector>

#include "../sparse-lm_amd/csrc/l0_host.hpp"

using namespace slm;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static std::vector<int> closed_of(const std::vector<int>& cptr, const std::vector<int>& cidx, int g) {
  return std::vector<int>(cidx.begin() + cptr[(size_t)g], cidx.begin() + cptr[(size_t)g + 1]);
}

static void test_close() {
  std::vector<int> cptr, cidx;
  {  // a chain 3 -> 2 -> 1 -> 0
    const int ptr[] = {0, 0, 1, 2, 3}, idx[] = {0, 1, 2};
    l0_lg_close(4, ptr, idx, cptr, cidx);
    CHECK(closed_of(cptr, cidx, 0).empty());
    CHECK((closed_of(cptr, cidx, 3) == std::vector<int>{0, 1, 2}));
    CHECK((closed_of(cptr, cidx, 2) == std::vector<int>{0, 1}));
  }
  {  // a two-cycle 0 <-> 1, and 2 needing 1: a group is never in its own list
    const int ptr[] = {0, 1, 2, 3}, idx[] = {1, 0, 1};
    l0_lg_close(3, ptr, idx, cptr, cidx);
    CHECK((closed_of(cptr, cidx, 0) == std::vector<int>{1}));
    CHECK((closed_of(cptr, cidx, 1) == std::vector<int>{0}));
    CHECK((closed_of(cptr, cidx, 2) == std::vector<int>{0, 1}));
    const int gstart[] = {0, 2, 3, 5};
    const double beta[] = {0, 0, 0, 0, 0.5};
    int in[3];
    CHECK(l0_lg_closure(beta, 3, gstart, cptr.data(), cidx.data(), in) == 3 && in[0] && in[1] && in[2]);
    const double beta0[] = {0, 1.0, 0, 0, 0};
    CHECK(l0_lg_closure(beta0, 3, gstart, cptr.data(), cidx.data(), in) == 2 && in[0] && in[1] && !in[2]);
  }
  {  // a diamond 3 -> {1, 2} -> 0, with a duplicate entry
    const int ptr[] = {0, 0, 1, 2, 5}, idx[] = {0, 0, 1, 2, 1};
    l0_lg_close(4, ptr, idx, cptr, cidx);
    CHECK((closed_of(cptr, cidx, 3) == std::vector<int>{0, 1, 2}));
  }
  l0_lg_close(3, nullptr, nullptr, cptr, cidx);
  CHECK(cptr.size() == 4 && cptr[3] == 0 && cidx.empty());
}

static void test_check() {
  const double* rows[1] = {nullptr};
  const long long neff[1] = {0};
  const double al[2] = {0.1, 0.2}, et[2] = {0.0, 0.0};
  const int gid[6] = {0, 0, 1, 1, 2, 2};
  int ng = -1;
  auto call = [&](const int* g, const int* ptr, const int* idx, bool sharded, long long p = 6, bool intercept = false, bool alone = true) {
    return l0_lg_check(1, rows, neff, 10, intercept, alone, 2, al, et, 100.0, 1, nullptr, p, g, ptr, idx, sharded, &ng);
  };
  CHECK(call(gid, nullptr, nullptr, false).kind == L0_LG_OK && ng == 3);
  CHECK(call(nullptr, nullptr, nullptr, false).kind == L0_LG_OK && ng == 6);
  {  // the intercept's column and group are not searched
    const int gi[7] = {0, 0, 1, 1, 2, 2, 3};
    CHECK(call(gi, nullptr, nullptr, false, 7, true).kind == L0_LG_OK && ng == 3);
    const L0LgRefusal R = call(gi, nullptr, nullptr, false, 7, true, false);
    CHECK(R.kind == L0_LG_LSF && R.lsf.kind == L0_LSF_INTERCEPT);
  }
  {  // what the shared check refuses comes first
    const double bad[2] = {0.1, -1.0};
    const L0LgRefusal R = l0_lg_check(1, rows, neff, 10, false, true, 2, bad, et, 100.0, 1, nullptr, 6, gid, nullptr, nullptr, true);
    CHECK(R.kind == L0_LG_LSF && R.lsf.kind == L0_LSF_LS && R.lsf.ls == L0_LS_ALPHA && R.which == 1);
    const L0LgRefusal W = l0_lg_check(1, rows, neff, 10, false, true, 2, al, et, 100.0, 1, nullptr, 1025, nullptr, nullptr, nullptr, false);
    CHECK(W.kind == L0_LG_LSF && W.lsf.ls == L0_LS_WIDTH);
    CHECK(l0_lg_check(17, rows, neff, 10, false, true, 2, al, et, 100.0, 1, nullptr, 6, gid, nullptr, nullptr, false).lsf.kind == L0_LSF_COUNT);
  }
  {  // groups that are not contiguous, not ascending, or do not start at 0
    const int apart[6] = {0, 1, 0, 1, 2, 2}, down[6] = {1, 1, 0, 0, 2, 2}, gap[6] = {0, 0, 2, 2, 3, 3}, late[6] = {1, 1, 2, 2, 3, 3};
    L0LgRefusal R = call(apart, nullptr, nullptr, false);
    CHECK(R.kind == L0_LG_ORDER && R.which == 2);
    R = call(down, nullptr, nullptr, false);
    CHECK(R.kind == L0_LG_ORDER && R.which == 0);
    R = call(gap, nullptr, nullptr, false);
    CHECK(R.kind == L0_LG_ORDER && R.which == 2);
    CHECK(call(late, nullptr, nullptr, false).kind == L0_LG_ORDER);
  }
  {  // the need lists
    const int ptr[4] = {0, 0, 1, 2}, idx[2] = {0, 1}, falls[4] = {0, 2, 1, 2}, off[4] = {1, 1, 1, 2}, out[2] = {0, 3}, neg[2] = {-1, 0};
    CHECK(call(gid, ptr, idx, false).kind == L0_LG_OK);
    L0LgRefusal R = call(gid, falls, idx, false);
    CHECK(R.kind == L0_LG_NEED_PTR && R.which == 2);
    CHECK(call(gid, off, idx, false).kind == L0_LG_NEED_PTR);
    R = call(gid, ptr, out, false);
    CHECK(R.kind == L0_LG_NEED_IDX && R.which == 1);
    R = call(gid, ptr, neg, false);
    CHECK(R.kind == L0_LG_NEED_IDX && R.which == 0);
    CHECK(call(gid, ptr, nullptr, false).kind == L0_LG_NEED_IDX);
    CHECK(call(gid, ptr, idx, true).kind == L0_LG_SHARDED);  // (last: everything about the arguments comes first)
    CHECK(call(gid, ptr, out, true).kind == L0_LG_NEED_IDX);
  }
}

template <class T>
static std::vector<T> take(std::ifstream& in, size_t n) {
  std::vector<T> v(n);
  for (size_t i = 0; i < n; ++i) in >> v[i];
  return v;
}

static int test_cases(const char* path) {
  std::ifstream in(path);
  int cases = 0;
  in >> cases;
  CHECK(in.good() && cases > 0);
  for (int t = 0; t < cases && in.good(); ++t) {
    int p, ng, swaps, has_start;
    double alpha, eta, big_M, yy;
    in >> p >> ng >> alpha >> eta >> big_M >> yy >> swaps >> has_start;
    const std::vector<int> gstart = take<int>(in, (size_t)ng + 1), ptr = take<int>(in, (size_t)ng + 1);
    const std::vector<int> idx = take<int>(in, (size_t)ptr[(size_t)ng]);
    const std::vector<double> G = take<double>(in, (size_t)p * p), c = take<double>(in, (size_t)p);
    const std::vector<double> start = take<double>(in, has_start ? (size_t)p : 0);
    int sweeps, nswaps, status, nclosed, nnz, trials;
    double F;
    in >> sweeps >> nswaps >> status >> nclosed >> nnz >> trials >> F;
    const std::vector<int> support = take<int>(in, (size_t)p), closed = take<int>(in, (size_t)ng);
    CHECK(!in.fail());
    if (in.fail()) break;
    const size_t ld = (size_t)p + 3;  // (a leading dimension that is not p; the padding holds NaN: it is never read)
    std::vector<double> Gl((size_t)p * ld, std::nan(""));
    for (int i = 0; i < p; ++i) std::memcpy(Gl.data() + (size_t)i * ld, G.data() + (size_t)i * p, sizeof(double) * (size_t)p);
    std::vector<int> cptr, cidx;
    l0_lg_close(ng, ptr.data(), idx.data(), cptr, cidx);
    cidx.push_back(0);  // (never an empty pointer)
    std::vector<double> beta((size_t)p);
    const L0LgResult R = l0_lg_solve(Gl.data(), ld, c.data(), p, ng, gstart.data(), cptr.data(), cidx.data(), alpha, eta, big_M, yy, swaps != 0,
                                     has_start ? start.data() : nullptr, beta.data());
    bool same = true;
    for (int j = 0; j < p; ++j) same = same && ((beta[(size_t)j] != 0.0) == (support[(size_t)j] != 0));
    std::vector<int> in_cl((size_t)ng);
    const int ncl = l0_lg_closure(beta.data(), ng, gstart.data(), cptr.data(), cidx.data(), in_cl.data());
    for (int g = 0; g < ng; ++g) same = same && (in_cl[(size_t)g] != 0) == (closed[(size_t)g] != 0);
    const double scale = std::max(std::fabs(F), alpha);
    const bool ok = same && R.sweeps == sweeps && R.swaps == nswaps && R.status == status && R.closed == nclosed && ncl == nclosed &&
                    R.nnz == nnz && R.trials == trials && std::fabs(R.F - F) <= 1e-10 * scale;
    if (!ok)
      std::printf("case %d (p %d, groups %d, alpha %g): twin sweeps %d swaps %d status %d closed %d nnz %d trials %d F %.15g; "
                  "restatement %d %d %d %d %d %d %.15g; supports %s\n", t, p, ng, alpha, R.sweeps, R.swaps, R.status, R.closed, R.nnz,
                  R.trials, R.F, sweeps, nswaps, status, nclosed, nnz, trials, F, same ? "equal" : "DIFFER");
    CHECK(ok);
    // the polish on a column list: the zeros it names are free, the value is the minimum on those columns
    std::vector<int> cols;
    for (int g = 0; g < ng; ++g)
      for (int j = gstart[(size_t)g]; j < gstart[(size_t)g + 1] && in_cl[(size_t)g]; ++j)
        if (Gl[(size_t)j * ld + j] + 2.0 * eta > 0.0) cols.push_back(j);
    std::vector<double> b2 = beta;
    const double q2 = l0_ls_polish_on(Gl.data(), ld, c.data(), eta, big_M, cols, b2.data());
    CHECK(q2 + alpha * ncl <= R.F + 1e-10 * scale);
  }
  return cases;
}

int main(int argc, char** argv) {
  test_close();
  test_check();
  int cases = 0;
  if (argc > 1) cases = test_cases(argv[1]);
  if (failures) {
    std::printf("l0_local_groups_host_test: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("l0_local_groups_host_test: ok (%d cases)\n", cases);
  return 0;
}
