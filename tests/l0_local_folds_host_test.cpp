// CPU test of the host side of the l0 local search over row sets (slm_solve_l0_local_folds) in csrc/l0_host.hpp: the argument
// check l0_lsf_check with every refusal and their order, the index map l0_lsf_index / l0_lsf_split, the elimination of the ones
// column at a leading dimension (l0_eliminate_last_ld, l0_eliminate_vectors) against l0_eliminate_last, and l0_local_solve<false> on an
// eliminated Gram against l0_local_solve<false> on the Gram of explicitly centred columns -- meant to run under AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_l0_local_cv_cpu.py builds and runs it both plainly and sanitized).
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../sparse-lm_amd/csrc/l0_host.hpp"

using namespace slm;

static int failures = 0;
#define CHECK(cond)                                                           \
  do {                                                                        \
    if (!(cond)) {                                                            \
      fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #cond, __FILE__, __LINE__); \
      ++failures;                                                             \
    }                                                                         \
  } while (0)

// an n x p design from a fixed recurrence, neighbouring columns correlated, every column shifted by `shift`; weights w
struct Data {
  int n = 0, p = 0;
  std::vector<double> A, y, w;
};
static Data data(int n, int p, double shift) {
  Data D;
  D.n = n;
  D.p = p;
  D.A.resize((size_t)n * p);
  D.y.resize((size_t)n);
  D.w.resize((size_t)n);
  unsigned v = 4711u;
  auto next = [&]() {
    v = v * 1103515245u + 12345u;
    return (double)((v >> 16) & 0x3ff) / 512.0 - 1.0;
  };
  for (int i = 0; i < n; ++i) {
    for (int j = 0; j < p; ++j) D.A[(size_t)i * p + j] = (j ? 0.4 * (D.A[(size_t)i * p + j - 1] - shift) : 0.0) + next() + shift;
    D.y[(size_t)i] = 0.3 * next() + 2.0;
    for (int j = 1; j < p; j += 3) D.y[(size_t)i] += ((j & 1) ? -1.0 : 1.0) * D.A[(size_t)i * p + j];
    D.w[(size_t)i] = 0.5 + 0.25 * (double)(i % 5);
  }
  double sum = 0.0;
  for (double x : D.w) sum += x;
  for (double& x : D.w) x *= n / sum;
  return D;
}
// the weighted Gram of the columns `cols` of B [n][q] (B: the design with whatever was appended or subtracted), [m][ld], padding NaN
static void gram(const Data& D, const std::vector<double>& B, int q, const std::vector<double>& t, size_t ld, std::vector<double>& G,
                 std::vector<double>& c, double* yy) {
  G.assign((size_t)q * ld, NAN);
  c.assign((size_t)q, 0.0);
  *yy = 0.0;
  for (int i = 0; i < q; ++i) {
    for (int j = 0; j < q; ++j) {
      double s = 0.0;
      for (int k = 0; k < D.n; ++k) s += D.w[(size_t)k] * B[(size_t)k * q + i] * B[(size_t)k * q + j];
      G[(size_t)i * ld + j] = s / D.n;
    }
    for (int k = 0; k < D.n; ++k) c[(size_t)i] += D.w[(size_t)k] * B[(size_t)k * q + i] * t[(size_t)k] / D.n;
  }
  for (int k = 0; k < D.n; ++k) *yy += D.w[(size_t)k] * t[(size_t)k] * t[(size_t)k] / D.n;
}

static void test_check() {
  const double al[3] = {0.1, 0.2, 0.0}, et[3] = {0.0, 0.5, 0.0};
  const double w0[4] = {1.0, 0.0, 2.0, 1.0}, w1[4] = {1.0, 1.0, 1.0, 1.0};
  const double* rw[3] = {w0, nullptr, w1};
  const long long ne[3] = {3, 0, 4};
  auto check = [&](long long count, const double* const* rws, const long long* nes, bool icpt, bool alone, long long cells, const double* a,
                   const double* e, double M, long long starts_n, const double* st, long long p) {
    return l0_lsf_check(count, rws, nes, 4, icpt, alone, cells, a, e, M, starts_n, st, p);
  };
  CHECK(check(3, rw, ne, false, true, 3, al, et, 1.0, 1, nullptr, 5).kind == L0_LSF_OK);
  CHECK(check(3, rw, ne, true, true, 3, al, et, 1.0, 1, nullptr, 5).kind == L0_LSF_OK);
  // the count first (no row set: no table of them either), then NULL arguments, both before anything about the cells
  CHECK(check(0, nullptr, nullptr, false, true, 0, nullptr, nullptr, 1.0, 1, nullptr, 5).kind == L0_LSF_COUNT);
  CHECK(check(3, nullptr, ne, false, true, 3, al, et, 1.0, 1, nullptr, 5).kind == L0_LSF_NULL);
  CHECK(check(3, rw, nullptr, false, true, 3, al, et, 1.0, 1, nullptr, 5).kind == L0_LSF_NULL);
  CHECK(check(3, rw, ne, false, true, 0, nullptr, et, 1.0, 1, nullptr, 5).kind == L0_LSF_NULL);
  CHECK(check(3, rw, ne, false, true, 0, al, nullptr, 1.0, 1, nullptr, 5).kind == L0_LSF_NULL);
  CHECK(check(0, rw, ne, false, true, 0, al, et, 1.0, 1, nullptr, 5).kind == L0_LSF_COUNT);
  CHECK(check(-1, rw, ne, false, true, 3, al, et, 1.0, 1, nullptr, 5).kind == L0_LSF_COUNT);
  CHECK(check(17, rw, ne, false, true, 3, al, et, 1.0, 1, nullptr, 5).kind == L0_LSF_COUNT);
  // what slm_solve_l0_local refuses, in its order
  L0LsfRefusal R = check(3, rw, ne, false, true, 0, al, et, 1.0, 0, nullptr, 5);
  CHECK(R.kind == L0_LSF_LS && R.ls == L0_LS_CELLS);
  R = check(3, rw, ne, false, true, 3, al, et, -1.0, 0, nullptr, 5);
  CHECK(R.kind == L0_LSF_LS && R.ls == L0_LS_STARTS);
  R = check(3, rw, ne, false, true, 3, al, et, -1.0, 1, nullptr, 5000);
  CHECK(R.kind == L0_LSF_LS && R.ls == L0_LS_BIG_M);
  R = check(3, rw, ne, false, true, 3, al, et, NAN, 1, nullptr, 5);
  CHECK(R.kind == L0_LSF_LS && R.ls == L0_LS_BIG_M);
  const double bad_al[3] = {0.1, -0.2, NAN}, bad_et[3] = {0.0, 0.0, INFINITY};
  R = check(3, rw, ne, false, true, 3, bad_al, bad_et, 1.0, 1, nullptr, 5);
  CHECK(R.kind == L0_LSF_LS && R.ls == L0_LS_ALPHA && R.which == 1);
  R = check(3, rw, ne, false, true, 3, al, bad_et, 1.0, 1, nullptr, 5);
  CHECK(R.kind == L0_LSF_LS && R.ls == L0_LS_ETA && R.which == 2);
  // the product of the three factors: each pair may fit
  {
    std::vector<double> a((size_t)L0_LS_MAX_PROBLEMS + 1, 0.1), e((size_t)L0_LS_MAX_PROBLEMS + 1, 0.0);
    const double* sixteen[16] = {};
    const long long n16[16] = {};
    CHECK(check(16, sixteen, n16, false, true, 512, a.data(), e.data(), 1.0, 1, nullptr, 5).kind == L0_LSF_OK);
    CHECK(check(16, sixteen, n16, false, true, 513, a.data(), e.data(), 1.0, 1, nullptr, 5).kind == L0_LSF_PRODUCT);
    CHECK(check(16, sixteen, n16, false, true, 256, a.data(), e.data(), 1.0, 2, nullptr, 5).kind == L0_LSF_OK);
    CHECK(check(16, sixteen, n16, false, true, 256, a.data(), e.data(), 1.0, 3, nullptr, 5).kind == L0_LSF_PRODUCT);
    CHECK(check(2, sixteen, n16, false, true, 4096, a.data(), e.data(), 1.0, 1, nullptr, 5).kind == L0_LSF_OK);
    CHECK(check(3, sixteen, n16, false, true, 4096, a.data(), e.data(), 1.0, 1, nullptr, 5).kind == L0_LSF_PRODUCT);
    CHECK(check(1, sixteen, n16, false, true, L0_LS_MAX_PROBLEMS + 1, a.data(), e.data(), 1.0, 1, nullptr, 5).kind == L0_LSF_PRODUCT);
    CHECK(check(1, sixteen, n16, false, true, 1 << 30, a.data(), e.data(), 1.0, 1 << 30, nullptr, 5).kind == L0_LSF_PRODUCT);  // (no overflow)
    // the product comes before a bad alpha, as n_cells * n_starts does in l0_ls_check
    a[0] = -1.0;
    CHECK(check(3, sixteen, n16, false, true, 4096, a.data(), e.data(), 1.0, 1, nullptr, 5).kind == L0_LSF_PRODUCT);
  }
  // the width counts the searched columns: 1025 with the intercept's, 1024 without
  CHECK(check(3, rw, ne, true, true, 3, al, et, 1.0, 1, nullptr, L0_LS_PMAX + 1).kind == L0_LSF_OK);
  R = check(3, rw, ne, true, true, 3, al, et, 1.0, 1, nullptr, L0_LS_PMAX + 2);
  CHECK(R.kind == L0_LSF_LS && R.ls == L0_LS_WIDTH);
  CHECK(check(3, rw, ne, false, true, 3, al, et, 1.0, 1, nullptr, L0_LS_PMAX).kind == L0_LSF_OK);
  R = check(3, rw, ne, false, true, 3, al, et, 1.0, 1, nullptr, L0_LS_PMAX + 1);
  CHECK(R.kind == L0_LSF_LS && R.ls == L0_LS_WIDTH);
  // the intercept column: last and alone, and there at all
  CHECK(check(3, rw, ne, true, false, 3, al, et, 1.0, 1, nullptr, 5).kind == L0_LSF_INTERCEPT);
  CHECK(check(3, rw, ne, true, true, 3, al, et, 1.0, 1, nullptr, 0).kind == L0_LSF_INTERCEPT);
  CHECK(check(3, rw, ne, false, false, 3, al, et, 1.0, 1, nullptr, 5).kind == L0_LSF_OK);  // (without an intercept nobody asks)
  // the weights: negative, NaN, infinite; a NULL row set is skipped
  double wbad[4] = {1.0, 1.0, -0.5, 1.0};
  const double* rwb[3] = {w0, nullptr, wbad};
  R = check(3, rwb, ne, false, true, 3, al, et, 1.0, 1, nullptr, 5);
  CHECK(R.kind == L0_LSF_WEIGHT && R.row_set == 2 && R.which == 2);
  wbad[2] = 1.0;
  wbad[3] = NAN;
  R = check(3, rwb, ne, false, true, 3, al, et, 1.0, 1, nullptr, 5);
  CHECK(R.kind == L0_LSF_WEIGHT && R.row_set == 2 && R.which == 3);
  wbad[3] = INFINITY;
  CHECK(check(3, rwb, ne, false, true, 3, al, et, 1.0, 1, nullptr, 5).kind == L0_LSF_WEIGHT);
  wbad[3] = 0.0;
  CHECK(check(3, rwb, ne, false, true, 3, al, et, 1.0, 1, nullptr, 5).kind == L0_LSF_OK);
  // the starts: count * n_cells * n_starts * ps of them, ps without the intercept's column
  {
    std::vector<double> st((size_t)3 * 3 * 2 * 4, 0.5);
    CHECK(check(3, rw, ne, true, true, 3, al, et, 1.0, 2, st.data(), 5).kind == L0_LSF_OK);
    st.back() = 1.5;
    R = check(3, rw, ne, true, true, 3, al, et, 1.0, 2, st.data(), 5);
    CHECK(R.kind == L0_LSF_LS && R.ls == L0_LS_START_BOX && R.which == (long long)st.size() - 1);
    st.back() = 0.5;
    st[7] = NAN;
    R = check(3, rw, ne, true, true, 3, al, et, 1.0, 2, st.data(), 5);
    CHECK(R.kind == L0_LSF_LS && R.ls == L0_LS_START_BOX && R.which == 7);
    // a bad weight comes before a bad start
    CHECK(check(3, rwb, ne, true, true, 3, al, et, 1.0, 2, st.data(), 5).kind == L0_LSF_LS);
    wbad[0] = -1.0;
    CHECK(check(3, rwb, ne, true, true, 3, al, et, 1.0, 2, st.data(), 5).kind == L0_LSF_WEIGHT);
  }
}

static void test_index_map() {
  const int shapes[5][3] = {{1, 1, 1}, {16, 3, 1}, {4, 7, 5}, {16, 130, 1}, {3, 2, 9}};
  for (const auto& sh : shapes) {
    const int count = sh[0], cells = sh[1], starts = sh[2], total = count * cells * starts;
    std::vector<char> seen((size_t)total, 0);
    int expect = 0;
    for (int r = 0; r < count; ++r)
      for (int e = 0; e < cells; ++e)
        for (int s = 0; s < starts; ++s) {
          const int q = l0_lsf_index(r, e, s, cells, starts);
          CHECK(q == expect++);  // row sets outermost, starts innermost
          CHECK(q >= 0 && q < total && !seen[(size_t)q]);
          if (q >= 0 && q < total) seen[(size_t)q] = 1;
          const L0LsfProblem P = l0_lsf_split(q, cells, starts);
          CHECK(P.r == r && P.e == e && P.s == s);
        }
    for (char c : seen) CHECK(c);
  }
  // one row set: the map of slm_solve_l0_local, cell q / n_starts
  for (int q = 0; q < 35; ++q) CHECK(l0_lsf_split(q, 7, 5).r == 0 && l0_lsf_split(q, 7, 5).e == q / 5);
}

// [A | 1]: its Gram at a leading dimension, the ones column eliminated, against l0_eliminate_last on the dense copy
static void test_elimination(size_t ld_extra) {
  const Data D = data(23, 9, 1.5);
  const int p = D.p + 1;
  const size_t ld = (size_t)p + ld_extra, lds = (size_t)(p - 1) + (ld_extra ? ld_extra + 2 : 0);
  std::vector<double> B((size_t)D.n * p);
  for (int i = 0; i < D.n; ++i) {
    for (int j = 0; j < D.p; ++j) B[(size_t)i * p + j] = D.A[(size_t)i * D.p + j];
    B[(size_t)i * p + D.p] = 1.0;
  }
  std::vector<double> G, c, Gd, cd;
  double yy = 0.0, yyd = 0.0;
  gram(D, B, p, D.y, ld, G, c, &yy);
  gram(D, B, p, D.y, (size_t)p, Gd, cd, &yyd);
  const int q = p - 1;
  std::vector<double> want((size_t)q * q), want_c((size_t)q), want_x((size_t)q), got((size_t)q * lds, NAN), got_c((size_t)q), got_x((size_t)q);
  double want_yy = 0.0, want_ym = 0.0, got_yy = 0.0, got_ym = 0.0;
  CHECK(l0_eliminate_last(Gd.data(), cd.data(), p, yyd, want.data(), want_c.data(), &want_yy, want_x.data(), &want_ym));
  CHECK(l0_eliminate_last_ld(G.data(), ld, c.data(), p, yy, got.data(), lds, got_c.data(), &got_yy, got_x.data(), &got_ym));
  CHECK(got_yy == want_yy && got_ym == want_ym);
  for (int i = 0; i < q; ++i) {
    CHECK(got_c[(size_t)i] == want_c[(size_t)i] && got_x[(size_t)i] == want_x[(size_t)i]);
    for (int j = 0; j < q; ++j) CHECK(got[(size_t)i * lds + j] == want[(size_t)i * q + j]);  // the same bits: the same arithmetic
    for (size_t j = (size_t)q; j < lds; ++j) CHECK(isnan(got[(size_t)i * lds + j]));         // the padding is left alone
  }
  // the vectors alone from the LAST ROW (what the engine fetches; the Gram is symmetric)
  std::vector<double> vc((size_t)q), vx((size_t)q);
  double vyy = 0.0, vym = 0.0;
  CHECK(l0_eliminate_vectors(G.data() + (size_t)q * ld, G[(size_t)q * ld + q], c.data(), q, yy, vc.data(), &vyy, vx.data(), &vym));
  CHECK(vyy == want_yy && vym == want_ym);
  for (int i = 0; i < q; ++i) CHECK(vc[(size_t)i] == want_c[(size_t)i] && vx[(size_t)i] == want_x[(size_t)i]);
  // a ones column without weight is refused, by both
  G[(size_t)q * ld + q] = 0.0;
  CHECK(!l0_eliminate_last_ld(G.data(), ld, c.data(), p, yy, got.data(), lds, got_c.data(), &got_yy, got_x.data(), &got_ym));
  CHECK(!l0_eliminate_vectors(G.data() + (size_t)q * ld, NAN, c.data(), q, yy, vc.data(), &vyy, vx.data(), &vym));
}

// the rule on the eliminated Gram of [A | 1] against the rule on the Gram of explicitly centred columns: the same supports and swap
// counts, objectives and coefficients to rounding (the two Grams differ by the elimination's cancellation: shift 1.5, spread ~0.6)
static void test_solve_on_eliminated() {
  const Data D = data(40, 12, 1.5);
  const int q = D.p, p = q + 1;
  const size_t ld = 16, lds = 16;
  std::vector<double> B((size_t)D.n * p), C((size_t)D.n * q), t(D.y);
  std::vector<double> mean((size_t)q, 0.0);
  double ymean = 0.0;
  for (int i = 0; i < D.n; ++i) {
    for (int j = 0; j < q; ++j) mean[(size_t)j] += D.w[(size_t)i] * D.A[(size_t)i * q + j] / D.n;
    ymean += D.w[(size_t)i] * D.y[(size_t)i] / D.n;
  }
  for (int i = 0; i < D.n; ++i) {
    for (int j = 0; j < q; ++j) {
      B[(size_t)i * p + j] = D.A[(size_t)i * q + j];
      C[(size_t)i * q + j] = D.A[(size_t)i * q + j] - mean[(size_t)j];
    }
    B[(size_t)i * p + q] = 1.0;
    t[(size_t)i] = D.y[(size_t)i] - ymean;
  }
  std::vector<double> G, c, Gc, cc, Ge((size_t)q * lds, NAN), ce((size_t)q), xm((size_t)q);
  double yy = 0.0, yyc = 0.0, yye = 0.0, ym = 0.0;
  gram(D, B, p, D.y, ld, G, c, &yy);
  gram(D, C, q, t, lds, Gc, cc, &yyc);
  CHECK(l0_eliminate_last_ld(G.data(), ld, c.data(), p, yy, Ge.data(), lds, ce.data(), &yye, xm.data(), &ym));
  CHECK(fabs(ym - ymean) <= 1e-14 * fabs(ymean) && fabs(yye - yyc) <= 1e-12 * yyc);
  for (int j = 0; j < q; ++j) CHECK(fabs(xm[(size_t)j] - mean[(size_t)j]) <= 1e-14 * fabs(mean[(size_t)j]));
  int nonempty = 0, swapped = 0;
  for (double rel : {0.002, 0.02, 0.2})
    for (double eta : {0.0, 0.05})
      for (bool swaps : {false, true}) {
        const double alpha = rel * yyc;
        std::vector<double> be((size_t)q), bc((size_t)q);
        const L0LsResult Re = l0_local_solve<false>(Ge.data(), lds, ce.data(), q, alpha, eta, 100.0, yye, swaps, nullptr, be.data());
        const L0LsResult Rc = l0_local_solve<false>(Gc.data(), lds, cc.data(), q, alpha, eta, 100.0, yyc, swaps, nullptr, bc.data());
        CHECK(Re.status == 0 && Rc.status == 0 && Re.swaps == Rc.swaps && Re.nnz == Rc.nnz);
        CHECK(fabs(Re.F - Rc.F) <= 1e-10 * fmax(fabs(Rc.F), alpha));
        for (int j = 0; j < q; ++j) {
          CHECK((be[(size_t)j] != 0.0) == (bc[(size_t)j] != 0.0));
          CHECK(fabs(be[(size_t)j] - bc[(size_t)j]) <= 1e-9 * fmax(1.0, fabs(bc[(size_t)j])));
        }
        nonempty += Rc.nnz > 0;
        swapped += Rc.swaps > 0;
      }
  CHECK(nonempty >= 8);
  printf("solve on the eliminated Gram: %d of 12 runs with a support, %d with a swap\n", nonempty, swapped);
}

int main() {
  test_check();
  test_index_map();
  test_elimination(0);  // ld = p
  test_elimination(7);  // ld > p, and another one for the result
  test_solve_on_eliminated();
  if (failures) {
    fprintf(stderr, "l0_local_folds_host_test: %d failure(s)\n", failures);
    return 1;
  }
  printf("l0_local_folds_host_test: ok\n");
  return 0;
}
