// Compiled binding of the hot calls of include/slm_engine.h (pybind11): slm_solve_lanes, slm_solve_path_lanes and
// slm_dataset_create, with the marshalling of a call -- path points and their secant factors, penalty vectors, warm starts,
// row masks, result blocks -- done here instead of in Python, and the GIL released while the engine works.  This is the
// "thin pybind11 C-ABI" layer the estimators' `_solve` seam goes through (reference src/sparselm/model/_base.py:512-519:
// the cvxpy `problem.solve(...)` call); sparselm_amd/_engine.py keeps its ctypes binding of EVERY entry point -- the ABI's
// test harness, and the route of everything that is not hot.  Plain C ABI underneath: nothing here knows the engine's types.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>

#include <cmath>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/slm_engine.h"

namespace py = pybind11;
using arr_d = py::array_t<double, py::array::c_style | py::array::forcecast>;

namespace {

py::object g_engine_error, g_nonfinite_error;  // sparselm_amd._engine.EngineError / NonFiniteError

// status code -> the exception the ctypes layer raises for it (_engine._check)
void check(int rc) {
  if (rc == SLM_OK) return;
  const char* m = slm_last_error();
  const std::string msg = m ? m : "";
  switch (rc) {
    case SLM_ERR_BAD_ARG: throw py::value_error(msg);
    case SLM_ERR_OOM: PyErr_SetString(PyExc_MemoryError, msg.c_str()); throw py::error_already_set();
    case SLM_ERR_UNSUPPORTED: PyErr_SetString(PyExc_NotImplementedError, msg.c_str()); throw py::error_already_set();
    case SLM_ERR_NON_FINITE:
      if (g_nonfinite_error) {
        PyErr_SetString(g_nonfinite_error.ptr(), msg.c_str());
        throw py::error_already_set();
      }
      [[fallthrough]];
    default: {
      const std::string full = "[slm status " + std::to_string(rc) + "] " + msg;
      if (g_engine_error) {
        PyErr_SetString(g_engine_error.ptr(), full.c_str());
        throw py::error_already_set();
      }
      throw std::runtime_error(full);
    }
  }
}

// secant factors gamma_k = (s_k - s_{k-1}) / (s_{k-1} - s_{k-2}) of a path whose points are multiples s_k of one penalty
// direction; zeros otherwise (the rule of _engine.path_extrapolation)
void extrapolation(const double* pts, int64_t K, double* gam) {
  for (int64_t k = 0; k < K; ++k) gam[k] = 0.0;
  if (K < 3) return;
  int64_t best = 0;
  double top = -1.0, big = 0.0;
  for (int64_t k = 0; k < K; ++k) {
    const double v = std::fabs(pts[3 * k]) + std::fabs(pts[3 * k + 1]) + std::fabs(pts[3 * k + 2]);
    if (v > top) {
      top = v;
      best = k;
    }
    for (int c = 0; c < 3; ++c) big = std::max(big, std::fabs(pts[3 * k + c]));
  }
  const double* ref = pts + 3 * best;
  const double nrm = ref[0] * ref[0] + ref[1] * ref[1] + ref[2] * ref[2];
  if (!(nrm > 0.0)) return;
  std::vector<double> s((size_t)K);
  double off = 0.0;
  for (int64_t k = 0; k < K; ++k) {
    s[(size_t)k] = (pts[3 * k] * ref[0] + pts[3 * k + 1] * ref[1] + pts[3 * k + 2] * ref[2]) / nrm;
    for (int c = 0; c < 3; ++c) off = std::max(off, std::fabs(s[(size_t)k] * ref[c] - pts[3 * k + c]));
  }
  if (off > 1e-12 * big) return;  // the penalty changes shape along the path: a prediction would be meaningless
  for (int64_t k = 2; k < K; ++k) {
    const double den = s[(size_t)k - 1] - s[(size_t)k - 2], num = s[(size_t)k] - s[(size_t)k - 1];
    if (den == 0.0) continue;
    const double g = num / den;
    if (std::isfinite(g) && std::fabs(g) <= 10.0) gam[k] = g;
  }
}

// what a call keeps alive until the engine returns: converted arrays, broadcast vectors
struct Keep {
  std::vector<py::object> objs;
  std::vector<std::vector<double>> vecs;
  // one conversion per (Python object, length): lanes that share a row mask hand the engine the SAME pointer -- one
  // check, one upload, one Gram
  std::unordered_map<PyObject*, std::pair<int64_t, const double*>> seen;
};

// None -> nullptr; an array of `size` doubles; a scalar / one-element array -> `size` copies of it
const double* vector_arg(const py::handle& v, int64_t size, const char* name, Keep& keep) {
  if (v.is_none()) return nullptr;
  auto hit = keep.seen.find(v.ptr());
  if (hit != keep.seen.end() && hit->second.first == size) return hit->second.second;
  arr_d a = arr_d::ensure(v);
  if (!a) throw py::value_error(std::string(name) + " is not convertible to float64");
  const double* out = nullptr;
  if (a.size() == size) {
    out = a.data();
    keep.objs.push_back(a);
  } else if (a.size() == 1) {
    keep.vecs.emplace_back((size_t)size, *a.data());
    out = keep.vecs.back().data();
  } else {
    throw py::value_error(std::string(name) + " has " + std::to_string(a.size()) + " entries, expected " + std::to_string(size));
  }
  keep.seen[v.ptr()] = {size, out};
  return out;
}

py::object dict_get(const py::dict& d, const char* key) {
  py::str k(key);
  return d.contains(k) ? py::reinterpret_borrow<py::object>(d[k]) : py::none();
}

py::tuple stats_tuple(const slm_solve_stats& st) {
  return py::make_tuple(st.grad_launches, st.grad_timed, st.grad_ms_total, st.wall_ms, st.lipschitz_ms, st.ws_builds, st.ws_appends,
                        st.ws_refined, st.ws_misses, st.ws_columns, st.ws_inner_iters, st.ws_direct_steps, st.mg_rounds, st.mg_inner_iters,
                        st.mg_rejected, st.mg_build_ms, st.light_passes, st.light_columns);
}

py::array info_bytes(int64_t count) {
  return py::array_t<uint8_t>((py::ssize_t)(count * (int64_t)sizeof(slm_point_info)));
}

// slm_solve_lanes: `specs` is the list of lane dicts of Dataset.solve_lanes; `alloc(n)` hands out a float64 block of n
// entries (the binding's page-locked result pool).  Returns (betas block, group-norm block or None, records as bytes,
// points per lane, stats).
// `reweighted`: every spec carries "reweight" = (coef_scale, group_scale or None, numerator, eps, tol, n_coef, n_group) and the
// call is slm_solve_lanes_reweighted; the tuple then ends with the rounds run per lane.
py::tuple solve_lanes_any(uintptr_t ds, const py::list& specs, int64_t n, int64_t p, int64_t G, double tol, int max_iter, int check_every,
                          double L, uint32_t flags, bool want_gn, bool extrapolate, const py::object& alloc, bool reweighted) {
  const int nl = (int)specs.size();
  std::vector<slm_reweight> rules(reweighted ? (size_t)nl : 0);
  std::vector<int32_t> rounds(reweighted ? (size_t)nl : 0, 0);
  if (nl < 1 || nl > SLM_MAX_CELLS) throw py::value_error("between 1 and " + std::to_string(SLM_MAX_CELLS) + " lanes, got " + std::to_string(nl));
  Keep keep;
  std::vector<slm_lane> lanes((size_t)nl);
  std::vector<slm_penalty> pens((size_t)nl);
  std::vector<std::vector<slm_path_point>> points((size_t)nl);
  std::vector<int64_t> ks((size_t)nl);
  int64_t total = 0;
  for (int l = 0; l < nl; ++l) {
    const py::dict spec = py::reinterpret_borrow<py::dict>(specs[(size_t)l]);
    arr_d pts = arr_d::ensure(dict_get(spec, "points"));
    if (!pts || pts.size() % 3 != 0 || pts.size() == 0) throw py::value_error("lane " + std::to_string(l) + ": points must be (K, 3)");
    const int64_t K = pts.size() / 3;
    std::vector<double> gam((size_t)K, 0.0);
    const py::object ex = dict_get(spec, "extrap");
    if (!ex.is_none()) {
      arr_d e = arr_d::ensure(ex);
      if (!e || e.size() != K) throw py::value_error("extrap has the wrong length");
      std::memcpy(gam.data(), e.data(), sizeof(double) * (size_t)K);
    } else if (extrapolate) {
      extrapolation(pts.data(), K, gam.data());
    }
    points[(size_t)l].resize((size_t)K);
    for (int64_t k = 0; k < K; ++k) points[(size_t)l][(size_t)k] = slm_path_point{pts.data()[3 * k], pts.data()[3 * k + 1], pts.data()[3 * k + 2], gam[(size_t)k]};
    pens[(size_t)l].a = vector_arg(dict_get(spec, "a"), p, "a", keep);
    pens[(size_t)l].b = vector_arg(dict_get(spec, "b"), G, "b", keep);
    pens[(size_t)l].d = vector_arg(dict_get(spec, "d"), G, "d", keep);
    slm_lane& ln = lanes[(size_t)l];
    std::memset(&ln, 0, sizeof(ln));
    ln.pen = &pens[(size_t)l];
    ln.points = points[(size_t)l].data();
    ln.n_points = (int32_t)K;
    ln.beta0 = vector_arg(dict_get(spec, "beta0"), p, "beta0", keep);
    ln.row_weight = vector_arg(dict_get(spec, "row_weight"), n, "row_weight", keep);
    const py::object ne = dict_get(spec, "n_eff");
    ln.n_eff = ne.is_none() ? 0 : ne.cast<int64_t>();
    ks[(size_t)l] = K;
    total += K;
    if (reweighted) {
      const py::object rw = dict_get(spec, "reweight");
      if (rw.is_none()) throw py::value_error("lane " + std::to_string(l) + ": no re-weighting rule");
      const py::tuple t = rw.cast<py::tuple>();
      if (t.size() != 7) throw py::value_error("reweight = (coef_scale, group_scale, numerator, eps, tol, n_coef, n_group)");
      slm_reweight& r = rules[(size_t)l];
      r.coef_scale = t[0].cast<double>();
      r.n_coef = t[5].cast<int32_t>();
      r.n_group = t[6].cast<int32_t>();
      r.group_scale = vector_arg(t[1], r.n_group, "group_scale", keep);
      r.numerator = t[2].cast<double>();
      r.eps = t[3].cast<double>();
      r.tol = t[4].cast<double>();
    }
  }
  py::array betas = alloc(total * p).cast<py::array>();
  py::object gn_obj = py::none();
  double* gn_ptr = nullptr;
  if (want_gn) {
    py::array g = alloc(total * G).cast<py::array>();
    gn_ptr = static_cast<double*>(g.mutable_data());
    gn_obj = g;
  }
  py::array infos = info_bytes(total);
  auto* inf = static_cast<slm_point_info*>(infos.mutable_data());
  std::memset(inf, 0, sizeof(slm_point_info) * (size_t)total);
  double* bp = static_cast<double*>(betas.mutable_data());
  int64_t at = 0;
  for (int l = 0; l < nl; ++l) {
    lanes[(size_t)l].betas_out = bp + at * p;
    lanes[(size_t)l].group_norms_out = gn_ptr ? gn_ptr + at * G : nullptr;
    lanes[(size_t)l].infos = inf + at;
    at += ks[(size_t)l];
  }
  slm_solve_opts opts{tol, max_iter, check_every, L, flags};
  slm_solve_stats st;
  std::memset(&st, 0, sizeof(st));
  int rc;
  {
    py::gil_scoped_release nogil;
    rc = reweighted ? slm_solve_lanes_reweighted(reinterpret_cast<slm_dataset*>(ds), lanes.data(), rules.data(), nl, &opts, &st, rounds.data())
                    : slm_solve_lanes(reinterpret_cast<slm_dataset*>(ds), lanes.data(), nl, &opts, &st);
  }
  check(rc);
  py::list kl;
  for (int64_t k : ks) kl.append(k);
  if (!reweighted) return py::make_tuple(betas, gn_obj, infos, kl, stats_tuple(st));
  py::list rl;
  for (int32_t r : rounds) rl.append(r);
  return py::make_tuple(betas, gn_obj, infos, kl, stats_tuple(st), rl);
}

py::tuple solve_lanes(uintptr_t ds, const py::list& specs, int64_t n, int64_t p, int64_t G, double tol, int max_iter, int check_every,
                      double L, uint32_t flags, bool want_gn, bool extrapolate, const py::object& alloc) {
  return solve_lanes_any(ds, specs, n, p, G, tol, max_iter, check_every, L, flags, want_gn, extrapolate, alloc, false);
}

py::tuple solve_lanes_reweighted(uintptr_t ds, const py::list& specs, int64_t n, int64_t p, int64_t G, double tol, int max_iter,
                                 int check_every, double L, uint32_t flags, bool want_gn, const py::object& alloc) {
  return solve_lanes_any(ds, specs, n, p, G, tol, max_iter, check_every, L, flags, want_gn, false, alloc, true);
}

// slm_solve_path_lanes: one path walked by `n_lanes` lanes.  Returns (betas, group norms or None, records as bytes, stats).
py::tuple solve_path_lanes(uintptr_t ds, const py::object& points_in, int64_t p, int64_t G, const py::object& a, const py::object& b,
                           const py::object& d, const py::object& beta0, int n_lanes, double tol, int max_iter, int check_every, double L,
                           uint32_t flags, bool want_gn, bool extrapolate, const py::object& alloc) {
  arr_d pts = arr_d::ensure(points_in);
  if (!pts || pts.size() % 3 != 0 || pts.size() == 0) throw py::value_error("points must be (K, 3)");
  const int64_t K = pts.size() / 3;
  std::vector<double> gam((size_t)K, 0.0);
  if (extrapolate) extrapolation(pts.data(), K, gam.data());
  std::vector<slm_path_point> cp((size_t)K);
  for (int64_t k = 0; k < K; ++k) cp[(size_t)k] = slm_path_point{pts.data()[3 * k], pts.data()[3 * k + 1], pts.data()[3 * k + 2], gam[(size_t)k]};
  Keep keep;
  slm_penalty pen{vector_arg(a, p, "a", keep), vector_arg(b, G, "b", keep), vector_arg(d, G, "d", keep)};
  const double* b0 = vector_arg(beta0, p, "beta0", keep);
  py::array betas = alloc(K * p).cast<py::array>();
  py::object gn_obj = py::none();
  double* gn_ptr = nullptr;
  if (want_gn) {
    py::array g = alloc(K * G).cast<py::array>();
    gn_ptr = static_cast<double*>(g.mutable_data());
    gn_obj = g;
  }
  py::array infos = info_bytes(K);
  std::memset(infos.mutable_data(), 0, sizeof(slm_point_info) * (size_t)K);
  slm_solve_opts opts{tol, max_iter, check_every, L, flags};
  slm_solve_stats st;
  std::memset(&st, 0, sizeof(st));
  int rc;
  {
    py::gil_scoped_release nogil;
    rc = slm_solve_path_lanes(reinterpret_cast<slm_dataset*>(ds), &pen, cp.data(), (int32_t)K, n_lanes, &opts, b0,
                              static_cast<double*>(betas.mutable_data()), gn_ptr, static_cast<slm_point_info*>(infos.mutable_data()), &st);
  }
  check(rc);
  return py::make_tuple(betas, gn_obj, infos, stats_tuple(st));
}

// slm_dataset_create from numpy arrays of any layout (C- and F-contiguous matrices go as they are).  Returns the handle.
uintptr_t dataset_create(uintptr_t eng, const py::array& X_in, const py::object& y_in, const py::object& rw_in) {
  py::array X = X_in;
  if (X.ndim() != 2) throw py::value_error("X must be 2-D");
  const bool f64 = py::isinstance<py::array_t<double>>(X);
  const bool c_ok = (X.flags() & py::array::c_style) != 0, f_ok = (X.flags() & py::array::f_style) != 0;
  if (!f64 || !(c_ok || f_ok)) {
    X = arr_d::ensure(X_in);
    if (!X) throw py::value_error("X is not convertible to float64");
  }
  const int64_t n = X.shape(0), p = X.shape(1);
  const bool c_order = (X.flags() & py::array::c_style) != 0;
  Keep keep;
  const double* y = vector_arg(y_in, n, "y", keep);
  if (!y) throw py::value_error("y is None");
  const double* rw = vector_arg(rw_in, n, "row_weight", keep);
  slm_dataset* out = nullptr;
  int rc;
  {
    py::gil_scoped_release nogil;
    rc = slm_dataset_create(reinterpret_cast<slm_engine*>(eng), static_cast<const double*>(X.data()), n, p, c_order ? p : 1, c_order ? 1 : n, y,
                            rw, &out);
  }
  check(rc);
  return reinterpret_cast<uintptr_t>(out);
}

// ---- the exact search over supports: slm_solve_l0 and its eight relatives -------------------------------------------------
//
// Every wrapper's tuple ends with (record as bytes, status).  status is SLM_OK or SLM_ERR_NOT_CONVERGED (the result is not
// proven -- the node budget ran out, say: the outputs hold the incumbent); anything else raises.
using arr_u64 = py::array_t<uint64_t, py::array::c_style | py::array::forcecast>;

// The need masks: one word per group (the wide entries: n_groups x 2 words, the low one first), or None.
const uint64_t* need_words(const py::object& need, arr_u64& hold) {
  if (need.is_none()) return nullptr;
  hold = arr_u64::ensure(need);
  if (!hold) throw py::value_error("need is not convertible to uint64");
  return hold.data();
}

// One call: a zeroed record, the GIL released while call(record) runs, and the status checked as above.
template <class Call>
std::pair<py::array, int> l0_call(Call call) {
  py::array info = info_bytes(1);
  auto* rec = static_cast<slm_point_info*>(info.mutable_data());
  std::memset(rec, 0, sizeof(*rec));
  int rc;
  {
    py::gil_scoped_release nogil;
    rc = call(rec);
  }
  if (rc != SLM_ERR_NOT_CONVERGED) check(rc);
  return {info, rc};
}

// The four entries with slm_solve_l0's signature.  Returns (beta, support, lower bound, nodes, record, status); the support is
// an integer, wide: an array of two words (the low one first).
template <class Entry>
py::tuple l0_search(bool wide, Entry entry, uintptr_t ds, int64_t p, double alpha, int32_t max_groups, double eta, const py::object& T,
                    double big_M, const py::object& need, int64_t max_nodes) {
  Keep keep;
  const double* Tp = vector_arg(T, p * p, "T", keep);
  arr_u64 need_arr;
  const uint64_t* needp = need_words(need, need_arr);
  py::array_t<double> beta((py::ssize_t)p);
  py::array_t<uint64_t> support(2);
  double* bp = beta.mutable_data();
  uint64_t* sup = support.mutable_data();
  sup[0] = sup[1] = 0;
  double lower = 0.0;
  int64_t nodes = 0;
  const auto [info, rc] = l0_call([&](slm_point_info* rec) {
    return entry(reinterpret_cast<slm_dataset*>(ds), alpha, max_groups, eta, Tp, big_M, needp, max_nodes, bp, sup, &lower, &nodes, rec);
  });
  if (wide) return py::make_tuple(beta, support, lower, nodes, info, rc);
  return py::make_tuple(beta, sup[0], lower, nodes, info, rc);
}
template <bool XB>  // slm_solve_l0; XB: the same search with the exclusion bound
py::tuple solve_l0(uintptr_t ds, int64_t p, double alpha, int32_t max_groups, double eta, const py::object& T, double big_M,
                   const py::object& need, int64_t max_nodes) {
  return l0_search(false, [](auto... a) { return XB ? slm_solve_l0_xb(a...) : slm_solve_l0(a...); }, ds, p, alpha, max_groups, eta, T, big_M,
                   need, max_nodes);
}
template <bool XB>
py::tuple solve_l0_wide(uintptr_t ds, int64_t p, double alpha, int32_t max_groups, double eta, const py::object& T, double big_M,
                        const py::object& need, int64_t max_nodes) {
  return l0_search(true, [](auto... a) { return XB ? slm_solve_l0_xb_wide(a...) : slm_solve_l0_wide(a...); }, ds, p, alpha, max_groups, eta, T,
                   big_M, need, max_nodes);
}

// slm_solve_l0_l1: the same search in l1 mode (the reference's L1L0); the tuple of solve_l0.
py::tuple solve_l0_l1(uintptr_t ds, int64_t p, double alpha, double eta_l1, double big_M, const py::object& need, int64_t max_nodes) {
  arr_u64 need_arr;
  const uint64_t* needp = need_words(need, need_arr);
  py::array_t<double> beta((py::ssize_t)p);
  double* bp = beta.mutable_data();
  uint64_t support = 0;
  double lower = 0.0;
  int64_t nodes = 0;
  const auto [info, rc] = l0_call([&](slm_point_info* rec) {
    return slm_solve_l0_l1(reinterpret_cast<slm_dataset*>(ds), alpha, eta_l1, big_M, needp, max_nodes, bp, &support, &lower, &nodes, rec);
  });
  return py::make_tuple(beta, support, lower, nodes, info, rc);
}

// slm_solve_l0_constrained: the search under lo <= A beta <= hi and a per-column box.  Returns the tuple of solve_l0 with the
// rows' multipliers after the support.
py::tuple solve_l0_constrained(uintptr_t ds, int64_t p, double alpha, int32_t max_groups, double eta, const py::object& T, double big_M,
                               const py::object& need, int64_t max_nodes, const py::object& A, int32_t m, const py::object& lo,
                               const py::object& hi, const py::object& box_lo, const py::object& box_hi, int32_t max_qp_sweeps) {
  Keep keep;
  const double* Tp = vector_arg(T, p * p, "T", keep);
  const int64_t rows = m > 0 ? m : 0;
  const double* Ap = vector_arg(A, rows * p, "A", keep);
  const double* lop = vector_arg(lo, rows, "lo", keep);
  const double* hip = vector_arg(hi, rows, "hi", keep);
  const double* blop = vector_arg(box_lo, p, "box_lo", keep);
  const double* bhip = vector_arg(box_hi, p, "box_hi", keep);
  arr_u64 need_arr;
  const uint64_t* needp = need_words(need, need_arr);
  py::array_t<double> beta((py::ssize_t)p), lam((py::ssize_t)rows);
  double *bp = beta.mutable_data(), *lp = lam.mutable_data();
  uint64_t support = 0;
  double lower = 0.0;
  int64_t nodes = 0;
  const auto [info, rc] = l0_call([&](slm_point_info* rec) {
    return slm_solve_l0_constrained(reinterpret_cast<slm_dataset*>(ds), alpha, max_groups, eta, Tp, big_M, needp, max_nodes, Ap, m, lop, hip,
                                    blop, bhip, max_qp_sweeps, bp, &support, &lower, &nodes, lp, rec);
  });
  return py::make_tuple(beta, support, lam, lower, nodes, info, rc);
}

// The two profile entries: the best support of every size up to max_groups from one search.  Returns (coefficients
// [max_groups + 1][p], support masks [max_groups + 1] (wide: [max_groups + 1][2] words), values, nodes, record, status).
template <class Entry>
py::tuple l0_profile(bool wide, Entry entry, uintptr_t ds, int64_t p, double alpha_min, int32_t max_groups, double eta, const py::object& T,
                     double big_M, const py::object& need, int64_t max_nodes) {
  if (max_groups < 0) throw py::value_error("max_groups must be >= 0");
  Keep keep;
  const double* Tp = vector_arg(T, p * p, "T", keep);
  arr_u64 need_arr;
  const uint64_t* needp = need_words(need, need_arr);
  const py::ssize_t rows = (py::ssize_t)max_groups + 1;
  py::array_t<double> beta({rows, (py::ssize_t)p}), value(rows);
  py::array_t<uint64_t> support = wide ? py::array_t<uint64_t>({rows, (py::ssize_t)2}) : py::array_t<uint64_t>(rows);
  double *bp = beta.mutable_data(), *vp = value.mutable_data();
  uint64_t* sup = support.mutable_data();
  int64_t nodes = 0;
  const auto [info, rc] = l0_call([&](slm_point_info* rec) {
    return entry(reinterpret_cast<slm_dataset*>(ds), alpha_min, max_groups, eta, Tp, big_M, needp, max_nodes, bp, sup, vp, &nodes, rec);
  });
  return py::make_tuple(beta, support, value, nodes, info, rc);
}
py::tuple solve_l0_profile(uintptr_t ds, int64_t p, double alpha_min, int32_t max_groups, double eta, const py::object& T, double big_M,
                           const py::object& need, int64_t max_nodes) {
  return l0_profile(false, [](auto... a) { return slm_solve_l0_profile(a...); }, ds, p, alpha_min, max_groups, eta, T, big_M, need, max_nodes);
}
py::tuple solve_l0_profile_wide(uintptr_t ds, int64_t p, double alpha_min, int32_t max_groups, double eta, const py::object& T,
                                double big_M, const py::object& need, int64_t max_nodes) {
  return l0_profile(true, [](auto... a) { return slm_solve_l0_profile_wide(a...); }, ds, p, alpha_min, max_groups, eta, T, big_M, need,
                    max_nodes);
}
// The two l1 profile entries (L1L0 at every alpha from one search): no ridge term and no T, so the helper's eta carries eta_l1 and
// its T stays None.  The tuple of solve_l0_profile / solve_l0_profile_wide.
py::tuple solve_l0_l1_profile(uintptr_t ds, int64_t p, double alpha_min, int32_t max_groups, double eta_l1, double big_M,
                              const py::object& need, int64_t max_nodes) {
  return l0_profile(false, [](slm_dataset* d, double am, int32_t K, double e1, const double*, auto... a) {
    return slm_solve_l0_l1_profile(d, am, K, e1, a...);
  }, ds, p, alpha_min, max_groups, eta_l1, py::none(), big_M, need, max_nodes);
}
py::tuple solve_l0_l1_profile_wide(uintptr_t ds, int64_t p, double alpha_min, int32_t max_groups, double eta_l1, double big_M,
                                   const py::object& need, int64_t max_nodes) {
  return l0_profile(true, [](slm_dataset* d, double am, int32_t K, double e1, const double*, auto... a) {
    return slm_solve_l0_l1_profile_wide(d, am, K, e1, a...);
  }, ds, p, alpha_min, max_groups, eta_l1, py::none(), big_M, need, max_nodes);
}

// slm_solve_l0_profile_batch: the profiles of several row sets of one dataset from one launch.  row_weights: a sequence of
// arrays of n weights or None; n_effs: as many integers.  Returns (coefficients [count][max_groups + 1][ps], intercepts
// [count][max_groups + 1], support masks, values, nodes [count], records as bytes, status); ps = p - 1 with an intercept.
// etas == nullptr: that entry, with its one ridge eta.  Otherwise slm_solve_l0_profile_grid: n_eta weights of kind eta_kind per row
// set, every output's leading dimension count * n_eta (problem r * n_eta + e: row set r with etas[e]).
py::tuple l0_profile_rows(uintptr_t ds, int64_t p, int64_t n, const py::sequence& row_weights, const py::sequence& n_effs, bool intercept,
                          const arr_d* etas, int32_t eta_kind, double alpha_min, int32_t max_groups, double eta, const py::object& T,
                          double big_M, const py::object& need, int64_t max_nodes) {
  if (max_groups < 0) throw py::value_error("max_groups must be >= 0");
  const py::ssize_t count = (py::ssize_t)py::len(row_weights);
  const py::ssize_t n_eta = etas ? (py::ssize_t)etas->size() : 1;
  if ((py::ssize_t)py::len(n_effs) != count) throw py::value_error("row_weights and n_effs differ in length");
  const int64_t ps = intercept && p > 0 ? p - 1 : p;
  Keep keep;
  const double* Tp = vector_arg(T, ps * ps, "T", keep);
  arr_u64 need_arr;
  const uint64_t* needp = need_words(need, need_arr);
  std::vector<const double*> wp((size_t)count);
  std::vector<int64_t> ne((size_t)count);
  for (py::ssize_t b = 0; b < count; ++b) {
    wp[(size_t)b] = vector_arg(row_weights[b], n, "row_weights", keep);
    ne[(size_t)b] = n_effs[b].cast<int64_t>();
  }
  // (count 0, no eta, more problems than any call takes: the engine refuses them, the outputs only have to exist)
  const py::ssize_t rows = (py::ssize_t)max_groups + 1;
  const py::ssize_t cnt = count > 0 && n_eta > 0 && count * n_eta <= 4 * SLM_L0_GRID_MAX ? count * n_eta : 1;
  py::array_t<double> beta({cnt, rows, (py::ssize_t)ps}), icpt({cnt, rows}), value({cnt, rows});
  py::array_t<uint64_t> support({cnt, rows});
  py::array_t<int64_t> nodes(cnt);
  double *bp = beta.mutable_data(), *ip = icpt.mutable_data(), *vp = value.mutable_data();
  uint64_t* sup = support.mutable_data();
  int64_t* np_ = nodes.mutable_data();
  py::array info = info_bytes(cnt);
  auto* rec = static_cast<slm_point_info*>(info.mutable_data());
  std::memset(rec, 0, sizeof(*rec) * (size_t)cnt);
  int rc;
  {
    py::gil_scoped_release nogil;
    if (etas)
      rc = slm_solve_l0_profile_grid(reinterpret_cast<slm_dataset*>(ds), (int32_t)count, wp.data(), ne.data(), intercept ? 1 : 0, (int32_t)n_eta,
                                     etas->data(), eta_kind, alpha_min, max_groups, Tp, big_M, needp, max_nodes, bp, ip, sup, vp, np_, rec);
    else
      rc = slm_solve_l0_profile_batch(reinterpret_cast<slm_dataset*>(ds), (int32_t)count, wp.data(), ne.data(), intercept ? 1 : 0, alpha_min,
                                      max_groups, eta, Tp, big_M, needp, max_nodes, bp, ip, sup, vp, np_, rec);
  }
  if (rc != SLM_ERR_NOT_CONVERGED) check(rc);
  return py::make_tuple(beta, icpt, support, value, nodes, info, rc);
}
py::tuple solve_l0_profile_batch(uintptr_t ds, int64_t p, int64_t n, const py::sequence& row_weights, const py::sequence& n_effs,
                                 bool intercept, double alpha_min, int32_t max_groups, double eta, const py::object& T, double big_M,
                                 const py::object& need, int64_t max_nodes) {
  return l0_profile_rows(ds, p, n, row_weights, n_effs, intercept, nullptr, 0, alpha_min, max_groups, eta, T, big_M, need, max_nodes);
}
// slm_solve_l0_profile_grid: the tuple of solve_l0_profile_batch with count * n_eta problems.
py::tuple solve_l0_profile_grid(uintptr_t ds, int64_t p, int64_t n, const py::sequence& row_weights, const py::sequence& n_effs,
                                bool intercept, const arr_d& etas, int32_t eta_kind, double alpha_min, int32_t max_groups,
                                const py::object& T, double big_M, const py::object& need, int64_t max_nodes) {
  return l0_profile_rows(ds, p, n, row_weights, n_effs, intercept, &etas, eta_kind, alpha_min, max_groups, 0.0, T, big_M, need, max_nodes);
}

// slm_solve_l0_local / slm_solve_l0_local_descent: the local search over n_cells cells from n_starts starts each.  starts: None
// (the zero start) or n_cells * n_starts * p doubles.  Returns (coefficients [n_cells][p], objectives [n_cells], winning starts
// [n_cells], records as bytes, status).
template <bool SWAPS>
py::tuple solve_l0_local(uintptr_t ds, int64_t p, int32_t n_cells, const arr_d& alphas, const arr_d& etas, double big_M, int32_t n_starts,
                         const py::object& starts) {
  const int64_t cells = n_cells > 0 ? n_cells : 0;
  if ((int64_t)alphas.size() < cells || (int64_t)etas.size() < cells) throw py::value_error("alphas and etas must have n_cells entries");
  // (no cell, more problems than any call takes: the engine refuses them, the outputs only have to exist)
  const bool sized = n_cells >= 1 && n_starts >= 1 && (int64_t)n_cells * n_starts <= SLM_L0_LOCAL_MAX_PROBLEMS;
  Keep keep;
  const double* sp = sized ? vector_arg(starts, (int64_t)n_cells * n_starts * p, "starts", keep) : nullptr;
  const py::ssize_t cnt = sized ? n_cells : 1;
  py::array_t<double> beta({cnt, (py::ssize_t)p}), objective(cnt);
  py::array_t<int32_t> winner(cnt);
  py::array info = info_bytes(cnt);
  auto* rec = static_cast<slm_point_info*>(info.mutable_data());
  std::memset(rec, 0, sizeof(*rec) * (size_t)cnt);
  double *bp = beta.mutable_data(), *op = objective.mutable_data();
  int32_t* wp = winner.mutable_data();
  std::memset(wp, 0, sizeof(int32_t) * (size_t)cnt);
  int rc;
  {
    py::gil_scoped_release nogil;
    auto* d = reinterpret_cast<slm_dataset*>(ds);
    rc = SWAPS ? slm_solve_l0_local(d, n_cells, alphas.data(), etas.data(), big_M, n_starts, sp, bp, op, wp, rec)
               : slm_solve_l0_local_descent(d, n_cells, alphas.data(), etas.data(), big_M, n_starts, sp, bp, op, wp, rec);
  }
  if (rc != SLM_ERR_NOT_CONVERGED) check(rc);
  return py::make_tuple(beta, objective, winner, info, rc);
}

// slm_solve_l0_local_bound: the proven lower bound of every cell.  starts: None (zero) or n_cells * p doubles.  Returns (bounds
// [n_cells], relaxed objectives [n_cells], u [n_cells][p], (sweeps, status word) [n_cells][2], records as bytes, status).
py::tuple solve_l0_local_bound(uintptr_t ds, int64_t p, int32_t n_cells, const arr_d& alphas, const arr_d& etas, double big_M,
                               const py::object& starts, int32_t max_sweeps, double gap_tol) {
  const int64_t cells = n_cells > 0 ? n_cells : 0;
  if ((int64_t)alphas.size() < cells || (int64_t)etas.size() < cells) throw py::value_error("alphas and etas must have n_cells entries");
  // (no cell, more cells than any call takes: the engine refuses them, the outputs only have to exist)
  const bool sized = n_cells >= 1 && n_cells <= SLM_L0_LOCAL_MAX_PROBLEMS;
  Keep keep;
  const double* sp = sized ? vector_arg(starts, (int64_t)n_cells * p, "starts", keep) : nullptr;
  const py::ssize_t cnt = sized ? n_cells : 1;
  py::array_t<double> lower(cnt), primal(cnt), u({cnt, (py::ssize_t)p});
  py::array_t<int32_t> stats({cnt, (py::ssize_t)2});
  py::array info = info_bytes(cnt);
  auto* rec = static_cast<slm_point_info*>(info.mutable_data());
  std::memset(rec, 0, sizeof(*rec) * (size_t)cnt);
  double *lp = lower.mutable_data(), *pp = primal.mutable_data(), *up = u.mutable_data();
  int32_t* tp = stats.mutable_data();
  std::memset(lp, 0, sizeof(double) * (size_t)cnt);
  std::memset(pp, 0, sizeof(double) * (size_t)cnt);
  std::memset(up, 0, sizeof(double) * (size_t)cnt * (size_t)p);
  std::memset(tp, 0, sizeof(int32_t) * 2 * (size_t)cnt);
  int rc;
  {
    py::gil_scoped_release nogil;
    rc = slm_solve_l0_local_bound(reinterpret_cast<slm_dataset*>(ds), n_cells, alphas.data(), etas.data(), big_M, sp, max_sweeps, gap_tol, lp,
                                  pp, up, tp, rec);
  }
  if (rc != SLM_ERR_NOT_CONVERGED) check(rc);
  return py::make_tuple(lower, primal, u, stats, info, rc);
}

// slm_solve_l0_local_folds: the local search on several row sets of one dataset from one launch.  row_weights: a sequence of
// arrays of n weights or None; n_effs: as many integers.  starts: None or count * n_cells * n_starts * ps doubles.  Returns
// (coefficients [count * n_cells][ps], intercepts, objectives, winning starts [count * n_cells], the four status words of every
// problem [count * n_cells * n_starts][4], records as bytes, status); ps = p - 1 with an intercept.
//
// slm_solve_l0_local_subsets: the same tuple from the cardinality rule -- `sizes` (int32) where the alphas are, six status
// words per problem.  One body serves both: `sizes` NULL is the penalised entry.
py::tuple l0_local_rows(uintptr_t ds, int64_t p, int64_t n, const py::sequence& row_weights, const py::sequence& n_effs, bool intercept,
                        int32_t n_cells, const double* alphas, const int32_t* sizes, const arr_d& etas, double big_M, int32_t n_starts,
                        const py::object& starts, bool swaps) {
  const py::ssize_t count = (py::ssize_t)py::len(row_weights);
  if ((py::ssize_t)py::len(n_effs) != count) throw py::value_error("row_weights and n_effs differ in length");
  const int64_t cells = n_cells > 0 ? n_cells : 0;
  if ((int64_t)etas.size() < cells) throw py::value_error("etas must have n_cells entries");
  const py::ssize_t nstat = sizes ? 6 : 4;
  const int64_t ps = intercept && p > 0 ? p - 1 : p;
  // (no row set, no cell, more problems than any call takes: the engine refuses them, the outputs only have to exist)
  const bool sized = count >= 1 && count <= 16 && n_cells >= 1 && n_starts >= 1 && (int64_t)n_cells * n_starts <= SLM_L0_LOCAL_MAX_PROBLEMS &&
                     (int64_t)count * n_cells * n_starts <= SLM_L0_LOCAL_MAX_PROBLEMS;
  Keep keep;
  const double* sp = sized ? vector_arg(starts, (int64_t)count * n_cells * n_starts * ps, "starts", keep) : nullptr;
  std::vector<const double*> wp((size_t)count);
  std::vector<int64_t> ne((size_t)count);
  for (py::ssize_t b = 0; b < count; ++b) {
    wp[(size_t)b] = vector_arg(row_weights[b], n, "row_weights", keep);
    ne[(size_t)b] = n_effs[b].cast<int64_t>();
  }
  const py::ssize_t cnt = sized ? count * n_cells : 1, problems = sized ? cnt * n_starts : 1;
  py::array_t<double> beta({cnt, (py::ssize_t)ps}), icpt(cnt), objective(cnt);
  py::array_t<int32_t> winner(cnt), stats({problems, nstat});
  py::array info = info_bytes(cnt);
  auto* rec = static_cast<slm_point_info*>(info.mutable_data());
  std::memset(rec, 0, sizeof(*rec) * (size_t)cnt);
  double *bp = beta.mutable_data(), *ip = icpt.mutable_data(), *op = objective.mutable_data();
  int32_t *wn = winner.mutable_data(), *tp = stats.mutable_data();
  std::memset(wn, 0, sizeof(int32_t) * (size_t)cnt);
  std::memset(tp, 0, sizeof(int32_t) * (size_t)nstat * (size_t)problems);
  int rc;
  {
    py::gil_scoped_release nogil;
    auto* d = reinterpret_cast<slm_dataset*>(ds);
    rc = sizes ? slm_solve_l0_local_subsets(d, (int32_t)count, wp.data(), ne.data(), intercept ? 1 : 0, n_cells, sizes, etas.data(), big_M,
                                            n_starts, sp, swaps ? 1 : 0, bp, ip, op, wn, tp, rec)
               : slm_solve_l0_local_folds(d, (int32_t)count, wp.data(), ne.data(), intercept ? 1 : 0, n_cells, alphas, etas.data(), big_M,
                                          n_starts, sp, swaps ? 1 : 0, bp, ip, op, wn, tp, rec);
  }
  if (rc != SLM_ERR_NOT_CONVERGED) check(rc);
  return py::make_tuple(beta, icpt, objective, winner, stats, info, rc);
}
py::tuple solve_l0_local_folds(uintptr_t ds, int64_t p, int64_t n, const py::sequence& row_weights, const py::sequence& n_effs, bool intercept,
                               int32_t n_cells, const arr_d& alphas, const arr_d& etas, double big_M, int32_t n_starts,
                               const py::object& starts, bool swaps) {
  if ((int64_t)alphas.size() < (n_cells > 0 ? n_cells : 0)) throw py::value_error("alphas and etas must have n_cells entries");
  return l0_local_rows(ds, p, n, row_weights, n_effs, intercept, n_cells, alphas.data(), nullptr, etas, big_M, n_starts, starts, swaps);
}
py::tuple solve_l0_local_subsets(uintptr_t ds, int64_t p, int64_t n, const py::sequence& row_weights, const py::sequence& n_effs, bool intercept,
                                 int32_t n_cells, const py::array_t<int32_t, py::array::c_style | py::array::forcecast>& sizes,
                                 const arr_d& etas, double big_M, int32_t n_starts, const py::object& starts, bool swaps) {
  if ((int64_t)sizes.size() < (n_cells > 0 ? n_cells : 0)) throw py::value_error("sizes and etas must have n_cells entries");
  return l0_local_rows(ds, p, n, row_weights, n_effs, intercept, n_cells, nullptr, sizes.data(), etas, big_M, n_starts, starts, swaps);
}

// slm_solve_l0_local_l1: the local search with an l1 term -- the tuple of solve_l0_local_folds; `l1s` beside the alphas, `ridges`
// an array or None (NULL: no ridge).
py::tuple solve_l0_local_l1(uintptr_t ds, int64_t p, int64_t n, const py::sequence& row_weights, const py::sequence& n_effs, bool intercept,
                            int32_t n_cells, const arr_d& alphas, const arr_d& l1s, const py::object& ridges, double big_M, int32_t n_starts,
                            const py::object& starts, bool swaps) {
  const py::ssize_t count = (py::ssize_t)py::len(row_weights);
  if ((py::ssize_t)py::len(n_effs) != count) throw py::value_error("row_weights and n_effs differ in length");
  const int64_t cells = n_cells > 0 ? n_cells : 0;
  if ((int64_t)alphas.size() < cells || (int64_t)l1s.size() < cells) throw py::value_error("alphas, l1s and ridges must have n_cells entries");
  const int64_t ps = intercept && p > 0 ? p - 1 : p;
  // (no row set, no cell, more problems than any call takes: the engine refuses them, the outputs only have to exist)
  const bool sized = count >= 1 && count <= 16 && n_cells >= 1 && n_starts >= 1 && (int64_t)n_cells * n_starts <= SLM_L0_LOCAL_MAX_PROBLEMS &&
                     (int64_t)count * n_cells * n_starts <= SLM_L0_LOCAL_MAX_PROBLEMS;
  Keep keep;
  const arr_d rd = ridges.is_none() ? arr_d() : arr_d::ensure(ridges);  // (at least n_cells entries, as the alphas: the engine reads that many)
  if (!ridges.is_none() && (!rd || (int64_t)rd.size() < cells)) throw py::value_error("alphas, l1s and ridges must have n_cells entries");
  const double* rp = ridges.is_none() ? nullptr : rd.data();
  const double* sp = sized ? vector_arg(starts, (int64_t)count * n_cells * n_starts * ps, "starts", keep) : nullptr;
  std::vector<const double*> wp((size_t)count);
  std::vector<int64_t> ne((size_t)count);
  for (py::ssize_t b = 0; b < count; ++b) {
    wp[(size_t)b] = vector_arg(row_weights[b], n, "row_weights", keep);
    ne[(size_t)b] = n_effs[b].cast<int64_t>();
  }
  const py::ssize_t cnt = sized ? count * n_cells : 1, problems = sized ? cnt * n_starts : 1;
  py::array_t<double> beta({cnt, (py::ssize_t)ps}), icpt(cnt), objective(cnt);
  py::array_t<int32_t> winner(cnt), stats({problems, (py::ssize_t)4});
  py::array info = info_bytes(cnt);
  auto* rec = static_cast<slm_point_info*>(info.mutable_data());
  std::memset(rec, 0, sizeof(*rec) * (size_t)cnt);
  double *bp = beta.mutable_data(), *ip = icpt.mutable_data(), *op = objective.mutable_data();
  int32_t *wn = winner.mutable_data(), *tp = stats.mutable_data();
  std::memset(wn, 0, sizeof(int32_t) * (size_t)cnt);
  std::memset(tp, 0, sizeof(int32_t) * 4 * (size_t)problems);
  int rc;
  {
    py::gil_scoped_release nogil;
    auto* d = reinterpret_cast<slm_dataset*>(ds);
    rc = slm_solve_l0_local_l1(d, (int32_t)count, wp.data(), ne.data(), intercept ? 1 : 0, n_cells, alphas.data(), l1s.data(), rp, big_M,
                               n_starts, sp, swaps ? 1 : 0, bp, ip, op, wn, tp, rec);
  }
  if (rc != SLM_ERR_NOT_CONVERGED) check(rc);
  return py::make_tuple(beta, icpt, objective, winner, stats, info, rc);
}

// slm_solve_l0_local_groups: the local search with groups and a hierarchy.  need_ptr / need_idx: None or int32 arrays (need_ptr
// with one entry per search group and one more: checked by the caller, sparselm_amd/_engine.py).  Returns (coefficients
// [count * n_cells][ps], intercepts, objectives, winning starts, cl(S) [count * n_cells][search groups], the six status words
// of every problem, records as bytes, status).
py::tuple solve_l0_local_groups(uintptr_t ds, int64_t p, int64_t n, int64_t n_groups, const py::sequence& row_weights,
                                const py::sequence& n_effs, bool intercept, int32_t n_cells, const arr_d& alphas, const arr_d& etas,
                                double big_M, const py::object& need_ptr, const py::object& need_idx, int32_t n_starts,
                                const py::object& starts, bool swaps) {
  using arr_i = py::array_t<int32_t, py::array::c_style | py::array::forcecast>;
  const py::ssize_t count = (py::ssize_t)py::len(row_weights);
  if ((py::ssize_t)py::len(n_effs) != count) throw py::value_error("row_weights and n_effs differ in length");
  const int64_t cells = n_cells > 0 ? n_cells : 0;
  if ((int64_t)alphas.size() < cells || (int64_t)etas.size() < cells) throw py::value_error("alphas and etas must have n_cells entries");
  const int64_t drop = intercept ? 1 : 0, ps = p > drop ? p - drop : 0, gs = n_groups > drop ? n_groups - drop : 0;
  arr_i ptr_a, idx_a;
  const int32_t *pp = nullptr, *ip = nullptr;
  if (!need_ptr.is_none()) {
    ptr_a = arr_i::ensure(need_ptr);
    if (!ptr_a || (int64_t)ptr_a.size() != gs + 1) throw py::value_error("need_ptr must have one entry per search group and one more");
    pp = ptr_a.data();
  }
  if (!need_idx.is_none()) {
    idx_a = arr_i::ensure(need_idx);
    if (!idx_a) throw py::value_error("need_idx is not convertible to int32");
    for (int64_t g = 0; pp && g <= gs; ++g)
      if ((int64_t)pp[g] > (int64_t)idx_a.size()) throw py::value_error("need_idx is shorter than need_ptr says");
    ip = idx_a.data();
  }
  // (no row set, no cell, more problems than any call takes: the engine refuses them, the outputs only have to exist)
  const bool sized = count >= 1 && count <= 16 && n_cells >= 1 && n_starts >= 1 && (int64_t)n_cells * n_starts <= SLM_L0_LOCAL_MAX_PROBLEMS &&
                     (int64_t)count * n_cells * n_starts <= SLM_L0_LOCAL_MAX_PROBLEMS;
  Keep keep;
  const double* sp = sized ? vector_arg(starts, (int64_t)count * n_cells * n_starts * ps, "starts", keep) : nullptr;
  std::vector<const double*> wp((size_t)count);
  std::vector<int64_t> ne((size_t)count);
  for (py::ssize_t b = 0; b < count; ++b) {
    wp[(size_t)b] = vector_arg(row_weights[b], n, "row_weights", keep);
    ne[(size_t)b] = n_effs[b].cast<int64_t>();
  }
  const py::ssize_t cnt = sized ? count * n_cells : 1, problems = sized ? cnt * n_starts : 1, gw = gs > 0 ? (py::ssize_t)gs : 1;
  py::array_t<double> beta({cnt, (py::ssize_t)ps}), icpt(cnt), objective(cnt);
  py::array_t<int32_t> winner(cnt), gsup({cnt, gw}), stats({problems, (py::ssize_t)6});
  py::array info = info_bytes(cnt);
  auto* rec = static_cast<slm_point_info*>(info.mutable_data());
  std::memset(rec, 0, sizeof(*rec) * (size_t)cnt);
  double *bp = beta.mutable_data(), *cp = icpt.mutable_data(), *op = objective.mutable_data();
  int32_t *wn = winner.mutable_data(), *gp = gsup.mutable_data(), *tp = stats.mutable_data();
  std::memset(wn, 0, sizeof(int32_t) * (size_t)cnt);
  std::memset(gp, 0, sizeof(int32_t) * (size_t)cnt * (size_t)gw);
  std::memset(tp, 0, sizeof(int32_t) * 6 * (size_t)problems);
  int rc;
  {
    py::gil_scoped_release nogil;
    auto* d = reinterpret_cast<slm_dataset*>(ds);
    rc = slm_solve_l0_local_groups(d, (int32_t)count, wp.data(), ne.data(), intercept ? 1 : 0, n_cells, alphas.data(), etas.data(), big_M, pp, ip,
                                   n_starts, sp, swaps ? 1 : 0, bp, cp, op, wn, gp, tp, rec);
  }
  if (rc != SLM_ERR_NOT_CONVERGED) check(rc);
  return py::make_tuple(beta, icpt, objective, winner, gsup, stats, info, rc);
}

}  // namespace

PYBIND11_MODULE(_slm_binding, m) {
  m.doc() = "compiled binding of the hot calls of libslm_hip.so (include/slm_engine.h)";
  m.def("set_error_types", [](py::object engine_error, py::object nonfinite_error) {
    g_engine_error = std::move(engine_error);
    g_nonfinite_error = std::move(nonfinite_error);
  });
  m.def("abi_version", []() { return slm_abi_version(); });
  m.def("info_record_bytes", []() { return (int)sizeof(slm_point_info); });
  m.def("solve_lanes", &solve_lanes);
  m.def("solve_lanes_reweighted", &solve_lanes_reweighted);
  m.def("solve_path_lanes", &solve_path_lanes);
  m.def("dataset_create", &dataset_create);
  m.def("solve_l0", &solve_l0<false>);
  m.def("solve_l0_xb", &solve_l0<true>);
  m.def("solve_l0_l1", &solve_l0_l1);
  m.def("solve_l0_constrained", &solve_l0_constrained);
  m.def("solve_l0_profile", &solve_l0_profile);
  m.def("solve_l0_wide", &solve_l0_wide<false>);
  m.def("solve_l0_xb_wide", &solve_l0_wide<true>);
  m.def("solve_l0_profile_wide", &solve_l0_profile_wide);
  m.def("solve_l0_profile_batch", &solve_l0_profile_batch);
  m.def("solve_l0_profile_grid", &solve_l0_profile_grid);
  m.def("solve_l0_l1_profile", &solve_l0_l1_profile);
  m.def("solve_l0_l1_profile_wide", &solve_l0_l1_profile_wide);
  m.def("solve_l0_local", &solve_l0_local<true>);
  m.def("solve_l0_local_descent", &solve_l0_local<false>);
  m.def("solve_l0_local_folds", &solve_l0_local_folds);
  m.def("solve_l0_local_subsets", &solve_l0_local_subsets);
  m.def("solve_l0_local_groups", &solve_l0_local_groups);
  m.def("solve_l0_local_l1", &solve_l0_local_l1);
  m.def("solve_l0_local_bound", &solve_l0_local_bound);
  m.def("path_extrapolation", [](const arr_d& pts) {
    if (pts.size() % 3 != 0) throw py::value_error("points must be (K, 3)");
    const int64_t K = pts.size() / 3;
    py::array_t<double> out((py::ssize_t)K);
    extrapolation(pts.data(), K, out.mutable_data());
    return out;
  });
  // (the module's globals are Python objects: dropped while the interpreter is still up)
  auto cleanup = []() {
    g_engine_error = py::object();
    g_nonfinite_error = py::object();
  };
  py::module_::import("atexit").attr("register")(py::cpp_function(cleanup));
}
