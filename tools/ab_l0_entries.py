"""A/B of two builds of the engine on the eight exact-l0 entries and the four local-search entries (csrc/engine_l0.hip): child processes that load the library
named by SLM_HIP_LIBRARY (every call then goes through ctypes), in the order given, each under its own time limit; the run
stops at the first child that does not exit cleanly.  Results only (timing: tools/l0_timing.py).

Cases: the smallest shapes at which the host side of a call can go wrong, from the builders of the l0 GPU tests -- the
12-column designs at n = 40 and n = 10, 20 singleton groups (past the ticket prefix), grouped columns under a hierarchy, a
binding box, a ridge term with a Tikhonov matrix, the l1 mode, the profile below and above the group count, the wide search at
80 singletons with a hierarchy across bit 64, the wide capacity case, the constrained search with no row, one row and an
infeasible row, both exclusion-bound entries where the bound runs and where it falls back, and one refused call per entry.

Compared bit for bit between the first library and the others: coefficients, supports, values, multipliers, lower bound, the
status, and every field of the info record -- except ``nodes``, and ``rejects`` where it counts descents or qp solves: those
depend on which wave found an incumbent first and are printed.  Of a call under a node budget of one batch only the return
code and the status are compared: its incumbent depends on timing.

The local search (slm_solve_l0_local, _descent, _folds, _subsets): p in {5, 64, 65, 130} at n = 40, 3 cells x 2 starts with
explicit starts and with none, swaps on and off, one NULL row set and three (two weighted, one NULL), intercept on and off,
sizes {1, 3, p}, one cell whose alpha leaves the winner empty, and one refused call per refusal kind of l0_ls_check,
l0_lsf_check and l0_lc_check.  Every output array, every field of every record and every raised message is compared: one wave
owns one problem, so nothing varies between two runs.  Of a call on data with a NaN the exception's type is compared and its
message printed (the single-set entry names X^T y where it named the Gram).

usage: ab_l0_entries.py libA.so libB.so [...] [--out FILE]     (name the first library twice to see that the comparison is stable)"""
import os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

CHILD = r'''
import os, sys, warnings
import numpy as np
ROOT, out_path = sys.argv[1], sys.argv[2]
sys.path[:0] = [ROOT, os.path.join(ROOT, "sparse-lm_amd"), os.path.join(ROOT, "tests")]
warnings.simplefilter("ignore")
from sparselm_amd import _engine
from test_l0_gpu import draw
from test_l0_search_gpu import suppressor
from test_l0_wide_gpu import ten_groups_of_eight
eng = _engine.get_engine(0)
out, records = {}, []

_call = _engine.Dataset._l0_call
def spy(self, *a, **k):  # the raw record of every call, beside what the method makes of it
    res = _call(self, *a, **k)
    records.append(res[1].copy())
    return res
_engine.Dataset._l0_call = spy

def words(v):  # a support of up to 128 bits
    return np.array([int(v) & (2 ** 64 - 1), int(v) >> 64], dtype=np.uint64)

def keep(tag, fn, timing=(), budget=False):
    """timing: the record fields that may differ between two runs of one build"""
    del records[:]
    try:
        res = fn()
    except Exception as exc:
        out[tag + "/raised"] = np.array(f"{type(exc).__name__}: {exc}")
        return
    info = res[-1]
    out[tag + "/status"] = np.array(f"{info['status']} proven={info['proven_optimal']} rc_ok={int(records[-1]['status']) == 0}")
    out[tag + "/print/nodes"] = np.array(info["nodes"])
    if budget:
        return
    for i, v in enumerate(res[:-1]):
        if isinstance(v, np.ndarray):
            out[f"{tag}/out{i}"] = v
        elif isinstance(v, list):
            out[f"{tag}/out{i}"] = np.stack([words(s) for s in v])
        else:
            out[f"{tag}/out{i}"] = words(v)
    if "lower_bound" in info:
        out[tag + "/lower_bound"] = np.array(info["lower_bound"])
    rec = records[-1]
    for name in rec.dtype.names:
        out[f"{tag}/{'print' if name in timing else 'rec'}/{name}"] = np.array(rec[name])

def refused(tag, fn):
    keep(tag + "/refused", fn)
    assert tag + "/refused/raised" in out, tag

COUNTS = ("rejects",)  # narrow, l1 and constrained: descents / qp solves
for n in (40, 10):
    X, y = draw(n)
    var = float(np.var(y))
    with eng.dataset(X, y) as ds:
        keep(f"l0_n{n}_K4", lambda: ds.solve_l0(max_groups=4, big_M=1000.0), COUNTS)
        keep(f"l0_n{n}_alpha", lambda: ds.solve_l0(alpha=0.01 * var, big_M=1000.0), COUNTS)
        keep(f"wide_n{n}_K4", lambda: ds.solve_l0_wide(max_groups=4, big_M=1000.0))
        keep(f"profile_n{n}_5", lambda: ds.solve_l0_profile(max_groups=5, big_M=1000.0))
        keep(f"profile_n{n}_15", lambda: ds.solve_l0_profile(max_groups=15, alpha_min=1e-3 * var, big_M=1000.0))  # above the 12 groups
        keep(f"profile_wide_n{n}_5", lambda: ds.solve_l0_profile_wide(max_groups=5, big_M=1000.0))
        # the exclusion bound: runs at n = 40 (mode 5), falls back at n = 10 (n < p, no ridge term: mode 6)
        keep(f"xb_n{n}", lambda: ds.solve_l0_xb(max_groups=4, big_M=1000.0), COUNTS)
        keep(f"xb_wide_n{n}", lambda: ds.solve_l0_xb_wide(max_groups=4, big_M=1000.0))
        assert int(out[f"xb_n{n}/rec/mode"]) == int(out[f"xb_wide_n{n}/rec/mode"]) == (5 if n == 40 else 6)
X, y = draw(40)
var, cinf = float(np.var(y)), float(np.max(np.abs(X.T @ y / len(y))))
W = np.random.default_rng(5).standard_normal((12, 12))
with eng.dataset(X, y) as ds:
    keep("box_binds", lambda: ds.solve_l0(max_groups=4, big_M=5.0), COUNTS)
    assert np.max(np.abs(out["box_binds/out0"])) == 5.0
    keep("ridge_T", lambda: ds.solve_l0(alpha=0.01 * var, eta=0.5, T=W.T @ W, big_M=1000.0), COUNTS)
    keep("l1", lambda: ds.solve_l0_l1(alpha=0.01 * var, eta_l1=0.05 * cinf, big_M=1000.0), COUNTS)
    ones = np.ones((1, 12))
    keep("con_m0", lambda: ds.solve_l0_constrained(np.zeros((0, 12)), [], [], max_groups=4, big_M=100.0), COUNTS)
    keep("con_m1", lambda: ds.solve_l0_constrained(ones, -np.inf, 10.0, max_groups=4, big_M=100.0), COUNTS)
    keep("con_box", lambda: ds.solve_l0_constrained(ones, -np.inf, 10.0, alpha=0.01 * var, eta=0.1, big_M=100.0, box_lo=0.0), COUNTS)
    # two columns forced away from zero, one slot: no admissible support (tests/test_l0_constrained_gpu.py)
    refused("con_infeasible", lambda: ds.solve_l0_constrained(np.eye(12)[[0, 5]], 0.2, np.inf, max_groups=1, big_M=100.0))
    refused("l0", lambda: ds.solve_l0(alpha=-1.0))
    refused("xb", lambda: ds.solve_l0_xb(alpha=-1.0))
    refused("l1", lambda: ds.solve_l0_l1(alpha=-1.0, eta_l1=0.1))
    refused("wide", lambda: ds.solve_l0_wide(alpha=-1.0))
    refused("xb_wide", lambda: ds.solve_l0_xb_wide(alpha=-1.0))
    refused("profile", lambda: ds.solve_l0_profile(alpha_min=-1.0, max_groups=3))
    refused("profile_wide", lambda: ds.solve_l0_profile_wide(alpha_min=-1.0, max_groups=3))
    refused("con", lambda: ds.solve_l0_constrained(ones, 0.0, 1.0, alpha=-1.0))
    refused("need_bit", lambda: ds.solve_l0(need=[1 << 12] + [0] * 11))
    refused("need_bit_wide", lambda: ds.solve_l0_wide(need=[1 << 12] + [0] * 11))
X, y, _, _, _ = suppressor(20)
with eng.dataset(X, y) as ds:  # 20 singleton groups: four levels below the ticket prefix
    keep("singletons_20", lambda: ds.solve_l0(max_groups=5, big_M=1000.0), COUNTS)
    keep("singletons_20_xb", lambda: ds.solve_l0_xb(max_groups=5, big_M=1000.0), COUNTS)
    keep("singletons_20_profile", lambda: ds.solve_l0_profile(max_groups=4, big_M=1000.0))
    keep("budget", lambda: ds.solve_l0(max_groups=10, big_M=1000.0, max_nodes=1), budget=True)
    assert "node_budget" in str(out["budget/status"])
X, y, groups, _, _ = suppressor(8, width=3, n=60)
with eng.dataset(X, y) as ds:  # grouped columns, a hierarchy: group 0 needs 5, group 3 needs 0
    ds.set_groups(np.asarray(groups, dtype=np.int64), 8)
    need = [1 << 5, 0, 0, 1 << 0, 0, 0, 0, 0]
    keep("groups_need", lambda: ds.solve_l0(max_groups=4, big_M=1000.0, need=need), COUNTS)
    keep("groups_need_wide", lambda: ds.solve_l0_wide(alpha=1e-4 * float(np.var(y)), big_M=1000.0, need=need))
    keep("groups_need_profile", lambda: ds.solve_l0_profile(max_groups=6, big_M=1000.0, need=need))
    keep("groups_need_con", lambda: ds.solve_l0_constrained(np.ones((1, 24)), -1.0, 1.0, max_groups=4, big_M=100.0, need=need), COUNTS)
X, y, _, _, _ = suppressor(80, pairs=1, tau=0.3, n=120)
with eng.dataset(X, y) as ds:  # 80 singletons: the high mask word; a hierarchy across bit 64
    need = [0] * 80
    need[3], need[70] = 1 << 70, 1 << 2
    keep("wide_80", lambda: ds.solve_l0_wide(max_groups=2, big_M=1000.0))
    keep("wide_80_need", lambda: ds.solve_l0_wide(max_groups=3, big_M=1000.0, need=need))
    keep("wide_80_xb", lambda: ds.solve_l0_xb_wide(max_groups=2, big_M=1000.0))
    keep("wide_80_profile", lambda: ds.solve_l0_profile_wide(max_groups=2, big_M=1000.0, need=need))
X, y, groups = ten_groups_of_eight()
with eng.dataset(X, y) as ds:  # ten groups of eight columns: includes are refused for capacity
    ds.set_groups(np.asarray(groups, dtype=np.int64), 10)
    keep("capacity", lambda: ds.solve_l0_wide(alpha=1e-9 * float(np.var(y)), big_M=1000.0))
    assert "capacity" in str(out["capacity/status"])

# ---- the local search: the four entries, by ctypes ---------------------------------------------------------------------------------
from test_l0_local_gpu import draw as draw_local

def keep_local(tag, fn, message=True):
    """every output array and every field of every record of the call, or what it raised"""
    del records[:]
    try:
        res = fn()
    except Exception as exc:
        if message:
            out[tag + "/raised"] = np.array(f"{type(exc).__name__}: {exc}")
        else:
            out[tag + "/raised_type"] = np.array(type(exc).__name__)
            out[tag + "/print/message"] = np.array(str(exc))
        return
    out[tag + "/status"] = np.array("returned")
    for i, v in enumerate(res[:-1]):
        out[f"{tag}/out{i}"] = np.asarray(v)
    for name in records[-1].dtype.names:
        out[f"{tag}/rec/{name}"] = np.array(records[-1][name])

def refused_local(tag, fn):
    keep_local(tag + "/refused", fn)
    assert tag + "/refused/raised" in out, tag

def raw(ds, name, args, cnt, ps, nstat=None):
    """the C entry with exactly these arguments (None: NULL), past the wrapper's coercions"""
    outs = [np.zeros((cnt, ps)), np.zeros(cnt), np.zeros(cnt, dtype=np.int32)]
    if nstat:
        outs = [outs[0], np.zeros(cnt), outs[1], outs[2], np.zeros((cnt, nstat), dtype=np.int32)]
    return ds._l0_call(name, False, args, outs, records=cnt)

rng = np.random.default_rng(7)
for p in (5, 64, 65, 130):
    X, y = draw_local(40, p, 3, p)
    var = float(np.var(y))
    alphas, etas = np.array([0.01, 0.1, 10.0]) * var, np.array([0.0, 0.02, 0.0])  # (the last alpha: an empty winner)
    sizes = np.array([1, 3, p])
    mask = np.ones(40)
    mask[rng.choice(40, 8, replace=False)] = 0.0
    sets = [mask * (40 / 32), rng.uniform(0.5, 1.5, 40), None]
    n_effs = [32, 40, 0]
    given = np.zeros((3, 2, p))
    given[:, 1, ::3] = 0.25
    if p > 64:
        given[:, 1, 62:66] = -0.25  # (a support across the slot boundary)
    with eng.dataset(X, y) as ds, eng.dataset(np.hstack([X, np.ones((40, 1))]), y) as ds1:
        for swaps in (True, False):
            for how, st, ns in (("given", given, None), ("none", None, 2)):
                tag = f"local_p{p}_{'swaps' if swaps else 'descent'}_{how}"
                keep_local(tag + "/single", lambda: ds.solve_l0_local(alphas, etas, starts=st, swaps=swaps, n_starts=ns))
                for count in (1, 3):
                    rws, nes = (sets, n_effs) if count == 3 else ([None], [0])
                    stc = None if st is None else np.broadcast_to(st, (count,) + st.shape)
                    for icpt, d in ((False, ds), (True, ds1)):
                        t = f"{tag}/count{count}_icpt{int(icpt)}"
                        keep_local(t + "/folds", lambda: d.solve_l0_local_folds(rws, nes, alphas, etas, intercept=icpt, starts=stc, swaps=swaps, n_starts=ns))
                        keep_local(t + "/subsets", lambda: d.solve_l0_local_subsets(rws, nes, sizes, etas, intercept=icpt, starts=stc, swaps=swaps, n_starts=ns))
        assert not out[f"local_p{p}_swaps_none/single/out0"][2].any() and out[f"local_p{p}_swaps_none/single/out0"][0].any()
X, y = draw_local(40, 5, 3, 5)
one, box = np.array([0.1]), np.full((1, 1, 5), 0.25)
wide = np.random.default_rng(0).standard_normal((8, 1025))
with eng.dataset(X, y) as ds, eng.dataset(wide, np.ones(8)) as dw:
    # l0_ls_check, by the single-set entry
    refused_local("ls_null", lambda: raw(ds, "solve_l0_local", (1, None, one, 100.0, 1, None), 1, 5))
    refused_local("ls_cells", lambda: ds.solve_l0_local(one, n_cells=0))
    refused_local("ls_starts", lambda: ds.solve_l0_local(one, n_starts=0))
    refused_local("ls_problems", lambda: ds.solve_l0_local(np.full(8193, 0.1)))
    refused_local("ls_big_M", lambda: ds.solve_l0_local(one, big_M=-1.0))
    refused_local("ls_alpha", lambda: ds.solve_l0_local([0.1, -1.0]))
    refused_local("ls_eta", lambda: ds.solve_l0_local([0.1, 0.1], etas=[0.0, np.nan]))
    refused_local("ls_width", lambda: dw.solve_l0_local(one))
    refused_local("ls_width_descent", lambda: dw.solve_l0_local(one, swaps=False))
    refused_local("ls_box", lambda: ds.solve_l0_local(one, big_M=0.1, starts=box))
    # l0_lsf_check, by the row-set entry
    ptr0, ne0 = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.int64)
    refused_local("lsf_count0", lambda: ds.solve_l0_local_folds([], [], one))
    refused_local("lsf_count17", lambda: ds.solve_l0_local_folds([None] * 17, [0] * 17, one))
    refused_local("lsf_null", lambda: raw(ds, "solve_l0_local_folds", (1, ptr0, ne0, 0, 1, None, one, 100.0, 1, None, 1), 1, 5, 4))
    refused_local("lsf_cells", lambda: ds.solve_l0_local_folds([None], [0], one, n_cells=0))
    refused_local("lsf_starts", lambda: ds.solve_l0_local_folds([None], [0], one, n_starts=0))
    refused_local("lsf_product", lambda: ds.solve_l0_local_folds([None] * 3, [0] * 3, np.full(4096, 0.1)))
    refused_local("lsf_big_M", lambda: ds.solve_l0_local_folds([None], [0], one, big_M=-1.0))
    refused_local("lsf_alpha", lambda: ds.solve_l0_local_folds([None], [0], [0.1, -1.0]))
    refused_local("lsf_eta", lambda: ds.solve_l0_local_folds([None], [0], [0.1, 0.1], etas=[0.0, np.nan]))
    refused_local("lsf_width", lambda: dw.solve_l0_local_folds([None], [0], one))
    refused_local("lsf_weight", lambda: ds.solve_l0_local_folds([np.r_[np.ones(39), -1.0]], [40], one))
    refused_local("lsf_box", lambda: ds.solve_l0_local_folds([None], [0], one, big_M=0.1, starts=box[None]))
    # l0_lc_check, by the cardinality entry
    refused_local("lc_null", lambda: ds.solve_l0_local_subsets([None], [0], None))
    refused_local("lc_size", lambda: ds.solve_l0_local_subsets([None], [0], [2, 0]))
    refused_local("lc_eta", lambda: ds.solve_l0_local_subsets([None], [0], [2, 2], etas=[0.0, -1.0]))
    refused_local("lc_lsf_big_M", lambda: ds.solve_l0_local_subsets([None], [0], [2], big_M=-1.0))
    refused_local("lc_lsf_count", lambda: ds.solve_l0_local_subsets([None] * 17, [0] * 17, [2]))
    # the dataset's shape, behind the checks: the intercept's column not alone in its group, then groups at all
    ds.set_groups(np.array([0, 1, 2, 3, 3]), 4)
    refused_local("lsf_intercept", lambda: ds.solve_l0_local_folds([None], [0], one, intercept=True))
    refused_local("groups_single", lambda: ds.solve_l0_local(one))
    refused_local("groups_folds", lambda: ds.solve_l0_local_folds([None], [0], one))
    refused_local("groups_subsets", lambda: ds.solve_l0_local_subsets([None], [0], [2]))
Xn = X.copy()
Xn[4, 2] = np.nan
with eng.dataset(Xn, y) as ds:  # (the constructor checks y alone)
    keep_local("nan_single", lambda: ds.solve_l0_local(one), message=False)
    keep_local("nan_folds", lambda: ds.solve_l0_local_folds([None], [0], one), message=False)
    keep_local("nan_subsets", lambda: ds.solve_l0_local_subsets([None], [0], [2]), message=False)
np.savez(out_path, **out)
'''


def run(lib, out_path, limit=300):
    env = dict(os.environ, SLM_HIP_LIBRARY=os.path.abspath(lib))
    o = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-c", CHILD, ROOT, out_path], env=env, capture_output=True, text=True)
    if o.returncode != 0:  # (a fault, an abort, a time limit: nothing more is started)
        print(o.stdout[-2000:], o.stderr[-3000:])
        raise SystemExit(f"{lib}: exit status {o.returncode}; stopped")


def compare(ref, other, say):
    same = set(ref.files) == set(other.files)
    if not same:
        say(f"  different keys: {sorted(set(ref.files) ^ set(other.files))}")
    for key in ref.files:
        if "/print/" in key or key not in other.files:
            continue
        a, b = ref[key], other[key]
        if a.dtype.kind in "iuUb":
            if not np.array_equal(a, b):
                same = False
                say(f"  {key}: {a.tolist()} != {b.tolist()}")
        elif not np.array_equal(a, b, equal_nan=True):
            same = False
            say(f"  {key}: differs: {a.tolist()} != {b.tolist()}" if a.size <= 4 else f"  {key}: differs")
    return same


if __name__ == "__main__":
    args = sys.argv[1:]
    out_file = None
    if "--out" in args:
        i = args.index("--out"); out_file = args[i + 1]; del args[i : i + 2]
    lines = []
    def say(text):
        print(text, flush=True); lines.append(text)
        if out_file:
            with open(out_file, "w") as f:
                f.write("\n".join(lines) + "\n")
    tmp = tempfile.mkdtemp()
    res, all_same = [], True
    for i, lib in enumerate(args):  # (in the order given: name the libraries alternately for alternating children)
        path = os.path.join(tmp, f"res{i}.npz")
        run(lib, path)
        res.append(np.load(path))
        keys = res[i].files
        if i == 0:
            say(f"{sum(k.endswith('/status') and '/rec/' not in k for k in keys)} calls that returned, {sum(k.endswith('/raised') for k in keys)} that raised, per library")
            for k in keys:
                if k.endswith("/raised"):
                    say(f"  {k}: {res[0][k]}")
        printed = sorted({k.split("/")[0] for k in keys if "/print/nodes" in k})
        say(f"child {i} ({lib}), not compared -- nodes[, descents or qp solves]: " + " ".join(
            f"{t} {int(res[i][t + '/print/nodes'])}" + (f",{int(res[i][t + '/print/rejects'])}" if t + "/print/rejects" in keys else "") for t in printed))
        for k in keys:
            if k.endswith("/print/message"):
                say(f"  child {i}, printed: {k.split('/')[0]} raised {res[i][k.replace('/print/message', '/raised_type')]}: {res[i][k]}")
        if i > 0:
            same = compare(res[0], res[i], say)
            all_same = all_same and same
            say(f"{lib} (child {i}) against {args[0]}: " + ("every output and every compared record field equal bit for bit" if same else "DIFFERENT (above)"))
    sys.exit(0 if all_same else 1)
