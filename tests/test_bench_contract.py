"""Host-side pieces of bench.py that need no GPU: the CPU share the CPU legs are sized to, the argument defaults of the
contract (`python bench.py` alone = one GPU, a few steps, nothing beside the headline without `--full`), the synthetic
coefficient law."""

import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _bench():
    spec = importlib.util.spec_from_file_location("_bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cpu_share_is_the_affinity_mask_cut_to_the_cgroup_quota(tmp_path, monkeypatch):
    bench = _bench()
    share = bench._host_cpu_share()
    assert 1 <= share <= len(os.sched_getaffinity(0))
    assert bench.HOST_CPUS == share
    # a quota of 2.5 CPUs in a cgroup-v2 file: three threads at most
    real_open = open

    def fake_open(path, *a, **k):
        if path == "/sys/fs/cgroup/cpu.max":
            p = tmp_path / "cpu.max"
            p.write_text("250000 100000\n")
            return real_open(p, *a, **k)
        return real_open(path, *a, **k)

    monkeypatch.setattr("builtins.open", fake_open)
    assert bench._host_cpu_share() == min(3, len(os.sched_getaffinity(0)))


def test_defaults_of_the_contract():
    bench = _bench()
    assert bench.PRIMING_PATHS >= 1 and bench.HBM_PEAK_GBS == 8000.0
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert '"--gpus", type=int, default=1' in src and '"--steps", type=int, default=5' in src
    coef = bench.make_coef(5000, 50, seed=0)
    assert coef.shape == (5000,) and np.count_nonzero(coef) == 50
    np.testing.assert_array_equal(coef, bench.make_coef(5000, 50, seed=0))


def test_a_plain_run_leaves_everything_beside_the_headline_to_full():
    bench = _bench()
    plain = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "2"])
    assert not plain.full and (plain.gpus, plain.steps, plain.warmup) == (1, 3, 2)
    assert bench.parse_args([]).full is False
    full = bench.parse_args(["--full", "--legs", "soak,config3_path", "--cpu-budget", "0"])
    assert full.full and full.legs == "soak,config3_path" and full.cpu_budget == 0.0


def test_strong_scaling_object_and_cpu_baseline_layout():
    """The objects the contract line carries beside `value` (round-5 verdict, items 2 and 8): keys a reader may rely on."""
    bench = _bench()
    ss = bench.strong_scaling_object(0.09, 0.027, 8)
    assert {"metric", "scaling", "n_gpus", "unit", "higher_is_better", "value", "seconds_per_grid", "route",
            "value_from_fold_grams", "seconds_per_grid_from_fold_grams", "note"} <= set(ss)
    assert ss["scaling"] == "strong" and ss["n_gpus"] == 8 and abs(ss["value"] - 2500.0 / 0.09) < 1e-9
    assert bench.strong_scaling_object(0.09, None, 1)["value_from_fold_grams"] is None
    port = {"value": 2.4, "unit": "fits/s", "cores": 16, "kind": "port", "sample": "first 49 ...", "beta_rel_inf_err_gpu_vs_oracle": 1e-8,
            "cvxpy": {"status": "cvxpy unavailable on box"}}
    assert bench.stock_first(dict(port), 50, 100000, 5000) == port  # (no scikit-learn figure: the port is the value)
    both = dict(port, sklearn_lasso_path={"value": 18.5, "unit": "fits/s", "cores": 16, "seconds_per_path": 2.7, "what": "lasso_path(...)",
                                          "beta_rel_inf_err_gpu_vs_sklearn": 2e-11})
    cb = bench.stock_first(both, 50, 100000, 5000)
    assert cb["kind"] == "stock" and cb["value"] == 18.5 and cb["port"]["kind"] == "port" and cb["port"]["value"] == 2.4
    assert {"value", "unit", "cores", "kind", "sample"} <= set(cb) and {"value", "unit", "cores", "kind", "sample"} <= set(cb["port"])


def test_dump_outputs_writes_the_path_result_in_float64(tmp_path):
    """--dump-outputs: every array of the path's result as DIR/<name>.npy, float64, the same on a second write."""
    bench = _bench()

    class FakeResult:  # the attributes of sparselm_amd._engine.PathResult that path_outputs reads
        betas = np.arange(12.0).reshape(3, 4)
        group_norms = None
        n_iter = np.array([5, 6, 7])
        status = np.zeros(3, dtype=np.int64)
        mode = np.array([1, 1, 0])
        resid = beta_norm = loss = kkt = mu = np.array([0.5, 0.25, 0.125])
        L = 3.5

    arrays = bench.path_outputs(FakeResult())
    assert set(arrays) == {"betas", "n_iter", "status", "mode", "resid", "beta_norm", "loss", "kkt", "mu", "L"}
    bench.write_dump(arrays, str(tmp_path / "a"))
    bench.write_dump(bench.path_outputs(FakeResult()), str(tmp_path / "b"))
    for name in arrays:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float64
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "betas.npy"), FakeResult.betas)
    assert np.load(tmp_path / "a" / "L.npy")[0] == 3.5


def test_dump_outputs_keeps_a_fixed_sample_of_columns_past_the_limit(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(3)
    arrays = {"betas": rng.standard_normal((10, 1000)), "group_norms": rng.standard_normal((10, 100)), "loss": np.ones(10)}
    limit = 20_000
    bench.write_dump(dict(arrays), str(tmp_path / "a"), limit=limit)
    bench.write_dump(dict(arrays), str(tmp_path / "b"), limit=limit)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["betas.npy", "betas_columns.npy", "group_norms.npy", "group_norms_columns.npy", "loss.npy"]
    assert sum(np.load(tmp_path / "a" / f).nbytes for f in files) <= limit
    for key in ("betas", "group_norms"):
        cols = np.load(tmp_path / "a" / f"{key}_columns.npy")
        np.testing.assert_array_equal(cols, np.load(tmp_path / "b" / f"{key}_columns.npy"))
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"{key}.npy"), arrays[key][:, cols.astype(np.int64)])
