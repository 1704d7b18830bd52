"""The driver's bench.py contract (one JSON line with the fields the round prompt names), run end to end on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"]


def _run_bench(*flags):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]          # rank 0 prints ONE JSON line
    return json.loads(lines[0])


def test_baseline_names_the_bench_workload():
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    sys.path.insert(0, ROOT)
    import bench
    cfgs = bench.workload_configs(4, 100, 6.0, seed=0, solver="SQP_RTI")
    assert "N=100" in base["metric"] and "dt=0.01" in base["metric"]
    assert len(cfgs) == 4 and all(c["N"] == 100 and c["Nsim"] == 600 and abs(c["dt"] - 0.01) < 1e-15 for c in cfgs)
    assert bench.bytes_per_mpc_step(100) == 8 * (108 * 100 + 95)


def test_dump_outputs_keeps_a_fixed_sample_within_the_budget(tmp_path):
    """--dump-outputs: every result array as float64, the timing arrays and timing columns left out; over the budget, the
    same seeded sample of simulations in every array, and the same one from run to run."""
    sys.path.insert(0, ROOT)
    import bench
    from robotic_mpc_amd import engine

    rng = np.random.default_rng(5)
    B, S = 40, 30
    outs = {name: (rng.standard_normal((B,) + shp(S, S + 1)) if ty == "f8" else rng.integers(0, 9, (B,) + shp(S, S + 1), dtype=np.int32))
            for name, ty, shp in engine.RESULT_FIELDS}
    outs["summary"] = rng.standard_normal((B, engine.NSUMMARY))
    info = bench.dump_outputs(outs, str(tmp_path / "all"))
    assert info["simulations"] == B and "solver_time" not in info["arrays"] and "plant_time" not in info["arrays"]
    for k in info["arrays"]:
        a = np.load(tmp_path / "all" / f"{k}.npy")
        assert a.dtype == np.float64
        if k != "summary":
            np.testing.assert_array_equal(a, outs[k])
    cols = [i for i, c in enumerate(engine.SUMMARY_COLS) if "time" not in c]
    np.testing.assert_array_equal(np.load(tmp_path / "all" / "summary.npy"), outs["summary"][:, cols])

    budget = 100_000
    a = bench.dump_outputs(outs, str(tmp_path / "a"), budget=budget)
    b = bench.dump_outputs(outs, str(tmp_path / "b"), budget=budget)
    assert 1 <= a["simulations"] < B and a == {**b, "dir": a["dir"]}
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= budget
    z = np.load(tmp_path / "a" / "z.npy")
    rows = [int(np.flatnonzero((outs["z"] == r).all(axis=(1, 2)))[0]) for r in z]
    assert rows == sorted(rows) and len(set(rows)) == len(rows)
    for k in ("u", "status", "summary"):
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f"{k}.npy")[:, 0], np.asarray(outs[k], np.float64)[rows][:, 0])
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "z.npy"), z)


@pytest.mark.timeout(300)
def test_plain_gpus_n_starts_its_own_ranks():
    """`python bench.py --gpus 2` (no launcher, no WORLD_SIZE) must start its ranks itself.  In a
    container without a GPU both ranks get as far as creating the engine and fail loudly there (no CPU fallback); the
    parent -- which never imports torch -- forwards the launcher's exit code."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("CPU-container check of the launch plumbing; the GPU run is test_self_launched_two_ranks_on_one_gpu")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                          "--backend", "gloo", "--no-cpu-baseline", "--batch", "4", "--sim-time", "0.05"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert out.returncode != 0
    assert "2-rank child launch exited" in out.stderr
    # the ranks themselves ran bench.py under torch.distributed.run (rank-tagged failure records), up to the device
    assert "ChildFailedError" in out.stderr or "exitcode" in out.stderr
    assert "needs one process per GPU" not in out.stderr


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_self_launched_two_ranks_on_one_gpu():
    """The same path on the GPU box: two gloo ranks sharing the one GPU, started by bench.py itself; rank 0 prints ONE
    line carrying n_gpus = 2, the whole-job value and the cpu_baseline (N > 1 lines carry it too)."""
    r = _run_bench("--gpus", "2", "--backend", "gloo", "--steps", "1", "--warmup", "1", "--batch", "32", "--sim-time", "0.3", "--full")
    assert r["n_gpus"] == 2 and r["scaling"] == "weak"
    assert abs(r["value"] - 2 * 32 * 30 / (r["ms_per_step"] * 1e-3)) <= 1e-6 * r["value"]
    assert r["cpu_baseline"] and r["cpu_baseline"]["kind"] == "port" and r["cpu_baseline"]["value"] > 0
    assert "gather" in r["config"]["timed_region"]


@pytest.mark.gpu
def test_bench_line_on_a_small_workload():
    # a reduced workload (the contract, not the number): 64 simulations, 60 closed-loop steps
    r = _run_bench("--steps", "2", "--warmup", "1", "--batch", "64", "--sim-time", "0.6", "--full")
    for k in REQUIRED:
        assert k in r, k
    assert r["n_gpus"] == 1 and r["steps"] == 2 and r["warmup"] == 1 and r["higher_is_better"] is True
    assert r["dtype"] == "f64" and r["scaling"] == "weak" and r["vs_baseline"] is None and "synthetic" in r["data"]
    assert "workload" in r["config"] and "model" not in r["config"]
    # value = whole-job MPC steps / timed seconds
    steps_per_pass = 64 * 60
    assert abs(r["value"] - steps_per_pass / (r["ms_per_step"] * 1e-3)) <= 1e-6 * r["value"]
    rf = r["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-12
    assert rf["avg_launch_ms"] <= r["ms_per_step"] + 1e-6       # the kernel is inside the timed region
    assert abs(rf["achieved"] - rf["algorithmic_bytes_per_launch"] / (rf["avg_launch_ms"] * 1e-3) / 1e9) <= 1e-6 * rf["achieved"]
    cb = r["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["value"] > 0 and "sample" in cb
    assert r["config"]["solver_failures"] == 0
    sec = r["secondary"]                     # extra record outside the timed region: the throughput geometry
    assert "4096" in sec["workload"] and sec["engine"].startswith("throughput") and sec["kernel_steps_per_s"] > 0 and sec["solver_failures"] == 0
    srf = sec["roofline"]                    # the throughput kernel's own roofline block
    assert srf["bound"] == "hbm" and abs(srf["frac"] - srf["achieved"] / srf["peak"]) < 1e-12 and "mpc_stream_kernel" in srf["kernel"]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_what_it_timed(orc, ur10_rb, tmp_path):
    """A plain run: `--steps` timed steps, no CPU baseline, no secondary record; --dump-outputs holds the last timed step's
    results of the seeded workload, which equal the oracle's on the same parameters."""
    sys.path.insert(0, ROOT)
    import bench

    r = _run_bench("--steps", "3", "--warmup", "1", "--batch", "4", "--sim-time", "0.3", "--dump-outputs", str(tmp_path))
    assert r["steps"] == 3 and r["cpu_baseline"] is None and "secondary" not in r
    assert len(r["config"]["pass_ms_rank0"]) == 3
    assert abs(r["value"] - 4 * 30 / (r["ms_per_step"] * 1e-3)) <= 1e-6 * r["value"]
    d = r["config"]["outputs_dumped"]
    assert d["simulations"] == 4 and d["sample"] == "all"
    out = {k: np.load(tmp_path / f"{k}.npy") for k in d["arrays"]}
    assert all(a.dtype == np.float64 and a.shape[0] == 4 for a in out.values())
    for i, c in enumerate(bench.workload_configs(4, 100, 0.3, seed=0, solver="SQP_RTI")):
        ref = orc.run(ur10_rb, orc.make_params(c))
        for k in ("z", "u", "ee_pose"):
            np.testing.assert_allclose(out[k][i], ref[k], atol=1e-9, rtol=0, err_msg=k)
        np.testing.assert_array_equal(out["status"][i], ref["status"])
