"""The configuration key plant_perturbation (robotic_mpc_amd/plant.py) on the host: validation, sampling, buckets, grid keys,
checkpoints, sharding.  No device."""
import json

import numpy as np
import pytest

from robotic_mpc_amd import config, packing, plant

NOISE = {"kind": "gaussian", "sigma_q": 1e-3, "sigma_qdot": 1e-2, "seed": 3}
DIST = {"kind": "gaussian", "sigma": 0.02, "seed": 3}
SPEC = {"wcv_scale": 0.9, "input_disturbance": DIST, "measurement_noise": NOISE}


def _cfg(**kw):
    return config.resolve_config(config.base_params(**{**dict(prediction_horizon=12, simulation_time=0.3), **kw}))


# ------------------------------------------------------------------------------------------------------------- validation
@pytest.mark.parametrize("spec,word", [
    ([1.0], "plant_perturbation must be a dict"),
    ({"wcv": 1.0}, "has the keys"),
    ({"wcv_scale": [1.0, 1.0]}, "wcv_scale"),
    ({"wcv_scale": 0.0}, "wcv_scale must be > 0"),
    ({"wcv_scale": "fast"}, "wcv_scale"),
    ({"wcv_scale": float("nan")}, "wcv_scale must be finite"),
    ({"input_disturbance": 0.05}, "input_disturbance must be a dict"),
    ({"input_disturbance": {"kind": "ramp"}}, "input_disturbance.kind"),
    ({"input_disturbance": {"kind": "step", "value": 0.05}}, "'step' plant_perturbation input_disturbance has the keys"),
    ({"input_disturbance": {"kind": "step", "start_time": -1.0, "value": 0.05}}, "input_disturbance.start_time"),
    ({"input_disturbance": {"kind": "step", "start_time": 0.1, "value": [0.05] * 5}}, "input_disturbance.value"),
    ({"input_disturbance": {"kind": "gaussian", "sigma": -1.0, "seed": 0}}, "input_disturbance.sigma must be >= 0"),
    ({"input_disturbance": {"kind": "gaussian", "sigma": 1.0, "seed": 0.5}}, "input_disturbance.seed"),
    ({"input_disturbance": {"kind": "table", "rows": [[0.0] * 5] * 30}}, "input_disturbance.rows must be \\[Nsim\\]\\[6\\]"),
    ({"measurement_noise": {"kind": "step", "start_time": 0.0, "value": 0.1}}, "measurement_noise.kind"),
    ({"measurement_noise": {"kind": "gaussian", "sigma_q": 1e-3, "seed": 0}}, "'gaussian' plant_perturbation measurement_noise has the keys"),
    ({"measurement_noise": {"kind": "gaussian", "sigma_q": 1e-3, "sigma_qdot": [1e-2] * 12, "seed": 0}}, "measurement_noise.sigma_qdot"),
    ({"measurement_noise": {"kind": "table", "rows": [[0.0] * 6] * 30}}, "measurement_noise.rows must be \\[Nsim\\]\\[12\\]"),
    ({"measurement_noise": {"kind": "table", "rows": [[float("inf")] * 12] * 30}}, "measurement_noise.rows must be finite"),
])
def test_bad_specs_are_refused_with_the_keys_name_when_the_config_is_resolved(spec, word):
    with pytest.raises(ValueError, match=word):
        plant.validate(spec)
    with pytest.raises(ValueError, match=word):
        _cfg(plant_perturbation=spec)


def test_table_row_counts_are_checked_against_the_run_length():
    assert _cfg()["Nsim"] == 30
    ok = _cfg(plant_perturbation={"input_disturbance": {"kind": "table", "rows": np.ones((30, 6)).tolist()},
                                  "measurement_noise": {"kind": "table", "rows": np.full((30, 12), 2.0).tolist()}})
    s = plant.sample(ok)
    assert (s["u_dist"] == 1.0).all() and (s["x_noise"] == 2.0).all() and np.array_equal(s["wcv"], ok["wcv"])
    with pytest.raises(ValueError, match="input_disturbance needs exactly Nsim = 30 rows, got 29"):
        _cfg(plant_perturbation={"input_disturbance": {"kind": "table", "rows": np.ones((29, 6)).tolist()}})
    with pytest.raises(ValueError, match="measurement_noise needs exactly Nsim = 30 rows, got 31"):
        _cfg(plant_perturbation={"measurement_noise": {"kind": "table", "rows": np.ones((31, 12)).tolist()}})


def test_fp32_refuses_a_perturbation_and_sample_refuses_a_config_without_one():
    with pytest.raises(ValueError, match="fp64"):
        _cfg(plant_perturbation=SPEC, riccati_precision="fp32")
    assert _cfg()["plant_perturbation"] is None
    with pytest.raises(ValueError, match="no plant_perturbation"):
        plant.sample(_cfg())
    assert plant.realised(_cfg()) == {}


# --------------------------------------------------------------------------------------------------------------- sampling
def test_sample_shapes_determinism_and_independent_streams():
    c = _cfg(plant_perturbation=SPEC)
    s = plant.sample(c)
    assert s["wcv"].shape == (6,) and s["u_dist"].shape == (30, 6) and s["x_noise"].shape == (30, 12)
    assert all(v.dtype == np.float64 for v in s.values())
    again = plant.sample(_cfg(plant_perturbation=json.loads(json.dumps(SPEC))))
    for k in s:
        np.testing.assert_array_equal(s[k], again[k])
    # the documented draws: default_rng([seed, k]), k = 0 the disturbance, k = 1 the noise
    np.testing.assert_array_equal(s["u_dist"], np.random.default_rng([3, 0]).standard_normal((30, 6)) * 0.02)
    sig = np.array([1e-3] * 6 + [1e-2] * 6)
    np.testing.assert_array_equal(s["x_noise"], np.random.default_rng([3, 1]).standard_normal((30, 12)) * sig)
    # the same seed in both parts: two streams, not one (the noise's q columns are not the disturbance rescaled)
    assert np.abs(s["x_noise"][:, :6] / 1e-3 - s["u_dist"] / 0.02).max() > 0.1
    # a part's table does not depend on the other part being there
    alone = plant.sample(_cfg(plant_perturbation={"measurement_noise": NOISE}))
    np.testing.assert_array_equal(alone["x_noise"], s["x_noise"])
    assert (alone["u_dist"] == 0).all() and np.array_equal(alone["wcv"], c["wcv"])
    other = plant.sample(_cfg(plant_perturbation={"measurement_noise": dict(NOISE, seed=4)}))
    assert np.abs(other["x_noise"] - s["x_noise"]).max() > 1e-4
    # per-joint sigmas
    v = plant.sample(_cfg(plant_perturbation={"input_disturbance": {"kind": "gaussian", "sigma": [0, 1, 2, 3, 4, 5], "seed": 3}}))
    np.testing.assert_array_equal(v["u_dist"], np.random.default_rng([3, 0]).standard_normal((30, 6)) * np.arange(6.0))


def test_wcv_scale_scalar_and_vector():
    base = _cfg()
    np.testing.assert_array_equal(plant.sample(_cfg(plant_perturbation={"wcv_scale": 0.8}))["wcv"], base["wcv"] * 0.8)
    scale = [0.7, 0.8, 0.9, 1.0, 1.1, 1.2]
    np.testing.assert_array_equal(plant.sample(_cfg(plant_perturbation={"wcv_scale": scale}))["wcv"], base["wcv"] * np.array(scale))
    np.testing.assert_array_equal(plant.sample(_cfg(plant_perturbation={}))["wcv"], base["wcv"])
    # the model keeps its bandwidths: the parameter record does not see the perturbation
    np.testing.assert_array_equal(packing.pack_params(_cfg(plant_perturbation={"wcv_scale": 0.8})), packing.pack_params(base))


def test_step_disturbance_starts_at_the_row_of_its_start_time():
    dt = _cfg()["dt"]
    for start, first in ((0.0, 0), (10 * dt, 10), (9.5 * dt, 10), (29 * dt, 29), (1.0, 30)):
        s = plant.sample(_cfg(plant_perturbation={"input_disturbance": {"kind": "step", "start_time": start, "value": [1, 2, 3, 4, 5, 6]}}))
        assert (s["u_dist"][:first] == 0).all(), start
        assert (s["u_dist"][first:] == np.arange(1.0, 7.0)).all(), start
    s = plant.sample(_cfg(plant_perturbation={"input_disturbance": {"kind": "step", "start_time": 0.1, "value": 0.05}}))
    assert (s["u_dist"][10:] == 0.05).all()


def test_realised_tables_are_what_get_data_adds():
    c = _cfg(plant_perturbation={"wcv_scale": 0.9, "measurement_noise": NOISE})
    r = plant.realised(c)
    assert sorted(r) == ["measurement_noise"] and r["measurement_noise"].shape == (30, 12)
    r = plant.realised(_cfg(plant_perturbation=SPEC))
    assert sorted(r) == ["input_disturbance", "measurement_noise"] and r["input_disturbance"].shape == (30, 6)


# ------------------------------------------------------------------------------------------ config, buckets, grid, shards
def test_config_key_survives_json_and_the_checkpoints_config_round_trip():
    from robotic_mpc_amd import results_io

    raw = config.base_params(plant_perturbation=SPEC, prediction_horizon=12, simulation_time=0.3)
    c = config.resolve_config(raw)
    assert c["plant_perturbation"] == SPEC and c["plant_perturbation"] is not SPEC
    assert c["plant_perturbation"]["measurement_noise"] is not NOISE
    back = json.loads(results_io.config_json(raw))
    assert back["plant_perturbation"] == SPEC
    for k, v in plant.sample(config.resolve_config(back)).items():
        np.testing.assert_array_equal(v, plant.sample(c)[k])                   # a resume draws the same tables
    other = config.base_params(plant_perturbation=dict(SPEC, measurement_noise=dict(NOISE, seed=4)), prediction_horizon=12, simulation_time=0.3)
    assert results_io.resume_key("a", raw) != results_io.resume_key("a", other)
    assert results_io.resume_key("a", raw) != results_io.resume_key("a", config.base_params(prediction_horizon=12, simulation_time=0.3))


def test_bucket_key_separates_perturbed_simulations():
    from robotic_mpc_amd import distributed
    from robotic_mpc_amd.engine import make_problem

    serp = {"kind": "serpentine", "lanes": 2, "lane_pitch": 0.03, "lane_time": 0.04, "turn_time": 0.05}
    plain, pert, pert2 = _cfg(), _cfg(plant_perturbation=SPEC), _cfg(plant_perturbation={"wcv_scale": 1.1})
    sched, both = _cfg(reference_schedule=serp), _cfg(reference_schedule=serp, plant_perturbation=SPEC)
    assert packing.bucket_key(plain) != packing.bucket_key(pert)
    assert packing.bucket_key(plain, ragged=True) != packing.bucket_key(pert, ragged=True)
    assert packing.bucket_key(pert) == packing.bucket_key(pert2)               # the spec itself is per-simulation data
    assert len({packing.bucket_key(c) for c in (plain, pert, sched, both)}) == 4
    # ragged merging as for schedules: the horizon leaves the key
    short = _cfg(plant_perturbation=SPEC, prediction_horizon=8)
    assert packing.bucket_key(pert) != packing.bucket_key(short) and packing.bucket_key(pert, ragged=True) == packing.bucket_key(short, ragged=True)
    buckets = distributed.group_buckets([plain, pert, plain, pert2, both])
    assert list(buckets.values()) == [[0, 2], [1, 3], [4]]
    with pytest.raises(ValueError):
        make_problem([plain, pert])


def test_dotted_grid_keys_reach_the_spec_at_every_depth():
    from robotic_mpc_amd.simulator import SimulationManager

    base = config.base_params(plant_perturbation={"wcv_scale": 1.0, "measurement_noise": dict(NOISE, seed=0)}, simulation_time=0.3,
                              prediction_horizon=12)
    mgr = SimulationManager(base)
    mgr.grid_search({"plant_perturbation.wcv_scale": [0.8, 1.2], "plant_perturbation.measurement_noise.seed": [0, 1],
                     "prediction_horizon": [8, 12]})
    got = [(s["config"]["plant_perturbation"]["wcv_scale"], s["config"]["plant_perturbation"]["measurement_noise"]["seed"],
            s["config"]["prediction_horizon"]) for s in mgr.simulations]
    assert got == [(w, s, N) for w in (0.8, 1.2) for s in (0, 1) for N in (8, 12)]
    assert mgr.base_config["plant_perturbation"] == {"wcv_scale": 1.0, "measurement_noise": dict(NOISE, seed=0)}   # copied, not aliased
    assert base["plant_perturbation"]["measurement_noise"]["seed"] == 0
    assert len({id(s["config"]["plant_perturbation"]["measurement_noise"]) for s in mgr.simulations}) == 8
    resolved = [config.resolve_config(s["config"]) for s in mgr.simulations]
    assert np.abs(plant.sample(resolved[0])["x_noise"] - plant.sample(resolved[2])["x_noise"]).max() > 1e-4
    np.testing.assert_array_equal(plant.sample(resolved[0])["x_noise"], plant.sample(resolved[4])["x_noise"])


def test_a_ranks_chunk_of_the_stack_is_the_stack_of_its_configs():
    from robotic_mpc_amd import distributed

    cfgs = [_cfg(plant_perturbation={"wcv_scale": 0.7 + 0.05 * i, "input_disturbance": dict(DIST, seed=i), "measurement_noise": dict(NOISE, seed=i)})
            for i in range(7)]
    full = plant.stack(cfgs)
    assert full["wcv"].shape == (7, 6) and full["u_dist"].shape == (7, 30, 6) and full["x_noise"].shape == (7, 30, 12)
    assert all(v.flags["C_CONTIGUOUS"] for v in full.values())
    seen = []
    for rank in range(3):
        for idxs in distributed.group_buckets(cfgs, 3).values():
            lo, hi = distributed.chunk_bounds(len(idxs), 3)[rank]              # (run_partitioned: a rank's contiguous chunk)
            mine = idxs[lo:hi]
            part = plant.stack([cfgs[i] for i in mine])
            for k in full:
                np.testing.assert_array_equal(part[k], full[k][list(mine)])
            seen += list(mine)
    assert sorted(seen) == list(range(7))


def test_host_buffer_path_refuses_a_perturbation_before_touching_a_device():
    from robotic_mpc_amd.engine import MpcBatchEngine

    eng = object.__new__(MpcBatchEngine)                                      # no handle: the refusal comes first
    with pytest.raises(ValueError, match="plant perturbation"):
        MpcBatchEngine.run_host_buffers(eng, [_cfg(plant_perturbation=SPEC)], None)
