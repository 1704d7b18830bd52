"""Task reference schedules of rollouts, the host side: the sampler (robotic_mpc_amd.reference), the configuration key, the launch
buckets and the generalised error formula (analysis.compute_errors yref=).  No device."""
import json

import numpy as np
import pytest

from robotic_mpc_amd import analysis, config, packing, reference

SERP = {"kind": "serpentine", "lanes": 3, "lane_pitch": 0.03, "lane_time": 0.04, "turn_time": 0.05}


def _cfg(**kw):
    kw.setdefault("prediction_horizon", 12)
    kw.setdefault("simulation_time", 0.30 + 1e-9)
    return config.resolve_config(config.base_params(**kw))


# ----------------------------------------------------------------------------------------------- sampler
def test_serpentine_lane_values_turns_and_hold():
    c = _cfg(reference_schedule=SERP, px_ref=0.37, vy_ref=0.04)
    y = reference.sample(c)
    assert y.shape == (c["Nsim"] + c["N"], 5) and y.dtype == np.float64
    np.testing.assert_array_equal(y[:, :3], np.tile([0.0, 1.0, 0.0], (len(y), 1)))
    t = np.arange(len(y)) * c["dt"]
    period = SERP["lane_time"] + SERP["turn_time"]
    for r, tr in enumerate(t):
        m = min(int(np.floor(tr / period)), SERP["lanes"] - 1)
        into = tr - m * period
        if into < SERP["lane_time"] or m == SERP["lanes"] - 1:
            # on a lane (or holding after the last one)
            assert y[r, 3] == pytest.approx(0.37 + m * 0.03, abs=1e-15), r
            assert y[r, 4] == pytest.approx((-1) ** m * 0.04, abs=1e-15), r
        else:
            tau = (into - SERP["lane_time"]) / SERP["turn_time"]
            s = 3 * tau ** 2 - 2 * tau ** 3
            assert y[r, 3] == pytest.approx(0.37 + (m + s) * 0.03, abs=1e-15), r
            assert y[r, 4] == pytest.approx((-1) ** m * 0.04 * (1 - 2 * s), abs=1e-15), r
    # the reference holds after the last lane has begun
    last = t >= (SERP["lanes"] - 1) * period - 1e-12
    assert last.sum() > 5
    np.testing.assert_array_equal(y[last], np.tile(y[-1], (last.sum(), 1)))
    assert y[-1, 3] == pytest.approx(0.37 + 2 * 0.03) and y[-1, 4] == pytest.approx(0.04)
    # v_y changes sign within the schedule
    assert (y[:, 4] > 0).any() and (y[:, 4] < 0).any()


def test_serpentine_is_continuous_across_a_turn():
    """Sampled finely, neither target jumps: a step of dt moves p_x by at most 1.5 * pitch * dt / turn_time (the steepest slope of
    3 tau^2 - 2 tau^3) and v_y by at most 3 * vy_ref * dt / turn_time."""
    spec = dict(SERP, lane_time=0.04, turn_time=0.05)
    c = _cfg(reference_schedule=spec, dt=0.0005, simulation_time=0.2 + 1e-9, prediction_horizon=4)
    y = reference.sample(c)
    assert np.abs(np.diff(y[:, 3])).max() <= 1.5 * 0.03 * 0.0005 / 0.05 * (1 + 1e-9)
    assert np.abs(np.diff(y[:, 4])).max() <= 3.0 * c["vy_ref"] * 0.0005 / 0.05 * (1 + 1e-9)
    assert np.ptp(y[:, 3]) == pytest.approx(2 * 0.03)


def test_single_lane_is_the_packed_reference():
    c = _cfg(reference_schedule=dict(SERP, lanes=1))
    y = reference.sample(c)
    np.testing.assert_array_equal(y, reference.packed_rows(c, len(y)))


def test_table_round_trip():
    rows = np.random.default_rng(0).uniform(-1, 1, (30 + 12, 5))
    c = _cfg(reference_schedule={"kind": "table", "rows": rows.tolist()})
    np.testing.assert_array_equal(reference.sample(c), rows)
    np.testing.assert_array_equal(reference.log_rows(c), rows[:31])
    assert reference.log_rows(_cfg()) is None


def test_stack_pads_shorter_horizons_with_their_last_row():
    a, b = _cfg(reference_schedule=SERP, prediction_horizon=5), _cfg(reference_schedule=SERP, prediction_horizon=12, px_ref=0.41)
    s = reference.stack([a, b])
    assert s.shape == (2, 30 + 12, 5)
    np.testing.assert_array_equal(s[0, :35], reference.sample(a))
    np.testing.assert_array_equal(s[0, 35:], np.tile(reference.sample(a)[-1], (7, 1)))
    np.testing.assert_array_equal(s[1], reference.sample(b))


@pytest.mark.parametrize("spec", [
    {"kind": "table", "rows": [[0, 1, 0, 0.4, 0.05]] * 41},                   # one row short of Nsim + N
    {"kind": "table", "rows": [[0, 1, 0, 0.4, 0.05]] * 43},                   # one too many
    {"kind": "table", "rows": [[0, 1, 0, 0.4]] * 42},                         # four columns
    {"kind": "table", "rows": [[0, 1, 0, 0.4, float("nan")]] * 42},           # not finite
    {"kind": "table", "rows": [[0, 1, 0, 0.4, float("inf")]] * 42},
    {"kind": "table"},
    dict(SERP, lanes=0), dict(SERP, lanes=1.5), dict(SERP, lane_time=0.0), dict(SERP, lane_time=-1.0), dict(SERP, turn_time=0.0),
    dict(SERP, lane_pitch=float("nan")), {k: v for k, v in SERP.items() if k != "turn_time"}, dict(SERP, extra=1),
    {"kind": "spiral"}, {"lanes": 2}, "serpentine", [1, 2, 3],
])
def test_bad_specs_are_refused_when_the_config_is_resolved(spec):
    with pytest.raises(ValueError):
        _cfg(reference_schedule=spec)


def test_sample_refuses_a_config_without_a_schedule_and_fp32_refuses_a_schedule():
    with pytest.raises(ValueError):
        reference.sample(_cfg())
    with pytest.raises(ValueError):
        _cfg(reference_schedule=SERP, riccati_precision="fp32")


# ----------------------------------------------------------------------------------------------- config, buckets
def test_config_key_resolves_defaults_to_none_and_survives_json():
    from robotic_mpc_amd import results_io

    assert _cfg()["reference_schedule"] is None
    raw = config.base_params(reference_schedule=SERP, prediction_horizon=12, simulation_time=0.3)
    c = config.resolve_config(raw)
    assert c["reference_schedule"] == SERP and c["reference_schedule"] is not SERP
    assert json.loads(json.dumps(c["reference_schedule"])) == SERP
    # the checkpoint resume key sees the spec
    other = config.base_params(reference_schedule=dict(SERP, lane_time=0.08), prediction_horizon=12, simulation_time=0.3)
    assert json.loads(results_io.config_json(raw))["reference_schedule"] == SERP
    assert results_io.resume_key("a", raw) != results_io.resume_key("a", other)
    assert results_io.resume_key("a", raw) != results_io.resume_key("a", config.base_params(prediction_horizon=12, simulation_time=0.3))


def test_grid_search_paths_reach_the_spec():
    from robotic_mpc_amd.simulator import SimulationManager

    mgr = SimulationManager(config.base_params(reference_schedule=SERP, simulation_time=0.3, prediction_horizon=12))
    mgr.grid_search({"reference_schedule.lane_time": [0.04, 0.08], "prediction_horizon": [8, 12]})
    got = [(s["config"]["reference_schedule"]["lane_time"], s["config"]["prediction_horizon"]) for s in mgr.simulations]
    assert got == [(0.04, 8), (0.04, 12), (0.08, 8), (0.08, 12)]
    assert mgr.base_config["reference_schedule"] == SERP                      # copied, not aliased
    for s in mgr.simulations:
        config.resolve_config(s["config"])


def test_bucket_key_separates_configurations_with_and_without_a_schedule():
    from robotic_mpc_amd import distributed
    from robotic_mpc_amd.engine import make_problem

    plain, sched, sched2 = _cfg(), _cfg(reference_schedule=SERP), _cfg(reference_schedule=dict(SERP, lane_time=0.08))
    assert packing.bucket_key(plain) != packing.bucket_key(sched)
    assert packing.bucket_key(plain, ragged=True) != packing.bucket_key(sched, ragged=True)
    assert packing.bucket_key(sched) == packing.bucket_key(sched2)            # the spec itself is per-simulation data
    buckets = distributed.group_buckets([plain, sched, plain, sched2])
    assert list(buckets.values()) == [[0, 2], [1, 3]]
    with pytest.raises(ValueError):
        make_problem([plain, sched])


def test_host_buffer_path_refuses_a_schedule_before_touching_a_device():
    from robotic_mpc_amd.engine import MpcBatchEngine

    eng = object.__new__(MpcBatchEngine)                                      # no handle: the refusal comes first
    with pytest.raises(ValueError, match="reference schedule"):
        MpcBatchEngine.run_host_buffers(eng, [_cfg(reference_schedule=SERP)], None)


# ----------------------------------------------------------------------------------------------- errors
def _logs(T, seed=3):
    """Pose / velocity logs of T columns: orthonormal rotations, positions near the default surface's workspace."""
    rng = np.random.default_rng(seed)
    pose, vel = np.zeros((12, T)), rng.uniform(-0.3, 0.3, (6, T))
    for t in range(T):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        pose[:3, t] = rng.uniform(-0.5, 0.5, 3) + [0.4, 0.0, 0.3]
        pose[3:, t] = q.reshape(9)
    return pose, vel


def test_compute_errors_with_the_packed_rows_equals_the_plain_formula_exactly():
    c = _cfg(px_ref=0.37, vy_ref=-0.03)
    pose, vel = _logs(31)
    a = analysis.compute_errors(pose, vel, c["coeffs"], c["t_ee"], c["px_ref"], c["vy_ref"])
    b = analysis.compute_errors(pose, vel, c["coeffs"], c["t_ee"], c["px_ref"], c["vy_ref"], yref=reference.packed_rows(c, 31))
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_compute_errors_against_a_literal_restatement_on_a_curved_schedule():
    c = _cfg(reference_schedule=SERP)
    T = c["Nsim"] + 1
    pose, vel = _logs(T, seed=8)
    y = reference.log_rows(c) + np.random.default_rng(1).uniform(-0.1, 0.1, (T, 5))     # every column of the reference moves
    got = analysis.errors_rows(analysis.compute_errors(pose, vel, c["coeffs"], c["t_ee"], c["px_ref"], c["vy_ref"], yref=y))
    a, b, cc, d, e, f = c["coeffs"]
    tee = np.asarray(c["t_ee"])
    for t in range(T):
        p, R, v, w = pose[:3, t], pose[3:, t].reshape(3, 3), vel[:3, t], vel[3:, t]
        tw = R @ tee
        X, Y, Z = p + tw
        vt = R @ (v + w @ tw)                                                 # the reference's :317 form, kept as it is
        n = np.array([2 * a * X + cc * Y + d, 2 * b * Y + cc * X + e, -1.0])
        n /= np.linalg.norm(n)
        S = a * X * X + b * Y * Y + cc * X * Y + d * X + e * Y + f
        want = [(S - Z) - y[t, 0], y[t, 1] - n @ R[:, 2], R[0, 1] - y[t, 2], y[t, 3] - X, y[t, 4] - vt[1], Z, p[1]]
        np.testing.assert_allclose(got[:, t], want, rtol=0, atol=1e-12, err_msg=f"column {t}")
    with pytest.raises(ValueError):
        analysis.compute_errors(pose, vel, c["coeffs"], c["t_ee"], c["px_ref"], c["vy_ref"], yref=y[:-1])


def test_simulator_fallbacks_measure_against_the_schedule():
    """Simulator.errors without device-logged rows, the runner-output completion and get_data()."""
    from robotic_mpc_amd import distributed
    from robotic_mpc_amd.simulator import Simulator

    raw = config.base_params(reference_schedule=SERP, prediction_horizon=12, simulation_time=0.3 + 1e-9)
    sim = Simulator(**raw)
    c, T = sim.resolved, sim.Nsim + 1
    pose, vel = _logs(T, seed=5)
    rec = dict(z=np.zeros((12, T)), u=np.zeros((6, T)), ee_pose=pose, ee_rpy=np.zeros((3, T)), ee_vel=vel,
               sqp_iter=np.ones(T - 1, int), qp_iter=np.ones(T - 1, int), status=np.zeros(T - 1, int), residuals=np.zeros((T - 1, 4)),
               solver_time=np.zeros(T - 1), cost=np.zeros(T - 1))
    sim._attach(rec)
    want = analysis.compute_errors(pose, vel, c["coeffs"], c["t_ee"], c["px_ref"], c["vy_ref"], yref=reference.log_rows(c))
    for k in want:
        np.testing.assert_array_equal(sim.errors[k], want[k], err_msg=k)
    assert np.abs(sim.errors["e5"] - analysis.compute_errors(pose, vel, c["coeffs"], c["t_ee"], c["px_ref"], c["vy_ref"])["e5"]).max() > 1e-3
    np.testing.assert_array_equal(sim.get_data()["reference_schedule"], reference.log_rows(c))
    assert "reference_schedule" not in _plain_data()
    local = {k: v[None] for k, v in rec.items() if k not in ("sqp_iter", "qp_iter", "status")}
    local.update(status=rec["status"][None], sqp_iter=rec["sqp_iter"][None], qp_iter=rec["qp_iter"][None])
    done = distributed.complete_runner_output(local, [c])
    np.testing.assert_array_equal(done["errors"][0], analysis.errors_rows(want))


def _plain_data():
    from robotic_mpc_amd.simulator import Simulator

    sim = Simulator(**config.base_params(prediction_horizon=12, simulation_time=0.05 + 1e-9))
    T = sim.Nsim + 1
    pose, vel = _logs(T)
    sim._attach(dict(z=np.zeros((12, T)), u=np.zeros((6, T)), ee_pose=pose, ee_rpy=np.zeros((3, T)), ee_vel=vel,
                     sqp_iter=np.ones(T - 1, int), qp_iter=np.ones(T - 1, int), status=np.zeros(T - 1, int),
                     residuals=np.zeros((T - 1, 4)), solver_time=np.zeros(T - 1), cost=np.zeros(T - 1)))
    return sim.get_data()
