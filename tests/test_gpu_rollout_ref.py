"""Rollouts that track a task reference schedule on the GPU (mpcb_rollout_ref; the configuration key reference_schedule), on both
engines.  The yardstick is what defines the scheduled rollout: BatchController stepped with the window of each step
(yref = sched[:, t : t + N], a new reference every step) over the built-in plant on the host (orc.plant_step), as
test_gpu_controller.py::test_step_loop_over_builtin_plant_equals_rollout closes the plain loop -- the controller step itself is held
to dense references by test_gpu_dense_qp.py and test_gpu_controller_reference.py.

The schedule of every tracking case is one serpentine (2 lanes, pitch 0.03, lane 0.04 s, turn 0.05 s at dt = 0.01): the turn
begins at row 4 and v_y's target changes sign at row 7.  Runs of 11 steps and more contain the sign change in their logged columns;
the runs of 3 to 6 steps that the long horizons and the large batch can afford contain it in the rows they read (run + horizon) --
both are asserted, each where it holds."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

SERP = {"kind": "serpentine", "lanes": 2, "lane_pitch": 0.03, "lane_time": 0.04, "turn_time": 0.05}
# the bounds of tests/golden/make_golden.py rti_tight_bounds, from rest: the first steps' QPs stay inside them (the fast path, qp_iter 1),
# the later ones run into them (interior point).  With that fixture's qdot_0 every QP of a 40-step run has active bounds.
TIGHT = dict(qdot_min=[-0.8] * 6, qdot_max=[0.8] * 6, qdot_0=[0.0] * 6)
INTS = ("status", "sqp_iter", "qp_iter")


def _raw(n, N, steps, seed, solver="SQP_RTI", schedule=SERP, **kw):
    """Raw configurations: test_gpu_controller.py's draws (flat surface, q_0 jitter) with a per-simulation px_ref jitter, so that the
    schedule rows differ between the simulations.  `N` may be a sequence (ragged horizons)."""
    from robotic_mpc_amd import config

    rng = np.random.default_rng(seed)
    flat = dict(a=0.0, b=0.0, c=0.0, d=0.0, e=0.0, f=0.0)
    Ns = list(N) if np.ndim(N) else [N] * n
    out = []
    for i in range(n):
        q0 = config.BASE_PARAMS["q_0"] + rng.uniform(-0.1, 0.1, 6)
        px = 0.40 + rng.uniform(-0.02, 0.02)
        out.append(config.base_params(**{**dict(prediction_horizon=Ns[i % len(Ns)], simulation_time=0.01 * steps + 1e-9, q_0=q0, px_ref=px,
                                                surface_coeffs=flat, solver_options={"nlp_solver_type": solver},
                                                reference_schedule=schedule), **kw}))
    return out


def _num_cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _resolve(raw):
    from robotic_mpc_amd import config

    return [config.resolve_config(r) for r in raw]


def _rollout(cfgs, ur10, sched="own", splits=None):
    """One bucket through setup / rollout(yref=) / sync; `sched`: "own" the configurations' schedules, None none, or an array
    [B, Nsim + N, 5].  `splits`: launch boundaries.  Returns (results as numpy, launch_info, queue_used of the last launch)."""
    import torch

    from robotic_mpc_amd import engine, reference

    e = engine.MpcBatchEngine(0)
    try:
        pb = e.setup(cfgs, ur10)
        bufs = e.alloc_results(pb)
        y = reference.stack(cfgs) if isinstance(sched, str) else sched
        yt = None if y is None else torch.from_numpy(np.ascontiguousarray(y)).to("cuda:0")
        bounds = [0] + list(splits or []) + [pb.Nsim]
        for s0, s1 in zip(bounds[:-1], bounds[1:]):
            e.rollout(bufs, s0, s1, yref=yt)
            e.sync()
        return {k: v.cpu().numpy() for k, v in bufs.items()}, e.launch_info(), e.queue_used()
    finally:
        e.close()


_LOOPS = {}


def _step_loop(orc, raw, sched, eng, key=None):
    """The reference: BatchController(raw, engine=eng) with a new window every step over orc.plant_step.  `sched` None: the packed
    references.  Computed once per `key` and shared."""
    if key is not None and key in _LOOPS:
        return _LOOPS[key]
    from robotic_mpc_amd import BatchController

    cfgs = _resolve(raw)
    ctl = BatchController(raw, engine=eng)
    B, S, N = len(cfgs), cfgs[0]["Nsim"], max(c["N"] for c in cfgs)
    o = dict(z=np.zeros((B, 12, S + 1)), u=np.zeros((B, 6, S + 1)), cost=np.zeros((B, S)), residuals=np.zeros((B, S, 4)),
             status=np.zeros((B, S), np.int32), sqp_iter=np.zeros((B, S), np.int32), qp_iter=np.zeros((B, S), np.int32))
    x = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    o["z"][:, :, 0] = x
    o["u"][:, :, 0] = np.stack([c["qdot0"] for c in cfgs])
    for t in range(S):
        y = None if sched is None else np.ascontiguousarray(sched[:, t:t + N])
        r = {n: v.cpu().numpy() for n, v in ctl.step(x, yref=y).items()}
        for k in ("cost", "residuals") + INTS:
            o[k][:, t] = r[k]
        x = np.stack([orc.plant_step(c["plant_integrator"], c["wcv"], c["dt"], x[i], r["u0"][i]) for i, c in enumerate(cfgs)])
        o["z"][:, :, t + 1], o["u"][:, :, t + 1] = x, r["u0"]
    o["launch_info"] = ctl.launch_info()
    if key is not None:
        _LOOPS[key] = o
    return o


def _compare(got, want, sched, cfgs, check=None):
    from robotic_mpc_amd import analysis

    idx = list(range(len(cfgs))) if check is None else list(check)
    S = cfgs[0]["Nsim"]
    np.testing.assert_allclose(got["z"][idx], want["z"][idx], atol=1e-9, rtol=0)
    np.testing.assert_allclose(got["u"][idx], want["u"][idx], atol=1e-9, rtol=0)
    np.testing.assert_allclose(got["cost"][idx], want["cost"][idx], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["residuals"][idx], want["residuals"][idx], atol=1e-9, rtol=1e-6)
    for k in INTS:
        np.testing.assert_array_equal(got[k][idx], want[k][idx], err_msg=k)
    for i in idx:
        c = cfgs[i]
        e = analysis.errors_rows(analysis.compute_errors(got["ee_pose"][i], got["ee_vel"][i], c["coeffs"], c["t_ee"], c["px_ref"], c["vy_ref"],
                                                         yref=sched[i, :S + 1]))
        np.testing.assert_allclose(got["errors"][i], e, atol=1e-12, rtol=0, err_msg=f"errors of simulation {i}")
    assert np.isfinite(got["solver_time"]).all() and (got["solver_time"] > 0).all()


def _guards(orc, raw, sched, want, eng, logged_sign_change, check=None):
    """From the reference loop alone: the schedule matters (the packed-reference loop ends up elsewhere), v_y's target changes sign."""
    cfgs = _resolve(raw)
    S, N = cfgs[0]["Nsim"], max(c["N"] for c in cfgs)
    packed = _step_loop(orc, raw, None, eng)
    idx = list(range(len(cfgs))) if check is None else list(check)
    assert np.abs(packed["z"][idx] - want["z"][idx]).max() > 1e-4
    rows = S + 1 if logged_sign_change else S + min(c["N"] for c in cfgs)
    for i in idx:
        vy = sched[i, :rows, 4]
        assert (vy > 0).any() and (vy < 0).any(), i
    assert np.abs(sched[idx[0]] - sched[idx[-1]]).max() > 1e-4              # the rows differ between simulations


def _tracking_case(orc, ur10, monkeypatch, eng, raw, waves, logged_sign_change, check=None):
    from robotic_mpc_amd import reference

    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs = _resolve(raw)
    sched = reference.stack(cfgs)
    want = _step_loop(orc, raw, sched, eng)
    _guards(orc, raw, sched, want, eng, logged_sign_change, check)
    got, info, _ = _rollout(cfgs, ur10)
    assert (info["engine"], info["waves_per_sim"]) == ((0, waves) if eng == "latency" else (1, 1)), info
    _compare(got, want, sched, cfgs, check)
    return got, want, sched, cfgs


# ------------------------------------------------------------------------------------------------------------ latency engine
@pytest.mark.parametrize("n,N,steps,waves,logged", [(4, 12, 14, 4, True), (3, 100, 6, 8, False), (2, 224, 3, 8, False),
                                                    (4, 12, 14, 2, True), (4, 12, 14, 1, True)])
def test_latency_engine_tracks_the_schedule(orc, ur10, monkeypatch, n, N, steps, waves, logged):
    if waves < 4:      # <2> and <1>: mpcb_setup never picks them by itself
        monkeypatch.setenv("MPCB_WAVES_PER_SIM", str(waves))
    _tracking_case(orc, ur10, monkeypatch, "latency", _raw(n, N, steps, seed=1), waves, logged)


def test_latency_engine_two_simulations_per_cu(orc, ur10, monkeypatch):
    n = _num_cus() + 64
    _tracking_case(orc, ur10, monkeypatch, "latency", _raw(n, 12, 5, seed=2), 4, False, check=range(0, n, 20))


def test_latency_engine_full_sqp(orc, ur10, monkeypatch):
    _tracking_case(orc, ur10, monkeypatch, "latency", _raw(3, 12, 4, seed=3, solver="SQP"), 4, False)


def test_tight_bounds_take_both_qp_paths(orc, ur10, monkeypatch):
    """The bounds of the rti_tight_bounds fixture: steps solved by the fast path (qp_iter 1) and by the interior point (more)."""
    _, want, _, _ = _tracking_case(orc, ur10, monkeypatch, "latency", _raw(4, 15, 14, seed=4, **TIGHT), 4, True)
    assert (want["qp_iter"] > 1).any() and (want["qp_iter"] == 1).any()


# --------------------------------------------------------------------------------------------------------- throughput engine
def test_throughput_engine_tracks_the_schedule(orc, ur10, monkeypatch):
    _tracking_case(orc, ur10, monkeypatch, "stream", _raw(6, 12, 14, seed=5), 1, True)


def test_throughput_engine_full_sqp(orc, ur10, monkeypatch):
    _tracking_case(orc, ur10, monkeypatch, "stream", _raw(3, 12, 4, seed=6, solver="SQP"), 1, False)


def test_throughput_engine_ragged_horizons_never_read_past_their_own(orc, ur10, monkeypatch):
    """Horizons {5, 9, 12} in one launch; the rows a simulation never reads -- past Nsim + N_i -- are NaN in the copy of the
    schedule the rollout gets: it must not matter."""
    from robotic_mpc_amd import reference

    raw = _raw(6, (5, 9, 12), 14, seed=7)
    got, want, sched, cfgs = _tracking_case(orc, ur10, monkeypatch, "stream", raw, 1, True)
    poisoned = sched.copy()
    for i, c in enumerate(cfgs):
        poisoned[i, c["Nsim"] + c["N"]:] = np.nan
    assert np.isnan(poisoned).any()
    again, info, _ = _rollout(cfgs, ur10, sched=poisoned)
    assert info["engine"] == 1
    for k in got:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(got[k], again[k], err_msg=k)
    # ... and the reference loop, whose windows hold NaN in the rows past each simulation's own horizon
    loop = _step_loop(orc, raw, _windows_with_nan(sched, cfgs), "stream")
    np.testing.assert_array_equal(loop["z"], want["z"])


class _windows_with_nan:
    """sched[:, t : t + N] with the rows k >= N_i of simulation i's window set to NaN."""

    def __init__(self, sched, cfgs):
        self.sched, self.cfgs = sched, cfgs

    def __getitem__(self, key):
        w = self.sched[key].copy()
        for i, c in enumerate(self.cfgs):
            w[i, c["N"]:] = np.nan
        return w


def test_throughput_engine_work_queue_is_bit_identical_to_the_plain_launch(orc, ur10, monkeypatch):
    """Batch 8, 11 steps, 4 resident wavefronts, chunks of 3 steps: every chunk of every simulation changes hands."""
    from robotic_mpc_amd import reference

    monkeypatch.setenv("MPCB_ENGINE", "stream")
    raw = _raw(8, 12, 11, seed=8)
    cfgs = _resolve(raw)
    sched = reference.stack(cfgs)
    plain, info, used = _rollout(cfgs, ur10)
    assert info["engine"] == 1 and not used
    monkeypatch.setenv("MPCB_STREAM_SLOTS", "4")
    monkeypatch.setenv("MPCB_STREAM_CHUNK", "3")
    queued, info, used = _rollout(cfgs, ur10)
    assert info["engine"] == 1 and used
    for k in plain:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(plain[k], queued[k], err_msg=k)
    want = _step_loop(orc, raw, sched, "stream")
    _guards(orc, raw, sched, want, "stream", True)
    _compare(queued, want, sched, cfgs)


# ------------------------------------------------------------------------------------------------------------- both engines
@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_launch_split_is_bit_identical(ur10, monkeypatch, eng):
    """Every step linearises from the stored iterate, so nothing depends on the launch boundary."""
    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs = _resolve(_raw(4, 12, 12, seed=9))
    one, info, _ = _rollout(cfgs, ur10)
    assert info["engine"] == (0 if eng == "latency" else 1)
    two, _, _ = _rollout(cfgs, ur10, splits=[5])
    for k in one:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(one[k], two[k], err_msg=k)


@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_constant_schedule_gives_the_plain_rollout(ur10, monkeypatch, eng):
    """A schedule equal to the packed row on every row: the results of mpcb_rollout (another pass order, so not the same bits)."""
    from robotic_mpc_amd import reference

    monkeypatch.setenv("MPCB_ENGINE", eng)
    plain_cfgs = _resolve(_raw(4, 12, 14, seed=10, schedule=None))
    raw = _raw(4, 12, 14, seed=10, schedule=None)
    for r, c in zip(raw, plain_cfgs):
        r["reference_schedule"] = {"kind": "table", "rows": reference.packed_rows(c, c["Nsim"] + c["N"]).tolist()}
    cfgs = _resolve(raw)
    plain, _, _ = _rollout(plain_cfgs, ur10, sched=None)
    got, _, _ = _rollout(cfgs, ur10)
    for k in ("z", "u", "ee_pose", "ee_rpy", "ee_vel", "errors", "cost", "residuals"):
        np.testing.assert_allclose(got[k], plain[k], atol=1e-9, rtol=0, err_msg=k)
    for k in INTS:
        np.testing.assert_array_equal(got[k], plain[k], err_msg=k)


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_and_null_schedule(ur10):
    import torch

    from robotic_mpc_amd import config, engine, reference

    raw = _raw(3, 12, 6, seed=11)
    cfgs = _resolve(raw)
    y = torch.from_numpy(reference.stack(cfgs)).to("cuda:0")
    e = engine.MpcBatchEngine(0)
    # a controller handle
    pb = e.setup_controller(cfgs, ur10)
    bufs = e.alloc_results(pb)
    with pytest.raises(engine.EngineError, match=r"\(-5\)"):                 # MPCB_ESTATE
        e.rollout(bufs, 0, pb.Nsim, yref=y)
    # the fp32 leg
    fp32 = _resolve(_raw(3, 12, 6, seed=11, schedule=None, riccati_precision="fp32"))
    e.setup(fp32, ur10)
    with pytest.raises(engine.EngineError, match=r"\(-1\)"):                 # MPCB_EINVAL
        e.rollout(bufs, 0, pb.Nsim, yref=y)
    e.rollout(bufs, 0, pb.Nsim)                                              # the handle still runs the fp32 rollout
    e.sync()
    with pytest.raises(ValueError):                                          # a wrong shape never reaches the library
        e.setup(cfgs, ur10)
        e.rollout(bufs, 0, pb.Nsim, yref=y[:, :-1].contiguous())
    # mpcb_rollout_ref(NULL) is mpcb_rollout
    e.setup(cfgs, ur10)
    e.rollout(bufs, 0, pb.Nsim)
    e.sync()
    a = {k: v.clone() for k, v in bufs.items()}
    r = e._result_struct(bufs)
    assert e.lib.mpcb_rollout_ref(e._h, 0, pb.Nsim, C.byref(r), None, None) == 0
    e.sync()
    for k in a:
        if k not in ("solver_time", "plant_time"):
            assert torch.equal(a[k], bufs[k]), k
    e.close()
    with pytest.raises(ValueError, match="reference schedule"):
        engine.MpcBatchEngine(0).run_host_buffers(cfgs, ur10)


# ----------------------------------------------------------------------------------------------------------- public interface
def test_grid_search_over_the_schedule_through_run_all(ur10, monkeypatch, tmp_path):
    """reference_schedule.lane_time x prediction_horizon through SimulationManager: one ragged scheduled bucket on the throughput
    engine, results in queue order, the device summary against the host formula over the logged columns, checkpoint and resume."""
    from robotic_mpc_amd import SimulationManager, analysis, base_params, packing, reference

    monkeypatch.setattr(packing, "RAGGED_MIN_BATCH", 4)
    base = base_params(simulation_time=0.14 + 1e-9, prediction_horizon=12, reference_schedule=SERP)
    grid = {"reference_schedule.lane_time": [0.04, 0.08], "prediction_horizon": [8, 12]}
    path = str(tmp_path / "grid.npz")
    m = SimulationManager(base)
    m.grid_search(grid)
    res = m.run_all(checkpoint=path)
    assert m.last_run_info["buckets"] == 1 and m.last_run_info["n_resumed"] == 0
    assert [(r["simulator"].resolved["reference_schedule"]["lane_time"], r["simulator"].prediction_horizon) for r in res] == \
        [(0.04, 8), (0.04, 12), (0.08, 8), (0.08, 12)]
    for r in res:
        sim = r["simulator"]
        c = sim.resolved
        rows = reference.log_rows(c)
        np.testing.assert_array_equal(r["data"]["reference_schedule"], rows)
        sm = sim.simulation_model
        e = analysis.compute_errors(sm._ee_pose_log, sm._ee_velocity_log, c["coeffs"], c["t_ee"], c["px_ref"], c["vy_ref"], yref=rows)
        for j, k in enumerate(("e1", "e2", "e3", "e4", "e5")):
            np.testing.assert_allclose(sim.errors[k], e[k], atol=1e-12, rtol=0, err_msg=k)
            assert abs(r["summary"][f"rmse_{k}"] - np.sqrt(np.mean(e[k] ** 2))) < 1e-12, k
    # the lane time matters, and so does the schedule
    assert np.abs(res[1]["data"]["q"] - res[3]["data"]["q"]).max() > 1e-4
    # resume: nothing runs again
    m2 = SimulationManager(base)
    m2.grid_search(grid)
    again = m2.run_all(checkpoint=path)
    assert m2.last_run_info["n_resumed"] == 4
    for a, b in zip(res, again):
        for k in ("q", "qdot", "u"):
            np.testing.assert_array_equal(a["data"][k], b["data"][k])
        np.testing.assert_array_equal(a["simulator"].errors["e5"], b["simulator"].errors["e5"])
