"""Rollouts over a perturbed plant on the GPU (mpcb_rollout_pert; the configuration key plant_perturbation), on both engines.  The
yardstick is what defines the perturbed rollout: BatchController stepped from the NOISY state with the window of each step
(yref = sched[:, t : t + N], a new reference every step) over a plant on the host (orc.plant_step) that has the PLANT's bandwidths,
starts from the TRUE state and gets the disturbed input -- the loop test_gpu_rollout_ref.py closes over the nominal plant.

Inputs: that file's draws (flat surface, q_0 jitter +-0.1, px_ref jitter, the 2-lane serpentine); on top, per simulation, a
bandwidth scale in [0.7, 1.2] (wcv dt = 2.0 here and RK4 is stable below 2.785), Gaussian measurement noise with sigma_q = 1e-3 and
sigma_qdot = 1e-2, and a step disturbance of 0.05 rad/s from one third of the run on.  Every test asserts from the reference loop
alone that every step has status 0 and that each active perturbation moves z by more than 1e-4, before it compares."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu

SERP = {"kind": "serpentine", "lanes": 2, "lane_pitch": 0.03, "lane_time": 0.04, "turn_time": 0.05}
# the bounds of tests/golden/make_golden.py rti_tight_bounds, from rest (test_gpu_rollout_ref.py)
TIGHT = dict(qdot_min=[-0.8] * 6, qdot_max=[0.8] * 6, qdot_0=[0.0] * 6)
INTS = ("status", "sqp_iter", "qp_iter")
ALL = ("wcv", "u_dist", "x_noise")


def _raw(n, N, steps, seed, solver="SQP_RTI", schedule=SERP, which=ALL, **kw):
    """Raw configurations: test_gpu_rollout_ref.py's draws, then -- from a generator of its own, so that those draws stay what they
    are -- the perturbation of each simulation.  `N` may be a sequence (ragged horizons); `which`: the perturbations that are on."""
    from robotic_mpc_amd import config

    rng = np.random.default_rng(seed)
    prng = np.random.default_rng([seed, 77])
    flat = dict(a=0.0, b=0.0, c=0.0, d=0.0, e=0.0, f=0.0)
    Ns = list(N) if np.ndim(N) else [N] * n
    on = which or ()
    out = []
    for i in range(n):
        q0 = config.BASE_PARAMS["q_0"] + rng.uniform(-0.1, 0.1, 6)
        px = 0.40 + rng.uniform(-0.02, 0.02)
        scale = prng.uniform(0.7, 1.2, 6)
        pert = {}
        if "wcv" in on:
            pert["wcv_scale"] = scale.tolist()
        if "u_dist" in on:
            pert["input_disturbance"] = {"kind": "step", "start_time": 0.01 * (steps // 3), "value": 0.05}
        if "x_noise" in on:
            pert["measurement_noise"] = {"kind": "gaussian", "sigma_q": 1e-3, "sigma_qdot": 1e-2, "seed": 1000 * seed + i}
        out.append(config.base_params(**{**dict(prediction_horizon=Ns[i % len(Ns)], simulation_time=0.01 * steps + 1e-9, q_0=q0, px_ref=px,
                                                surface_coeffs=flat, solver_options={"nlp_solver_type": solver},
                                                reference_schedule=schedule, plant_perturbation=pert if which is not None else None),
                                         **kw}))
    return out


def _num_cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _resolve(raw):
    from robotic_mpc_amd import config

    return [config.resolve_config(r) for r in raw]


def _nominal(cfgs):
    """The perturbation arrays that perturb nothing."""
    B, S = len(cfgs), cfgs[0]["Nsim"]
    return {"wcv": np.stack([c["wcv"] for c in cfgs]), "u_dist": np.zeros((B, S, 6)), "x_noise": np.zeros((B, S, 12))}


def _rollout(cfgs, ur10, sched, pert, splits=None):
    """One bucket through setup / rollout(yref=, pert=) / sync.  `pert`: dict of numpy arrays (members may be None or missing), or
    None for the scheduled rollout.  Returns (results as numpy, launch_info, queue_used of the last launch, kernel_info)."""
    import torch

    from robotic_mpc_amd import engine

    e = engine.MpcBatchEngine(0)
    try:
        pb = e.setup(cfgs, ur10)
        bufs = e.alloc_results(pb)
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
        yt = dev(sched)
        pt = None if pert is None else {k: dev(v) for k, v in pert.items()}
        bounds = [0] + list(splits or []) + [pb.Nsim]
        for s0, s1 in zip(bounds[:-1], bounds[1:]):
            e.rollout(bufs, s0, s1, yref=yt, pert=pt)
            e.sync()
        return {k: v.cpu().numpy() for k, v in bufs.items()}, e.launch_info(), e.queue_used(), e.kernel_info()
    finally:
        e.close()


def _step_loop(orc, raw, sched, pert, eng):
    """The reference: BatchController(raw, engine=eng) stepped from z + x_noise[t] with a new window every step, over
    orc.plant_step with the plant's bandwidths, from the true z, with the input u0 + u_dist[t]."""
    from robotic_mpc_amd import BatchController

    cfgs = _resolve(raw)
    ctl = BatchController(raw, engine=eng)
    B, S, N = len(cfgs), cfgs[0]["Nsim"], max(c["N"] for c in cfgs)
    o = dict(z=np.zeros((B, 12, S + 1)), u=np.zeros((B, 6, S + 1)), cost=np.zeros((B, S)), residuals=np.zeros((B, S, 4)),
             status=np.zeros((B, S), np.int32), sqp_iter=np.zeros((B, S), np.int32), qp_iter=np.zeros((B, S), np.int32))
    z = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    o["z"][:, :, 0] = z
    o["u"][:, :, 0] = np.stack([c["qdot0"] for c in cfgs])
    for t in range(S):
        r = {n: v.cpu().numpy() for n, v in ctl.step(z + pert["x_noise"][:, t], yref=np.ascontiguousarray(sched[:, t:t + N])).items()}
        for k in ("cost", "residuals") + INTS:
            o[k][:, t] = r[k]
        z = np.stack([orc.plant_step(c["plant_integrator"], pert["wcv"][i], c["dt"], z[i], r["u0"][i] + pert["u_dist"][i, t])
                      for i, c in enumerate(cfgs)])
        o["z"][:, :, t + 1], o["u"][:, :, t + 1] = z, r["u0"]
    o["launch_info"] = ctl.launch_info()
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


def _guards(orc, raw, sched, pert, want, eng, active=ALL, check=None):
    """From the reference loop alone: every step has status 0, and each active perturbation matters -- the loop with it switched
    off ends up more than 1e-4 away."""
    cfgs = _resolve(raw)
    idx = list(range(len(cfgs))) if check is None else list(check)
    assert (want["status"] == 0).all()
    off = _nominal(cfgs)
    for k in active:
        without = _step_loop(orc, raw, sched, {**pert, k: off[k]}, eng)
        assert np.abs(without["z"][idx] - want["z"][idx]).max() > 1e-4, k


def _case(orc, ur10, monkeypatch, eng, raw, waves, check=None, active=ALL):
    from robotic_mpc_amd import plant, reference

    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs = _resolve(raw)
    sched, pert = reference.stack(cfgs), plant.stack(cfgs)
    want = _step_loop(orc, raw, sched, pert, eng)
    _guards(orc, raw, sched, pert, want, eng, active, check)
    got, info, _, _ = _rollout(cfgs, ur10, sched, pert)
    assert (info["engine"], info["waves_per_sim"]) == ((0, waves) if eng == "latency" else (1, 1)), info
    _compare(got, want, sched, cfgs, check)
    return got, want, sched, pert, cfgs


# ------------------------------------------------------------------------------------------------------------ latency engine
@pytest.mark.parametrize("n,N,steps,waves", [(4, 12, 14, 4), (3, 100, 6, 8), (2, 224, 3, 8), (4, 12, 14, 2), (4, 12, 14, 1)])
def test_latency_engine_over_the_perturbed_plant(orc, ur10, monkeypatch, n, N, steps, waves):
    if waves < 4:      # <2> and <1>: mpcb_setup never picks them by itself
        monkeypatch.setenv("MPCB_WAVES_PER_SIM", str(waves))
    _case(orc, ur10, monkeypatch, "latency", _raw(n, N, steps, seed=1), waves)


def test_latency_engine_two_simulations_per_cu(orc, ur10, monkeypatch):
    n = _num_cus() + 64
    _case(orc, ur10, monkeypatch, "latency", _raw(n, 12, 5, seed=2), 4, check=range(0, n, 20))


def test_latency_engine_full_sqp(orc, ur10, monkeypatch):
    _case(orc, ur10, monkeypatch, "latency", _raw(3, 12, 4, seed=3, solver="SQP"), 4)


def test_tight_bounds_take_both_qp_paths(orc, ur10, monkeypatch):
    """The bounds of the rti_tight_bounds fixture: steps solved by the fast path (qp_iter 1) and by the interior point (more)."""
    _, want, _, _, _ = _case(orc, ur10, monkeypatch, "latency", _raw(4, 15, 14, seed=4, **TIGHT), 4)
    assert (want["qp_iter"] > 1).any() and (want["qp_iter"] == 1).any()


# --------------------------------------------------------------------------------------------------------- throughput engine
def test_throughput_engine_over_the_perturbed_plant(orc, ur10, monkeypatch):
    _case(orc, ur10, monkeypatch, "stream", _raw(6, 12, 14, seed=5), 1)


def test_throughput_engine_full_sqp(orc, ur10, monkeypatch):
    _case(orc, ur10, monkeypatch, "stream", _raw(3, 12, 4, seed=6, solver="SQP"), 1)


def test_throughput_engine_ragged_horizons(orc, ur10, monkeypatch):
    """Horizons {5, 9, 12} in one launch."""
    _, _, _, _, cfgs = _case(orc, ur10, monkeypatch, "stream", _raw(6, (5, 9, 12), 14, seed=7), 1)
    assert sorted({c["N"] for c in cfgs}) == [5, 9, 12]


def test_throughput_engine_work_queue_is_bit_identical_to_the_plain_launch(orc, ur10, monkeypatch):
    """Batch 8, 11 steps, 4 resident wavefronts, chunks of 3 steps: every chunk of every simulation changes hands -- and what it
    hands on is the true state."""
    from robotic_mpc_amd import plant, reference

    monkeypatch.setenv("MPCB_ENGINE", "stream")
    raw = _raw(8, 12, 11, seed=8)
    cfgs = _resolve(raw)
    sched, pert = reference.stack(cfgs), plant.stack(cfgs)
    plain, info, used, _ = _rollout(cfgs, ur10, sched, pert)
    assert info["engine"] == 1 and not used
    monkeypatch.setenv("MPCB_STREAM_SLOTS", "4")
    monkeypatch.setenv("MPCB_STREAM_CHUNK", "3")
    queued, info, used, _ = _rollout(cfgs, ur10, sched, pert)
    assert info["engine"] == 1 and used
    for k in plain:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(plain[k], queued[k], err_msg=k)
    monkeypatch.delenv("MPCB_STREAM_SLOTS")
    monkeypatch.delenv("MPCB_STREAM_CHUNK")
    want = _step_loop(orc, raw, sched, pert, "stream")
    _guards(orc, raw, sched, pert, want, "stream")
    _compare(queued, want, sched, cfgs)


# ------------------------------------------------------------------------------------------------------------- both engines
@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_launch_split_is_bit_identical(ur10, monkeypatch, eng):
    """What carries across a launch boundary is the true state; the next launch forms its feedback state from x_noise[step0]."""
    from robotic_mpc_amd import plant, reference

    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs = _resolve(_raw(4, 12, 12, seed=9))
    sched, pert = reference.stack(cfgs), plant.stack(cfgs)
    one, info, _, _ = _rollout(cfgs, ur10, sched, pert)
    assert info["engine"] == (0 if eng == "latency" else 1)
    two, _, _, _ = _rollout(cfgs, ur10, sched, pert, splits=[5])
    for k in one:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(one[k], two[k], err_msg=k)
    assert np.abs(pert["x_noise"][:, 5]).min() > 0                            # the boundary's noise row is not a zero row


@pytest.mark.parametrize("eng", ["latency", "stream"])
@pytest.mark.parametrize("only", ALL)
def test_one_perturbation_at_a_time(orc, ur10, monkeypatch, eng, only):
    """Bandwidth only, disturbance only, noise only: a swapped or ignored array fails here.  The other two members are NULL."""
    from robotic_mpc_amd import plant, reference

    monkeypatch.setenv("MPCB_ENGINE", eng)
    raw = _raw(3, 12, 8, seed=12, which=(only,))
    cfgs = _resolve(raw)
    sched, full = reference.stack(cfgs), plant.stack(cfgs)
    off = _nominal(cfgs)
    for k in ALL:
        if k != only:
            np.testing.assert_array_equal(full[k], off[k])                   # the spec switches the other two off
    want = _step_loop(orc, raw, sched, full, eng)
    _guards(orc, raw, sched, full, want, eng, active=(only,))
    got, info, _, _ = _rollout(cfgs, ur10, sched, {only: full[only]})
    assert info["engine"] == (0 if eng == "latency" else 1)
    _compare(got, want, sched, cfgs)


@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_null_cases(ur10, monkeypatch, eng):
    """pert == NULL is mpcb_rollout_ref bit for bit; all-NULL members, and scale 1 with zero tables, are its results through the
    kernels of the perturbed rollout."""
    import torch

    from robotic_mpc_amd import engine, reference

    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs = _resolve(_raw(4, 12, 14, seed=10, which=None))
    sched = reference.stack(cfgs)
    ref, info, _, kinfo = _rollout(cfgs, ur10, sched, None)
    assert info["engine"] == (0 if eng == "latency" else 1)
    # mpcb_rollout_pert(pert = NULL)
    e = engine.MpcBatchEngine(0)
    try:
        pb = e.setup(cfgs, ur10)
        bufs = e.alloc_results(pb)
        y = torch.from_numpy(sched).to("cuda:0")
        r = e._result_struct(bufs)
        assert e.lib.mpcb_rollout_pert(e._h, 0, pb.Nsim, C.byref(r), C.cast(C.c_void_p(y.data_ptr()), C.POINTER(C.c_double)), None, None) == 0
        e.sync()
        for k, v in bufs.items():
            if k not in ("solver_time", "plant_time"):
                np.testing.assert_array_equal(v.cpu().numpy(), ref[k], err_msg=k)
        assert e.kernel_info() == kinfo                                       # (and reports the scheduled path's kernel, as before)
    finally:
        e.close()
    for pert in ({}, _nominal(cfgs)):
        got, _, _, _ = _rollout(cfgs, ur10, sched, pert)
        for k in ("z", "u", "ee_pose", "ee_rpy", "ee_vel", "errors"):
            np.testing.assert_allclose(got[k], ref[k], atol=1e-9, rtol=0, err_msg=k)
        np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-9, atol=0)
        np.testing.assert_allclose(got["residuals"], ref["residuals"], atol=1e-9, rtol=1e-6)
        for k in INTS:
            np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ur10):
    import torch

    from robotic_mpc_amd import engine, plant, reference

    raw = _raw(3, 12, 6, seed=11)
    cfgs = _resolve(raw)
    y = torch.from_numpy(reference.stack(cfgs)).to("cuda:0")
    pert = {k: torch.from_numpy(v).to("cuda:0") for k, v in plant.stack(cfgs).items()}
    e = engine.MpcBatchEngine(0)
    try:
        # a controller handle
        pb = e.setup_controller(cfgs, ur10)
        bufs = e.alloc_results(pb)
        with pytest.raises(engine.EngineError, match=r"\(-5\)"):                 # MPCB_ESTATE
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pert)
        # the fp32 leg
        fp32 = _resolve(_raw(3, 12, 6, seed=11, schedule=None, which=None, riccati_precision="fp32"))
        e.setup(fp32, ur10)
        with pytest.raises(engine.EngineError, match=r"\(-1\)"):                 # MPCB_EINVAL
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pert)
        # a perturbation without a schedule, at the C level
        e.setup(cfgs, ur10)
        r = e._result_struct(bufs)
        p = engine.MpcbPlantPert()
        assert e.lib.mpcb_rollout_pert(e._h, 0, pb.Nsim, C.byref(r), None, C.byref(p), None) == -1
        # wrong shapes never reach the library (the handle's error text stays that of the call above)
        before = e.lib.mpcb_last_error(e._h)
        with pytest.raises(ValueError, match="x_noise"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert={**pert, "x_noise": pert["x_noise"][:, :-1].contiguous()})
        with pytest.raises(ValueError, match="u_dist"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert={**pert, "u_dist": pert["x_noise"]})
        with pytest.raises(ValueError, match="wcv"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert={**pert, "wcv": pert["wcv"].float()})
        with pytest.raises(ValueError, match="yref"):
            e.rollout(bufs, 0, pb.Nsim, pert=pert)
        assert e.lib.mpcb_last_error(e._h) == before
        # ... and the handle still runs
        e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pert)
        e.sync()
        assert (bufs["status"].cpu().numpy() == 0).all()
    finally:
        e.close()
    with pytest.raises(ValueError, match="plant perturbation"):
        engine.MpcBatchEngine(0).run_host_buffers(_resolve(_raw(3, 12, 6, seed=11, schedule=None)), ur10)


# ----------------------------------------------------------------------------------------------------------- public interface
def test_grid_search_over_the_perturbation_through_run_all(ur10, monkeypatch, tmp_path):
    """plant_perturbation.wcv_scale x plant_perturbation.measurement_noise.seed x prediction_horizon through SimulationManager,
    without a schedule (the packed rows): one ragged perturbed bucket on the throughput engine, results in queue order, the realised
    tables in `data`, the device summary against the host formula over the logged columns, checkpoint and resume."""
    from robotic_mpc_amd import SimulationManager, analysis, base_params, packing, plant

    monkeypatch.setattr(packing, "RAGGED_MIN_BATCH", 4)
    noise = {"kind": "gaussian", "sigma_q": 1e-3, "sigma_qdot": 1e-2, "seed": 0}
    base = base_params(simulation_time=0.14 + 1e-9, prediction_horizon=12,
                       plant_perturbation={"wcv_scale": 1.0, "input_disturbance": {"kind": "step", "start_time": 0.04, "value": 0.05},
                                           "measurement_noise": noise})
    grid = {"plant_perturbation.wcv_scale": [0.8, 1.2], "plant_perturbation.measurement_noise.seed": [0, 1], "prediction_horizon": [8, 12]}
    path = str(tmp_path / "grid.npz")
    m = SimulationManager(base)
    m.grid_search(grid)
    assert base["plant_perturbation"]["measurement_noise"]["seed"] == 0 and base["plant_perturbation"]["wcv_scale"] == 1.0
    res = m.run_all(checkpoint=path)
    assert m.last_run_info["buckets"] == 1 and m.last_run_info["n_resumed"] == 0
    want_order = [(w, s, N) for w in (0.8, 1.2) for s in (0, 1) for N in (8, 12)]
    assert [(r["simulator"].resolved["plant_perturbation"]["wcv_scale"], r["simulator"].resolved["plant_perturbation"]["measurement_noise"]["seed"],
             r["simulator"].prediction_horizon) for r in res] == want_order
    for r in res:
        sim = r["simulator"]
        c = sim.resolved
        tables = plant.sample(c)
        np.testing.assert_array_equal(r["data"]["measurement_noise"], tables["x_noise"])
        np.testing.assert_array_equal(r["data"]["input_disturbance"], tables["u_dist"])
        assert r["data"]["measurement_noise"].shape == (14, 12) and r["data"]["input_disturbance"].shape == (14, 6)
        sm = sim.simulation_model
        e = analysis.compute_errors(sm._ee_pose_log, sm._ee_velocity_log, c["coeffs"], c["t_ee"], c["px_ref"], c["vy_ref"])
        for k in ("e1", "e2", "e3", "e4", "e5"):
            np.testing.assert_allclose(sim.errors[k], e[k], atol=1e-12, rtol=0, err_msg=k)
            assert abs(r["summary"][f"rmse_{k}"] - np.sqrt(np.mean(e[k] ** 2))) < 1e-12, k
    # the seed matters, and so does the bandwidth
    assert np.abs(res[1]["data"]["q"] - res[3]["data"]["q"]).max() > 1e-4
    assert np.abs(res[1]["data"]["q"] - res[5]["data"]["q"]).max() > 1e-4
    # resume: nothing runs again
    m2 = SimulationManager(base)
    m2.grid_search(grid)
    again = m2.run_all(checkpoint=path)
    assert m2.last_run_info["n_resumed"] == 8
    for a, b in zip(res, again):
        for k in ("q", "qdot", "u", "measurement_noise"):
            np.testing.assert_array_equal(a["data"][k], b["data"][k])
        np.testing.assert_array_equal(a["simulator"].errors["e5"], b["simulator"].errors["e5"])
