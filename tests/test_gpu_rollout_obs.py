"""Rollouts with an on-device disturbance observer on the GPU (mpcb_rollout_obs; the configuration key disturbance_observer), on both
engines.  The yardstick is what defines this rollout: the BatchController loop of test_gpu_rollout_pert.py::_step_loop, over the same
perturbed plant on the host, whose step t is ctl.step(z_t + noise_t, yref = sched[:, t : t + N], dist = d_hat_t) with d_hat_t from
the torch DisturbanceObserver (robotic_mpc_amd/observer.py) that measured z_t + noise_t and the commanded u_{t-1}.  Compared at
_compare's tolerances of that file -- atol 1e-9 on the logs, rtol 1e-9 on the cost, atol 1e-9 with rtol 1e-6 on the residuals -- and
atol 1e-9 on d_hat.

Inputs: that file's draws and perturbations (bandwidth scale, Gaussian noise, a step disturbance of 0.05 rad/s from one third of the
run on); the poles alternate 0 (deadbeat) and 0.2 over the simulations.  Every test that compares first asserts from the reference
loop alone that every step has status 0, that d_hat leaves zero and that the loop without the observer ends up more than 1e-4 away
in z."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_rollout_pert as tp  # noqa: E402

pytestmark = pytest.mark.gpu
INTS = tp.INTS
POLES = (0.0, 0.2)
_dp = C.POINTER(C.c_double)


def _raw(n, N, steps, seed, **kw):
    raw = tp._raw(n, N, steps, seed=seed, **kw)
    for i, r in enumerate(raw):
        r["disturbance_observer"] = {"pole": POLES[i % 2]}
    return raw


def _rollout(cfgs, ur10, sched, pert, gain, splits=None):
    """One bucket through setup / rollout(yref=, pert=, obs=) / sync.  `gain` [B, 12] (None: no obs=).  Returns (results as numpy,
    d_hat among them, launch_info, queue_used of the last launch, kernel_info)."""
    import torch

    from robotic_mpc_amd import engine

    e = engine.MpcBatchEngine(0)
    try:
        pb = e.setup(cfgs, ur10)
        bufs = e.alloc_results(pb)
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
        yt = dev(sched)
        pt = None if pert is None else {k: dev(v) for k, v in pert.items()}
        ot = None if gain is None else {"gain": dev(gain), "d_hat": torch.full((pb.batch, pb.Nsim, 6), float("nan"), dtype=torch.float64,
                                                                                device="cuda:0")}
        bounds = [0] + list(splits or []) + [pb.Nsim]
        for s0, s1 in zip(bounds[:-1], bounds[1:]):
            e.rollout(bufs, s0, s1, yref=yt, pert=pt, obs=ot)
            e.sync()
        out = {k: v.cpu().numpy() for k, v in bufs.items()}
        if ot is not None:
            out["d_hat"] = ot["d_hat"].cpu().numpy()
        return out, e.launch_info(), e.queue_used(), e.kernel_info()
    finally:
        e.close()


def _step_loop(orc, raw, sched, pert, eng, observer=True):
    """The reference: test_gpu_rollout_pert._step_loop with dist = d_hat_t of the torch observer at every step (observer False:
    without an estimate)."""
    import torch

    from robotic_mpc_amd import BatchController
    from robotic_mpc_amd.observer import DisturbanceObserver

    cfgs = tp._resolve(raw)
    ctl = BatchController(raw, engine=eng)
    B, S, N = len(cfgs), cfgs[0]["Nsim"], max(c["N"] for c in cfgs)
    obs = [DisturbanceObserver(c["wcv"], c["dt"], c["disturbance_observer"]["pole"]) for c in cfgs]
    o = dict(z=np.zeros((B, 12, S + 1)), u=np.zeros((B, 6, S + 1)), cost=np.zeros((B, S)), residuals=np.zeros((B, S, 4)),
             status=np.zeros((B, S), np.int32), sqp_iter=np.zeros((B, S), np.int32), qp_iter=np.zeros((B, S), np.int32),
             d_hat=np.zeros((B, S, 6)))
    z = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    o["z"][:, :, 0] = z
    o["u"][:, :, 0] = np.stack([c["qdot0"] for c in cfgs])
    u_prev = np.zeros((B, 6))
    for t in range(S):
        xhat = z + pert["x_noise"][:, t]
        kw = {}
        if observer:
            d = np.stack([ob.update(torch.from_numpy(xhat[i:i + 1]), torch.from_numpy(u_prev[i:i + 1])).numpy()[0] for i, ob in enumerate(obs)])
            o["d_hat"][:, t] = d
            kw["dist"] = np.ascontiguousarray(d)
        r = {n: v.cpu().numpy() for n, v in ctl.step(xhat, yref=np.ascontiguousarray(sched[:, t:t + N]), **kw).items()}
        for k in ("cost", "residuals") + INTS:
            o[k][:, t] = r[k]
        z = np.stack([orc.plant_step(c["plant_integrator"], pert["wcv"][i], c["dt"], z[i], r["u0"][i] + pert["u_dist"][i, t])
                      for i, c in enumerate(cfgs)])
        o["z"][:, :, t + 1], o["u"][:, :, t + 1] = z, r["u0"]
        u_prev = r["u0"].copy()
    return o


def _inputs(raw):
    """(cfgs, sched, the plant's arrays for the loop, pert for the rollout (None: nominal), gain [B, 12])."""
    from robotic_mpc_amd import observer, plant, reference

    cfgs = tp._resolve(raw)
    perturbed = cfgs[0]["plant_perturbation"] is not None
    arrays = plant.stack(cfgs) if perturbed else tp._nominal(cfgs)
    return cfgs, reference.stack(cfgs), arrays, (arrays if perturbed else None), observer.stack(cfgs)


def _guards(orc, raw, sched, arrays, want, eng, check=None):
    """From the reference loop alone: every step has status 0, the estimate leaves zero, and it matters."""
    idx = list(range(len(raw))) if check is None else list(check)
    assert (want["status"] == 0).all()
    assert (want["d_hat"][:, 0] == 0).all() and (np.abs(want["d_hat"][idx, -1]).max(axis=1) > 1e-3).all()
    without = _step_loop(orc, raw, sched, arrays, eng, observer=False)
    assert np.abs(without["z"][idx] - want["z"][idx]).max() > 1e-4


def _compare(got, want, sched, cfgs, check=None):
    idx = list(range(len(cfgs))) if check is None else list(check)
    tp._compare(got, want, sched, cfgs, check)
    np.testing.assert_allclose(got["d_hat"][idx], want["d_hat"][idx], atol=1e-9, rtol=0)


def _case(orc, ur10, monkeypatch, eng, raw, waves, check=None):
    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs, sched, arrays, pert, gain = _inputs(raw)
    want = _step_loop(orc, raw, sched, arrays, eng)
    _guards(orc, raw, sched, arrays, want, eng, check)
    got, info, _, _ = _rollout(cfgs, ur10, sched, pert, gain)
    assert (info["engine"], info["waves_per_sim"]) == ((0, waves) if eng == "latency" else (1, 1)), info
    _compare(got, want, sched, cfgs, check)
    return got, want, cfgs


# ------------------------------------------------------------------------------------------------------------ latency engine
@pytest.mark.parametrize("n,N,steps,waves", [(4, 12, 14, 4), (3, 100, 6, 8), (2, 224, 3, 8), (4, 12, 14, 2), (4, 12, 14, 1)])
def test_latency_engine_with_an_observer_over_the_perturbed_plant(orc, ur10, monkeypatch, n, N, steps, waves):
    if waves < 4:      # <2> and <1>: mpcb_setup never picks them by itself
        monkeypatch.setenv("MPCB_WAVES_PER_SIM", str(waves))
    # (in the runs of 3 and 6 steps the estimate leaves zero through the noise and the bandwidth mismatch: the guard holds there too)
    _case(orc, ur10, monkeypatch, "latency", _raw(n, N, steps, seed=1), waves)


def test_latency_engine_two_simulations_per_cu(orc, ur10, monkeypatch):
    n = tp._num_cus() + 64
    _case(orc, ur10, monkeypatch, "latency", _raw(n, 12, 5, seed=2), 4, check=range(0, n, 20))


def test_tight_bounds_take_both_qp_paths(orc, ur10, monkeypatch):
    """The bounds of the rti_tight_bounds fixture: steps solved by the fast path (qp_iter 1) and by the interior point (more)."""
    _, want, _ = _case(orc, ur10, monkeypatch, "latency", _raw(4, 15, 14, seed=4, **tp.TIGHT), 4)
    assert (want["qp_iter"] > 1).any() and (want["qp_iter"] == 1).any()


# --------------------------------------------------------------------------------------------------------- throughput engine
def test_throughput_engine_with_an_observer(orc, ur10, monkeypatch):
    _case(orc, ur10, monkeypatch, "stream", _raw(6, 12, 14, seed=5), 1)


def test_throughput_engine_ragged_horizons(orc, ur10, monkeypatch):
    """Horizons {5, 9, 12} in one launch."""
    _, _, cfgs = _case(orc, ur10, monkeypatch, "stream", _raw(6, (5, 9, 12), 14, seed=7), 1)
    assert sorted({c["N"] for c in cfgs}) == [5, 9, 12]


def test_throughput_engine_horizon_of_one(orc, ur10, monkeypatch):
    _case(orc, ur10, monkeypatch, "stream", _raw(3, 1, 10, seed=6), 1)


def test_throughput_engine_work_queue_is_bit_identical_to_the_plain_launch(orc, ur10, monkeypatch):
    """Batch 8, 11 steps, 4 resident wavefronts, chunks of 3 steps: every chunk of every simulation changes hands, and the estimate
    travels with the true state."""
    monkeypatch.setenv("MPCB_ENGINE", "stream")
    raw = _raw(8, 12, 11, seed=8)
    cfgs, sched, arrays, pert, gain = _inputs(raw)
    plain, info, used, _ = _rollout(cfgs, ur10, sched, pert, gain)
    assert info["engine"] == 1 and not used
    monkeypatch.setenv("MPCB_STREAM_SLOTS", "4")
    monkeypatch.setenv("MPCB_STREAM_CHUNK", "3")
    queued, info, used, _ = _rollout(cfgs, ur10, sched, pert, gain)
    assert info["engine"] == 1 and used
    for k in plain:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(plain[k], queued[k], err_msg=k)
    monkeypatch.delenv("MPCB_STREAM_SLOTS")
    monkeypatch.delenv("MPCB_STREAM_CHUNK")
    want = _step_loop(orc, raw, sched, arrays, "stream")
    _guards(orc, raw, sched, arrays, want, "stream")
    _compare(queued, want, sched, cfgs)


# ------------------------------------------------------------------------------------------------------------- both engines
@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_launch_split_is_bit_identical(ur10, monkeypatch, eng):
    """Split at steps 5 and 9 of 12, the disturbance acting from step 4 on: the estimate that crosses each boundary is not zero."""
    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs, sched, _, pert, gain = _inputs(_raw(4, 12, 12, seed=9))
    one, info, _, _ = _rollout(cfgs, ur10, sched, pert, gain)
    assert info["engine"] == (0 if eng == "latency" else 1)
    assert (np.abs(one["d_hat"][:, 5]).max(axis=1) > 0).all() and (np.abs(one["d_hat"][:, 9]).max(axis=1) > 1e-3).all()
    two, _, _, _ = _rollout(cfgs, ur10, sched, pert, gain, splits=[5, 9])
    for k in one:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(one[k], two[k], err_msg=k)


@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_null_cases(ur10, monkeypatch, eng):
    """obs_gain == NULL is mpcb_rollout_pert bit for bit, on its kernels; l2 = 0 keeps d_hat at zero and gives its results through
    the kernels of this rollout."""
    import torch

    from robotic_mpc_amd import engine

    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs, sched, _, pert, gain = _inputs(_raw(4, 12, 14, seed=10))
    ref, info, _, kinfo = tp._rollout(cfgs, ur10, sched, pert)
    assert info["engine"] == (0 if eng == "latency" else 1)
    e = engine.MpcBatchEngine(0)
    try:
        pb = e.setup(cfgs, ur10)
        bufs = e.alloc_results(pb)
        keep = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (sched, pert["wcv"], pert["u_dist"], pert["x_noise"])]
        dh = torch.full((pb.batch, pb.Nsim, 6), 7.0, dtype=torch.float64, device="cuda:0")
        ptr = [C.cast(C.c_void_p(t.data_ptr()), _dp) for t in keep + [dh]]
        p = engine.MpcbPlantPert(ptr[1], ptr[2], ptr[3])
        r = e._result_struct(bufs)
        assert e.lib.mpcb_rollout_obs(e._h, 0, pb.Nsim, C.byref(r), ptr[0], C.byref(p), None, ptr[4], None) == 0
        e.sync()
        for k, v in bufs.items():
            if k not in ("solver_time", "plant_time"):
                np.testing.assert_array_equal(v.cpu().numpy(), ref[k], err_msg=k)
        assert e.kernel_info() == kinfo                                       # (the perturbed rollout's kernel)
        assert (dh.cpu().numpy() == 7.0).all()                                # d_hat is ignored
    finally:
        e.close()
    g0 = gain.copy()
    g0[:, 6:] = 0.0
    got, _, _, kobs = _rollout(cfgs, ur10, sched, pert, g0)
    assert (got["d_hat"] == 0).all()
    for k in ("z", "u", "ee_pose", "ee_rpy", "ee_vel", "errors"):
        np.testing.assert_allclose(got[k], ref[k], atol=1e-9, rtol=0, err_msg=k)
    np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["residuals"], ref["residuals"], atol=1e-9, rtol=1e-6)
    for k in INTS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert kobs["vgprs"] > 0                                                  # (this rollout's kernel reports itself)


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ur10):
    import torch

    from robotic_mpc_amd import engine

    raw = _raw(3, 12, 6, seed=11)
    cfgs, sched, _, pert, gain = _inputs(raw)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
    y = dev(sched)
    pt = {k: dev(v) for k, v in pert.items()}
    ot = {"gain": dev(gain), "d_hat": torch.zeros((3, 6, 6), dtype=torch.float64, device="cuda:0")}
    e = engine.MpcBatchEngine(0)
    try:
        # a controller handle
        pb = e.setup_controller(cfgs, ur10)
        bufs = e.alloc_results(pb)
        with pytest.raises(engine.EngineError, match=r"\(-5\)"):                 # MPCB_ESTATE
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, obs=ot)
        # the fp32 leg
        e.setup(tp._resolve(tp._raw(3, 12, 6, seed=11, schedule=None, which=None, riccati_precision="fp32")), ur10)
        with pytest.raises(engine.EngineError, match=r"\(-1\).*fp64"):           # MPCB_EINVAL
            e.rollout(bufs, 0, pb.Nsim, yref=y, obs=ot)
        # full SQP
        e.setup(tp._resolve(tp._raw(3, 12, 6, seed=11, solver="SQP")), ur10)
        with pytest.raises(engine.EngineError, match=r"\(-1\).*SQP_RTI"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, obs=ot)
        # a gain without d_hat, and without a schedule, at the C level
        e.setup(cfgs, ur10)
        r = e._result_struct(bufs)
        yp, gp, dp = (C.cast(C.c_void_p(t.data_ptr()), _dp) for t in (y, ot["gain"], ot["d_hat"]))
        assert e.lib.mpcb_rollout_obs(e._h, 0, pb.Nsim, C.byref(r), yp, None, gp, None, None) == -1
        assert b"d_hat" in e.lib.mpcb_last_error(e._h)
        assert e.lib.mpcb_rollout_obs(e._h, 0, pb.Nsim, C.byref(r), None, None, gp, dp, None) == -1
        assert b"schedule" in e.lib.mpcb_last_error(e._h)
        # the step-range rules of mpcb_rollout
        assert e.lib.mpcb_rollout_obs(e._h, 2, pb.Nsim, C.byref(r), yp, None, gp, dp, None) == -5
        assert e.lib.mpcb_rollout_obs(e._h, 0, pb.Nsim + 1, C.byref(r), yp, None, gp, dp, None) == -1
        # wrong shapes never reach the library (the handle's error text stays that of the call above)
        before = e.lib.mpcb_last_error(e._h)
        with pytest.raises(ValueError, match="d_hat"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, obs={**ot, "d_hat": ot["d_hat"][:, :-1].contiguous()})
        with pytest.raises(ValueError, match="gain"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, obs={**ot, "gain": ot["gain"].float()})
        with pytest.raises(ValueError, match="d_hat"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, obs={**ot, "d_hat": ot["d_hat"].cpu()})
        with pytest.raises(ValueError, match="keys"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, obs={"gain": ot["gain"]})
        with pytest.raises(ValueError, match="yref"):
            e.rollout(bufs, 0, pb.Nsim, pert=pt, obs=ot)
        assert e.lib.mpcb_last_error(e._h) == before
        # ... and the handle still runs
        e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, obs=ot)
        e.sync()
        assert (bufs["status"].cpu().numpy() == 0).all() and np.abs(ot["d_hat"].cpu().numpy()).max() > 0
    finally:
        e.close()


# ----------------------------------------------------------------------------------------------------------- public interface
def test_grid_over_the_pole_through_run_all(ur10):
    """A 4-point grid over disturbance_observer.pole through SimulationManager.run_all over a disturbed plant: one bucket, results in
    queue order, get_data()["d_hat"] [6, Nsim] that starts at zero, moves, differs from pole to pole, and is the replay of the torch
    observer on the logged states and inputs (no measurement noise here: the log is what the observer measured)."""
    import torch

    from robotic_mpc_amd import SimulationManager, base_params
    from robotic_mpc_amd.observer import DisturbanceObserver

    base = base_params(simulation_time=0.14 + 1e-9, prediction_horizon=12, solver_options={"nlp_solver_type": "SQP_RTI"},
                       plant_perturbation={"wcv_scale": 0.8, "input_disturbance": {"kind": "step", "start_time": 0.03, "value": 0.05}},
                       disturbance_observer={"pole": 0.5})
    poles = [0.0, 0.2, 0.5, 0.8]
    m = SimulationManager(base)
    m.grid_search({"disturbance_observer.pole": poles})
    res = m.run_all()
    assert m.last_run_info["buckets"] == 1 and base["disturbance_observer"] == {"pole": 0.5}
    assert [r["simulator"].resolved["disturbance_observer"]["pole"] for r in res] == poles
    for r, pole in zip(res, poles):
        sim, d = r["simulator"], r["data"]["d_hat"]
        assert d.shape == (6, 14) and (d[:, 0] == 0).all() and np.abs(d[:, -1]).max() > 1e-3
        assert (sim.solver_status == 0).all()
        np.testing.assert_array_equal(sim.get_data()["d_hat"], d)
        ob = DisturbanceObserver(sim.resolved["wcv"], sim.dt, pole)
        z, u = sim.simulation_model.z, sim.simulation_model.u
        for t in range(14):
            x = torch.from_numpy(np.ascontiguousarray(z[:, t])[None])
            up = torch.from_numpy(np.ascontiguousarray(u[:, t])[None]) if t else torch.zeros(1, 6, dtype=torch.float64)
            np.testing.assert_allclose(ob.update(x, up).numpy()[0], d[:, t], atol=1e-9, rtol=0, err_msg=f"pole {pole} step {t}")
    assert np.abs(res[0]["data"]["d_hat"] - res[3]["data"]["d_hat"]).max() > 1e-3
    assert np.abs(res[0]["data"]["q"] - res[3]["data"]["q"]).max() > 1e-6
