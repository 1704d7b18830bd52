"""The controller step on the GPU (mpcb_setup_controller / mpcb_step, BatchController): every shipped geometry against the
oracle's step-level solver on a plant that is not the engine's, the step loop over the built-in plant against
MpcBatchEngine.run, a batch above the throughput engine's threshold, a non-default stream, and the call-order refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


def _raw(n, N, steps, seed=0, solver="SQP_RTI", fast=True):
    """bench.workload_configs (BASELINE configs[1]'s draws) as the raw dicts BatchController takes; `steps` at dt = 0.01."""
    from robotic_mpc_amd import config

    rng = np.random.default_rng(seed)
    flat = dict(a=0.0, b=0.0, c=0.0, d=0.0, e=0.0, f=0.0)
    return [config.base_params(prediction_horizon=N, simulation_time=0.01 * steps, q_0=config.BASE_PARAMS["q_0"] + rng.uniform(-0.1, 0.1, 6),
                               surface_coeffs=flat, solver_options={"nlp_solver_type": solver}, qp_fast_path=fast) for _ in range(n)]


def _num_cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _check_against_oracle(orc, ur10_rb, raw, steps, check, predict=True, atol=1e-9):
    """Close the loop of BatchController(raw) over RK4 at 80 % of the model's bandwidths plus a seeded <= 1e-3 perturbation;
    simulations `check` are compared with orc.Solver fed the same states.  Returns the controller."""
    from robotic_mpc_amd import BatchController, config

    ctl = BatchController(raw)
    cfgs = [config.resolve_config(r) for r in raw]
    refs = {i: orc.Solver(ur10_rb, orc.make_params(cfgs[i])) for i in check}
    rng = np.random.default_rng(11)
    x = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    for k in range(steps):
        out = {n: t.cpu().numpy() for n, t in ctl.step(x, predict=predict).items()}
        for i in check:
            r = refs[i].step(x[i])
            where = f"step {k} sim {i}"
            np.testing.assert_allclose(out["u0"][i], r["u0"], atol=atol, rtol=0, err_msg=where)
            assert (out["status"][i], out["sqp_iter"][i], out["qp_iter"][i]) == (r["status"], r["sqp_iter"], r["qp_iter"]), where
            np.testing.assert_allclose(out["residuals"][i], r["res"], atol=atol, rtol=1e-6, err_msg=where)
            if predict:
                xr, ur, _ = refs[i].iterate()
                np.testing.assert_allclose(out["x_pred"][i], xr, atol=atol, rtol=0, err_msg=where)
                np.testing.assert_allclose(out["u_pred"][i], ur, atol=atol, rtol=0, err_msg=where)
        assert np.isfinite(out["solver_time"]).all() and (out["solver_time"] > 0).all()
        wcv = np.stack([c["wcv"] for c in cfgs]) * 0.8
        x = np.stack([orc.plant_step(0, wcv[i], cfgs[i]["dt"], x[i], out["u0"][i]) for i in range(len(cfgs))])
        x += rng.uniform(-1e-3, 1e-3, x.shape)
    return ctl


@pytest.mark.parametrize("solver,fast", [("SQP_RTI", True), ("SQP_RTI", False), ("SQP", True), ("SQP", False)])
def test_geometry_8_1_against_oracle(orc, ur10_rb, solver, fast):
    raw = _raw(min(8, _num_cus()), 100, 8, seed=1, solver=solver, fast=fast)
    ctl = _check_against_oracle(orc, ur10_rb, raw, 8 if solver == "SQP_RTI" else 4, check=range(len(raw)))
    assert ctl.launch_info() == dict(ctl.launch_info(), waves_per_sim=8, engine=0)


def test_geometry_4_1_against_oracle(orc, ur10_rb):
    raw = _raw(6, 40, 10, seed=2)
    ctl = _check_against_oracle(orc, ur10_rb, raw, 10, check=range(6))
    info = ctl.launch_info()
    assert (info["waves_per_sim"], info["engine"]) == (4, 0)


def test_geometry_4_2_against_oracle(orc, ur10_rb):
    raw = _raw(320, 100, 5, seed=3)
    check = list(range(0, 320, 20))
    ctl = _check_against_oracle(orc, ur10_rb, raw, 5, check=check)
    info = ctl.launch_info()
    assert (info["waves_per_sim"], info["engine"]) == (4, 0)
    assert ctl.engine.kernel_info()["vgprs"] <= 256         # two simulations per CU: the 256-register build


def test_segment_sweeps_against_oracle(orc, ur10_rb):
    raw = _raw(4, 224, 3, seed=4)
    ctl = _check_against_oracle(orc, ur10_rb, raw, 3, check=range(4))
    info = ctl.launch_info()
    assert (info["waves_per_sim"], info["engine"]) == (8, 0)


def test_batch_above_stream_threshold_runs_on_latency_engine(orc, ur10_rb):
    from robotic_mpc_amd import engine

    raw = _raw(1536, 100, 4, seed=5)
    lib = engine.load_library()
    assert engine.engine_for(1536, 100, 4, "SQP_RTI", lib=lib) == 1      # a rollout of this bucket would take the throughput engine
    ctl = _check_against_oracle(orc, ur10_rb, raw, 4, check=list(range(0, 1536, 192)), predict=False)
    assert ctl.launch_info()["engine"] == 0


def test_step_loop_over_builtin_plant_equals_rollout(orc, ur10):
    """32 simulations of configs[1] x 600 steps: the step API closed over the built-in plant (orc.plant_step on the host)
    equals MpcBatchEngine.run on the same configurations."""
    import bench

    from robotic_mpc_amd import BatchController, engine

    cfgs = bench.workload_configs(32, 100, 6.0, seed=0, solver="SQP_RTI")
    raw = _raw(32, 100, 600, seed=0)
    e = engine.MpcBatchEngine(0)
    roll = e.run(cfgs, ur10)
    e.close()
    ctl = BatchController(raw)
    B, S = 32, cfgs[0]["Nsim"]
    z = np.zeros((B, 12, S + 1)); u = np.zeros((B, 6, S + 1))
    st, sq, qp = (np.zeros((B, S), np.int32) for _ in range(3))
    x = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    z[:, :, 0] = x
    u[:, :, 0] = np.stack([c["qdot0"] for c in cfgs])
    for k in range(S):
        o = {n: t.cpu().numpy() for n, t in ctl.step(x).items()}
        st[:, k], sq[:, k], qp[:, k] = o["status"], o["sqp_iter"], o["qp_iter"]
        x = np.stack([orc.plant_step(0, c["wcv"], c["dt"], x[i], o["u0"][i]) for i, c in enumerate(cfgs)])
        z[:, :, k + 1], u[:, :, k + 1] = x, o["u0"]
    np.testing.assert_allclose(z, roll["z"], atol=1e-9, rtol=0)
    np.testing.assert_allclose(u, roll["u"], atol=1e-9, rtol=0)
    for name, v in (("status", st), ("sqp_iter", sq), ("qp_iter", qp)):
        np.testing.assert_array_equal(v, roll[name], err_msg=name)


def test_non_default_stream_and_reset(ur10):
    """A step on a side stream gives what the same step gives on the default stream; reset() restarts the sequence."""
    import torch

    from robotic_mpc_amd import BatchController

    raw = _raw(16, 50, 10, seed=6)
    x0 = torch.tensor(np.stack([np.concatenate([r["q_0"], r["qdot_0"]]) for r in raw]), dtype=torch.float64, device="cuda:0")
    xs = [x0 + 1e-3 * k for k in range(4)]
    ctl = BatchController(raw)
    ref = [{n: t.clone() for n, t in ctl.step(x, predict=True).items()} for x in xs]
    ctl.reset()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = [{n: t.clone() for n, t in ctl.step(x, predict=True).items()} for x in xs]
    side.synchronize()
    for a, b in zip(ref, got):
        for n in a:
            if n != "solver_time":
                assert torch.equal(a[n], b[n]), n
    lean = BatchController(raw)
    lean.step(x0)
    assert "x_pred" not in lean._bufs and "u_pred" not in lean._bufs     # prediction buffers only once a step asks for them
    with pytest.raises(ValueError):
        ctl.step(x0.float())
    with pytest.raises(ValueError):
        ctl.step(x0[:, :6])
    with pytest.raises(ValueError):
        ctl.step(x0.cpu())


def test_call_order_refusals(ur10):
    from robotic_mpc_amd import engine, config

    cfgs = [config.resolve_config(r) for r in _raw(4, 20, 5, seed=7)]
    e = engine.MpcBatchEngine(0)
    e.setup_controller(cfgs, ur10)
    bufs = e.alloc_results(e._pb)
    for call in (lambda: e.rollout(bufs, 0, 5), lambda: e.summary(bufs)):
        with pytest.raises(engine.EngineError, match=r"\(-5\)"):
            call()
    e.setup(cfgs, ur10)                                       # set up for rollouts again: rollout works, step is refused
    e.rollout(bufs, 0, 5)
    e.sync()
    import torch

    io = {n: torch.zeros((4,) + shp(20), dtype=torch.float64 if ty == "f8" else torch.int32, device="cuda:0")
          for n, ty, shp in engine.STEP_FIELDS}
    with pytest.raises(engine.EngineError, match=r"\(-5\)"):
        e.step(io)
    # the controller refuses ragged horizons and fp32 Riccati (MPCB_EINVAL)
    pb, params, robot = e.prepare(cfgs, ur10)
    params[1, 65] = 10
    assert e.lib.mpcb_setup_controller(e._h, C.byref(pb), params.ctypes.data_as(C.POINTER(C.c_double)),
                                       robot.ctypes.data_as(C.POINTER(C.c_double))) == -1
    pb32, params32, _ = e.prepare(cfgs, ur10)
    pb32.precision = 1
    assert e.lib.mpcb_setup_controller(e._h, C.byref(pb32), params32.ctypes.data_as(C.POINTER(C.c_double)),
                                       robot.ctypes.data_as(C.POINTER(C.c_double))) == -1
    e.close()
