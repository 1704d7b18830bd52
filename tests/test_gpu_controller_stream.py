"""The controller step on the throughput engine (mpcb_setup_controller_on(MPCB_ENGINE_STREAM), BatchController(engine="stream"))
on the GPU: both solvers with the fast path on and off, both sides of the item-parallel residual switch, a ragged batch and a batch
larger than the GPU holds wavefronts against the oracle's step-level solver on a plant that is not the engine's; the step loop over the
built-in plant against the throughput engine's rollout; the two engines against each other; a side stream; the refusals."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.gpu


def _raw(horizons, steps, seed=0, solver="SQP_RTI", fast=True):
    """bench.workload_configs's draws (BASELINE configs[1]) as raw dicts, one per horizon in `horizons`; `steps` at dt = 0.01."""
    from robotic_mpc_amd import config

    rng = np.random.default_rng(seed)
    flat = dict(a=0.0, b=0.0, c=0.0, d=0.0, e=0.0, f=0.0)
    return [config.base_params(prediction_horizon=int(N), simulation_time=0.01 * steps,
                               q_0=config.BASE_PARAMS["q_0"] + rng.uniform(-0.1, 0.1, 6), surface_coeffs=flat,
                               solver_options={"nlp_solver_type": solver}, qp_fast_path=fast) for N in horizons]


def _against_oracle(orc, rb, raw, steps, check, engine="stream", predict=True, atol=1e-9):
    """Close the loop of BatchController(raw, engine=engine) over RK4 at 80 % of the model's bandwidths plus a seeded <= 1e-3
    perturbation; simulations `check` are compared with orc.Solver fed the same states.  Returns (controller, qp_iter [steps, B])."""
    from robotic_mpc_amd import BatchController, config

    ctl = BatchController(raw, engine=engine)
    cfgs = [config.resolve_config(r) for r in raw]
    refs = {i: orc.Solver(rb, orc.make_params(cfgs[i])) for i in check}
    rng = np.random.default_rng(11)
    x = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    wcv = np.stack([c["wcv"] for c in cfgs]) * 0.8
    qp = []
    for k in range(steps):
        out = {n: t.cpu().numpy() for n, t in ctl.step(x, predict=predict).items()}
        qp.append(out["qp_iter"])
        for i in check:
            r = refs[i].step(x[i])
            where = f"step {k} sim {i} (N = {cfgs[i]['N']})"
            np.testing.assert_allclose(out["u0"][i], r["u0"], atol=atol, rtol=0, err_msg=where)
            assert (out["status"][i], out["sqp_iter"][i], out["qp_iter"][i]) == (r["status"], r["sqp_iter"], r["qp_iter"]), where
            np.testing.assert_allclose(out["residuals"][i], r["res"], atol=atol, rtol=1e-6, err_msg=where)
            if predict:
                Ni = cfgs[i]["N"]
                xr, ur, _ = refs[i].iterate()
                np.testing.assert_allclose(out["x_pred"][i][:Ni + 1], xr, atol=atol, rtol=0, err_msg=where)
                np.testing.assert_allclose(out["u_pred"][i][:Ni], ur, atol=atol, rtol=0, err_msg=where)
        assert np.isfinite(out["solver_time"]).all() and (out["solver_time"] > 0).all()
        x = np.stack([orc.plant_step(0, wcv[i], cfgs[i]["dt"], x[i], out["u0"][i]) for i in range(len(cfgs))])
        x += rng.uniform(-1e-3, 1e-3, x.shape)
    return ctl, np.array(qp)


@pytest.mark.parametrize("solver,fast", [("SQP_RTI", True), ("SQP_RTI", False), ("SQP", True), ("SQP", False)])
def test_solvers_and_fast_path_against_oracle(orc, ur10_rb, solver, fast):
    raw = _raw([100] * 8, 8, seed=1, solver=solver, fast=fast)
    ctl, _ = _against_oracle(orc, ur10_rb, raw, 8 if solver == "SQP_RTI" else 4, check=range(8))
    assert ctl.launch_info() == dict(waves_per_sim=1, pool_bytes=0, engine=1)
    assert ctl.engine.kernel_info()["vgprs"] <= 256         # two wavefronts per SIMD stay resident


@pytest.mark.parametrize("N", [245, 246])
def test_residual_items_switch_against_oracle(orc, ur10_rb, N):
    """N = 245 runs the interior-point residual pass item-parallel, N = 246 sequentially (mpc_stream.h residual_items_ok); with the
    fast path off every QP of the start-up transient runs interior-point iterations."""
    raw = _raw([N] * 2, 4, seed=2, fast=False)
    _, qp = _against_oracle(orc, ur10_rb, raw, 4, check=range(2))
    assert qp.max() >= 2


def test_ragged_batch_against_oracle(orc, ur10_rb):
    """One launch over horizons 1..60 (SQP_RTI): every simulation against the oracle at its own horizon; the prediction rows past a
    simulation's horizon are NaN."""
    horizons = list(range(1, 61))
    raw = _raw(horizons, 5, seed=3)
    ctl, _ = _against_oracle(orc, ur10_rb, raw, 5, check=range(60), engine="auto")
    assert ctl.launch_info()["engine"] == 1 and ctl.N == 60 and list(ctl.horizons) == horizons
    x0 = np.stack([np.concatenate([r["q_0"], r["qdot_0"]]) for r in raw])
    out = {n: t.cpu().numpy() for n, t in ctl.step(x0, predict=True).items()}
    assert out["x_pred"].shape == (60, 61, 12) and out["u_pred"].shape == (60, 60, 6)
    for i, Ni in enumerate(horizons):
        assert np.isfinite(out["x_pred"][i, :Ni + 1]).all() and np.isnan(out["x_pred"][i, Ni + 1:]).all(), Ni
        assert np.isfinite(out["u_pred"][i, :Ni]).all() and np.isnan(out["u_pred"][i, Ni:]).all(), Ni


def test_batch_beyond_resident_wavefronts(orc, ur10_rb):
    """4096 simulations, more than the 2048 wavefronts the GPU holds at once: every 256th against the oracle."""
    from robotic_mpc_amd import engine

    raw = _raw([100] * 4096, 3, seed=4)
    ctl, _ = _against_oracle(orc, ur10_rb, raw, 3, check=list(range(0, 4096, 256)))
    assert ctl.launch_info()["engine"] == 1
    assert engine.controller_engine_for(4096, 100, lib=ctl.engine.lib) == 1      # and "auto" would have chosen it too


def test_step_loop_over_builtin_plant_equals_stream_rollout(orc, ur10, monkeypatch):
    """32 simulations of configs[1] x 600 steps: the stream controller closed over the built-in plant (orc.plant_step on the host)
    equals MpcBatchEngine.run of the same configurations on the throughput engine."""
    import bench

    from robotic_mpc_amd import BatchController, engine

    cfgs = bench.workload_configs(32, 100, 6.0, seed=0, solver="SQP_RTI")
    raw = _raw([100] * 32, 600, seed=0)
    monkeypatch.setenv("MPCB_ENGINE", "stream")
    e = engine.MpcBatchEngine(0)
    roll = e.run(cfgs, ur10)
    assert e.launch_info()["engine"] == 1
    e.close()
    monkeypatch.delenv("MPCB_ENGINE")
    ctl = BatchController(raw, engine="stream")
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


def test_engines_agree(orc):
    """The same uniform batch on both engines, fed the same states for 20 steps."""
    from robotic_mpc_amd import BatchController, config

    raw = _raw([60] * 48, 20, seed=5)
    lat, stm = BatchController(raw, engine="latency"), BatchController(raw, engine="stream")
    assert (lat.launch_info()["engine"], stm.launch_info()["engine"]) == (0, 1)
    cfgs = [config.resolve_config(r) for r in raw]
    x = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    wcv = np.stack([c["wcv"] for c in cfgs]) * 0.8
    for k in range(20):
        a = {n: t.cpu().numpy() for n, t in lat.step(x, predict=True).items()}
        b = {n: t.cpu().numpy() for n, t in stm.step(x, predict=True).items()}
        for n in ("u0", "x_pred", "u_pred", "residuals", "cost"):
            np.testing.assert_allclose(b[n], a[n], atol=1e-9, rtol=1e-9, err_msg=f"step {k} {n}")
        for n in ("status", "sqp_iter", "qp_iter"):
            np.testing.assert_array_equal(b[n], a[n], err_msg=f"step {k} {n}")
        x = np.stack([orc.plant_step(0, wcv[i], cfgs[i]["dt"], x[i], a["u0"][i]) for i in range(len(cfgs))])


def test_non_default_stream_and_reset():
    """A step on a side stream gives what the same step gives on the default stream, bit for bit; reset() restarts the sequence."""
    import torch

    from robotic_mpc_amd import BatchController

    raw = _raw([20, 35, 50, 50] * 4, 10, seed=6)
    x0 = torch.tensor(np.stack([np.concatenate([r["q_0"], r["qdot_0"]]) for r in raw]), dtype=torch.float64, device="cuda:0")
    xs = [x0 + 1e-3 * k for k in range(4)]
    ctl = BatchController(raw, engine="stream")
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
                assert torch.equal(a[n].nan_to_num(7.0), b[n].nan_to_num(7.0)), n


def test_refusals_on_the_device(ur10):
    import torch

    from robotic_mpc_amd import config, engine

    dp = C.POINTER(C.c_double)
    cfgs = [config.resolve_config(r) for r in _raw([20] * 4, 5, seed=7)]
    e = engine.MpcBatchEngine(0)
    pb, params, robot = e.prepare(cfgs, ur10)
    ragged = params.copy()
    ragged[1, 65] = 10
    setup = lambda p, prm, eng: e.lib.mpcb_setup_controller_on(e._h, C.byref(p), prm.ctypes.data_as(dp), robot.ctypes.data_as(dp), eng)
    assert setup(pb, ragged, 0) == -1                         # ragged on the latency engine
    assert setup(pb, params, 7) == -1                         # unknown engine
    pb32, _, _ = e.prepare(cfgs, ur10)
    pb32.precision = 1
    for eng in (-1, 0, 1):
        assert setup(pb32, params, eng) == -1                 # fp32 Riccati on every engine
    pbs, _, _ = e.prepare(cfgs, ur10)
    pbs.solver_type = 0
    assert setup(pbs, ragged, 1) == -1                        # ragged full SQP
    assert setup(pb, ragged, 1) == 0                          # ragged SQP_RTI on the throughput engine
    assert e.lib.mpcb_engine(e._h) == 1
    bufs = e.alloc_results(pb)
    e._pb = pb
    for call in (lambda: e.rollout(bufs, 0, 5), lambda: e.summary(bufs)):
        with pytest.raises(engine.EngineError, match=r"\(-5\)"):
            call()
    e.setup(cfgs, ur10)                                       # set up for rollouts: step is refused
    io = {n: torch.zeros((4,) + shp(20), dtype=torch.float64 if ty == "f8" else torch.int32, device="cuda:0")
          for n, ty, shp in engine.STEP_FIELDS}
    with pytest.raises(engine.EngineError, match=r"\(-5\)"):
        e.step(io)
    e.close()
