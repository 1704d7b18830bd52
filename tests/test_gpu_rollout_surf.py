"""Rollouts over a scheduled, stage-varying surface on the GPU (mpcb_rollout_surf; the configuration key surface_schedule), on both
engines.  The yardstick is what defines this rollout: the BatchController loop of test_gpu_rollout_pert.py::_step_loop, over the same
perturbed plant on the host, whose step t is ctl.step(z_t + noise_t, yref = sched[:, t : t + N], surface = surf[:, t : t + N]).
Compared at _compare's tolerances of that file -- atol 1e-9 on the logs, rtol 1e-9 on the cost, atol 1e-9 with rtol 1e-6 on the
residuals -- with the error log recomputed on the host from surface row t and reference row t (atol 1e-12).

Inputs: that file's draws and perturbations; on top, per simulation, a surface table whose rows vary curvature (a, b, c), slope
(d, e) and height (f) smoothly (tests/step_surf_cases.py variation).  Every test that compares first asserts from the reference loop
alone that every step has status 0 and that the loop on the constant surface ends up more than 1e-4 away in z."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import step_surf_cases as ss  # noqa: E402
import test_gpu_rollout_pert as tp  # noqa: E402

pytestmark = pytest.mark.gpu
INTS = tp.INTS
_dp = C.POINTER(C.c_double)


def _raw(n, N, steps, seed, constant=False, **kw):
    """tp._raw with a table of Nsim + N_i rows per simulation: its own (flat) coefficients plus the seeded variation (constant: the
    packed coefficients on every row)."""
    raw = tp._raw(n, N, steps, seed=seed, **kw)
    for i, r in enumerate(raw):
        rows = steps + int(r["prediction_horizon"])
        base = np.array([r["surface_coeffs"][k] for k in "abcdef"])
        tab = np.tile(base, (rows, 1)) if constant else base[None] + ss.variation(rows, 2000 + 10 * seed + i)
        r["surface_schedule"] = {"kind": "table", "rows": tab.tolist()}
    return raw


def _rollout(cfgs, ur10, sched, pert, surf, splits=None):
    """One bucket through setup / rollout(yref=, pert=, surf=) / sync.  Returns (results as numpy, launch_info, queue_used of the
    last launch, kernel_info)."""
    import torch

    from robotic_mpc_amd import engine

    e = engine.MpcBatchEngine(0)
    try:
        pb = e.setup(cfgs, ur10)
        bufs = e.alloc_results(pb)
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
        yt, st = dev(sched), dev(surf)
        pt = None if pert is None else {k: dev(v) for k, v in pert.items()}
        bounds = [0] + list(splits or []) + [pb.Nsim]
        for s0, s1 in zip(bounds[:-1], bounds[1:]):
            e.rollout(bufs, s0, s1, yref=yt, pert=pt, surf=st)
            e.sync()
        return {k: v.cpu().numpy() for k, v in bufs.items()}, e.launch_info(), e.queue_used(), e.kernel_info()
    finally:
        e.close()


def _step_loop(orc, raw, sched, pert, surf, eng):
    """The reference: test_gpu_rollout_pert._step_loop with surface = window t of the table at every step (surf None: the constant
    surface, the plain step)."""
    from robotic_mpc_amd import BatchController

    cfgs = tp._resolve(raw)
    ctl = BatchController([{k: v for k, v in r.items() if k != "surface_schedule"} for r in raw], engine=eng)
    B, S, N = len(cfgs), cfgs[0]["Nsim"], max(c["N"] for c in cfgs)
    o = dict(z=np.zeros((B, 12, S + 1)), u=np.zeros((B, 6, S + 1)), cost=np.zeros((B, S)), residuals=np.zeros((B, S, 4)),
             status=np.zeros((B, S), np.int32), sqp_iter=np.zeros((B, S), np.int32), qp_iter=np.zeros((B, S), np.int32))
    z = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    o["z"][:, :, 0] = z
    o["u"][:, :, 0] = np.stack([c["qdot0"] for c in cfgs])
    for t in range(S):
        kw = {} if surf is None else dict(surface=np.ascontiguousarray(surf[:, t:t + N]))
        r = {n: v.cpu().numpy() for n, v in ctl.step(z + pert["x_noise"][:, t], yref=np.ascontiguousarray(sched[:, t:t + N]), **kw).items()}
        for k in ("cost", "residuals") + INTS:
            o[k][:, t] = r[k]
        z = np.stack([orc.plant_step(c["plant_integrator"], pert["wcv"][i], c["dt"], z[i], r["u0"][i] + pert["u_dist"][i, t])
                      for i, c in enumerate(cfgs)])
        o["z"][:, :, t + 1], o["u"][:, :, t + 1] = z, r["u0"]
    ctl.close()
    return o


def _inputs(raw):
    """(cfgs, sched, the plant's arrays for the loop, pert for the rollout (None: nominal), surf [B, Nsim + Nmax, 6])."""
    from robotic_mpc_amd import plant, reference, surface

    cfgs = tp._resolve(raw)
    perturbed = cfgs[0]["plant_perturbation"] is not None
    arrays = plant.stack(cfgs) if perturbed else tp._nominal(cfgs)
    return cfgs, reference.stack(cfgs), arrays, (arrays if perturbed else None), surface.stack(cfgs)


def _guards(orc, raw, sched, arrays, want, eng, check=None):
    """From the reference loop alone: every step has status 0, and the schedule matters."""
    idx = list(range(len(raw))) if check is None else list(check)
    assert (want["status"] == 0).all()
    without = _step_loop(orc, raw, sched, arrays, None, eng)
    if max(int(r["prediction_horizon"]) for r in raw) == 1:
        # a horizon of one has a single task residual, at stage 0, whose state is pinned to the feedback state: the surface cannot
        # reach u0, so z is the constant surface's exactly -- what the schedule moves there is the cost (about dt w r1 dr1 ~ 1e-4 .. 1e-3)
        assert np.abs(without["z"][idx] - want["z"][idx]).max() == 0.0
        assert np.abs(without["cost"][idx] - want["cost"][idx]).max() > 1e-5
        return
    assert np.abs(without["z"][idx] - want["z"][idx]).max() > 1e-4


def _compare(got, want, sched, surf, cfgs, check=None):
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
        e = analysis.errors_rows(analysis.compute_errors(got["ee_pose"][i], got["ee_vel"][i], surf[i, :S + 1].T, c["t_ee"], c["px_ref"],
                                                         c["vy_ref"], yref=sched[i, :S + 1]))
        np.testing.assert_allclose(got["errors"][i], e, atol=1e-12, rtol=0, err_msg=f"errors of simulation {i}")
    assert np.isfinite(got["solver_time"]).all() and (got["solver_time"] > 0).all()


def _case(orc, ur10, monkeypatch, eng, raw, waves, check=None):
    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs, sched, arrays, pert, surf = _inputs(raw)
    assert (np.ptp(surf[:, :, :5], axis=1).max(axis=0) > 1e-3).all()     # curvature and slope move, not only f
    want = _step_loop(orc, raw, sched, arrays, surf, eng)
    _guards(orc, raw, sched, arrays, want, eng, check)
    got, info, _, _ = _rollout(cfgs, ur10, sched, pert, surf)
    assert (info["engine"], info["waves_per_sim"]) == ((0, waves) if eng == "latency" else (1, 1)), info
    _compare(got, want, sched, surf, cfgs, check)
    return got, want, cfgs


# ------------------------------------------------------------------------------------------------------------ latency engine
@pytest.mark.parametrize("n,N,steps,waves", [(4, 12, 14, 4), (3, 100, 6, 8), (2, 224, 3, 8), (4, 12, 14, 2), (4, 12, 14, 1)])
def test_latency_engine_over_a_scheduled_surface(orc, ur10, monkeypatch, n, N, steps, waves):
    if waves < 4:      # <2> and <1>: mpcb_setup never picks them by itself
        monkeypatch.setenv("MPCB_WAVES_PER_SIM", str(waves))
    _case(orc, ur10, monkeypatch, "latency", _raw(n, N, steps, seed=1), waves)


def test_latency_engine_two_simulations_per_cu(orc, ur10, monkeypatch):
    n = tp._num_cus() + 64
    _case(orc, ur10, monkeypatch, "latency", _raw(n, 12, 5, seed=2), 4, check=range(0, n, 20))


def test_tight_bounds_take_both_qp_paths(orc, ur10, monkeypatch):
    """The bounds of the rti_tight_bounds fixture: steps solved by the fast path (qp_iter 1) and by the interior point (more)."""
    _, want, _ = _case(orc, ur10, monkeypatch, "latency", _raw(4, 15, 14, seed=4, **tp.TIGHT), 4)
    assert (want["qp_iter"] > 1).any() and (want["qp_iter"] == 1).any()


# --------------------------------------------------------------------------------------------------------- throughput engine
def test_throughput_engine_over_a_scheduled_surface(orc, ur10, monkeypatch):
    _case(orc, ur10, monkeypatch, "stream", _raw(6, 12, 14, seed=5), 1)


def test_throughput_engine_ragged_horizons(orc, ur10, monkeypatch):
    """Horizons {5, 9, 12} in one launch: tables strided by the longest, every simulation reads the rows of its own."""
    _, _, cfgs = _case(orc, ur10, monkeypatch, "stream", _raw(6, (5, 9, 12), 14, seed=7), 1)
    assert sorted({c["N"] for c in cfgs}) == [5, 9, 12]


def test_throughput_engine_horizon_of_one(orc, ur10, monkeypatch):
    _case(orc, ur10, monkeypatch, "stream", _raw(3, 1, 10, seed=6), 1)


def test_throughput_engine_work_queue_is_bit_identical_to_the_plain_launch(orc, ur10, monkeypatch):
    """Batch 8, 11 steps, 4 resident wavefronts, chunks of 3 steps: every chunk of every simulation changes hands; the row index is
    the absolute step number whichever wavefront runs the chunk."""
    monkeypatch.setenv("MPCB_ENGINE", "stream")
    raw = _raw(8, 12, 11, seed=8)
    cfgs, sched, arrays, pert, surf = _inputs(raw)
    plain, info, used, _ = _rollout(cfgs, ur10, sched, pert, surf)
    assert info["engine"] == 1 and not used
    monkeypatch.setenv("MPCB_STREAM_SLOTS", "4")
    monkeypatch.setenv("MPCB_STREAM_CHUNK", "3")
    queued, info, used, _ = _rollout(cfgs, ur10, sched, pert, surf)
    assert info["engine"] == 1 and used
    for k in plain:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(plain[k], queued[k], err_msg=k)
    monkeypatch.delenv("MPCB_STREAM_SLOTS")
    monkeypatch.delenv("MPCB_STREAM_CHUNK")
    want = _step_loop(orc, raw, sched, arrays, surf, "stream")
    _guards(orc, raw, sched, arrays, want, "stream")
    _compare(queued, want, sched, surf, cfgs)


# ------------------------------------------------------------------------------------------------------------- both engines
@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_launch_split_is_bit_identical(ur10, monkeypatch, eng):
    """Split at steps 5 and 9 of 12: a launch finds its rows by the absolute step number."""
    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs, sched, _, pert, surf = _inputs(_raw(4, 12, 12, seed=9))
    one, info, _, _ = _rollout(cfgs, ur10, sched, pert, surf)
    assert info["engine"] == (0 if eng == "latency" else 1)
    two, _, _, _ = _rollout(cfgs, ur10, sched, pert, surf, splits=[5, 9])
    for k in one:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(one[k], two[k], err_msg=k)


@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_null_cases(ur10, monkeypatch, eng):
    """surf_sched == NULL is mpcb_rollout_pert bit for bit, on its kernels; a schedule whose every row equals the packed
    coefficients gives its results through the kernels of this rollout."""
    import torch

    from robotic_mpc_amd import engine

    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs, sched, _, pert, surf = _inputs(_raw(4, 12, 14, seed=10, constant=True))
    assert (surf == np.stack([c["coeffs"] for c in cfgs])[:, None]).all()
    ref, info, _, kinfo = tp._rollout(cfgs, ur10, sched, pert)
    assert info["engine"] == (0 if eng == "latency" else 1)
    e = engine.MpcBatchEngine(0)
    try:
        pb = e.setup(cfgs, ur10)
        bufs = e.alloc_results(pb)
        keep = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (sched, pert["wcv"], pert["u_dist"], pert["x_noise"])]
        ptr = [C.cast(C.c_void_p(t.data_ptr()), _dp) for t in keep]
        p = engine.MpcbPlantPert(ptr[1], ptr[2], ptr[3])
        r = e._result_struct(bufs)
        assert e.lib.mpcb_rollout_surf(e._h, 0, pb.Nsim, C.byref(r), ptr[0], C.byref(p), None, None) == 0
        e.sync()
        for k, v in bufs.items():
            if k not in ("solver_time", "plant_time"):
                np.testing.assert_array_equal(v.cpu().numpy(), ref[k], err_msg=k)
        assert e.kernel_info() == kinfo                                       # (the perturbed rollout's kernel)
    finally:
        e.close()
    got, _, _, ksurf = _rollout(cfgs, ur10, sched, pert, surf)
    for k in ("z", "u", "ee_pose", "ee_rpy", "ee_vel", "errors"):
        np.testing.assert_allclose(got[k], ref[k], atol=1e-9, rtol=0, err_msg=k)
    np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["residuals"], ref["residuals"], atol=1e-9, rtol=1e-6)
    for k in INTS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert ksurf["vgprs"] > 0                                                 # (this rollout's kernel reports itself)
    print(f"\n[surf] kernel_info {eng}: perturbed rollout {kinfo}, scheduled surface {ksurf}")


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ur10):
    import torch

    from robotic_mpc_amd import engine

    raw = _raw(3, 12, 6, seed=11)
    cfgs, sched, _, pert, surf = _inputs(raw)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
    y, st = dev(sched), dev(surf)
    pt = {k: dev(v) for k, v in pert.items()}
    e = engine.MpcBatchEngine(0)
    try:
        # a controller handle
        pb = e.setup_controller(cfgs, ur10)
        bufs = e.alloc_results(pb)
        with pytest.raises(engine.EngineError, match=r"\(-5\)"):                 # MPCB_ESTATE
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, surf=st)
        # the fp32 leg
        e.setup(tp._resolve(tp._raw(3, 12, 6, seed=11, schedule=None, which=None, riccati_precision="fp32")), ur10)
        with pytest.raises(engine.EngineError, match=r"\(-1\).*fp64"):           # MPCB_EINVAL
            e.rollout(bufs, 0, pb.Nsim, yref=y, surf=st)
        # full SQP
        e.setup(tp._resolve(tp._raw(3, 12, 6, seed=11, solver="SQP")), ur10)
        with pytest.raises(engine.EngineError, match=r"\(-1\).*SQP_RTI"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, surf=st)
        # without a reference schedule, at the C level; the step-range rules of mpcb_rollout
        e.setup(cfgs, ur10)
        r = e._result_struct(bufs)
        yp, sp = (C.cast(C.c_void_p(t.data_ptr()), _dp) for t in (y, st))
        assert e.lib.mpcb_rollout_surf(e._h, 0, pb.Nsim, C.byref(r), None, None, sp, None) == -1
        assert b"schedule" in e.lib.mpcb_last_error(e._h)
        assert e.lib.mpcb_rollout_surf(e._h, 2, pb.Nsim, C.byref(r), yp, None, sp, None) == -5
        assert e.lib.mpcb_rollout_surf(e._h, 0, pb.Nsim + 1, C.byref(r), yp, None, sp, None) == -1
        # wrong shapes and combinations never reach the library (the handle's error text stays that of the call above)
        before = e.lib.mpcb_last_error(e._h)
        with pytest.raises(ValueError, match="surf"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, surf=st[:, :-1].contiguous())
        with pytest.raises(ValueError, match="surf"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, surf=st.float())
        with pytest.raises(ValueError, match="surf"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, surf=st.cpu())
        with pytest.raises(ValueError, match="yref"):
            e.rollout(bufs, 0, pb.Nsim, pert=pt, surf=st)
        with pytest.raises(ValueError, match="obs"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, surf=st, obs={})
        with pytest.raises(ValueError, match="term"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, surf=st, term={})
        assert e.lib.mpcb_last_error(e._h) == before
        # ... and the handle still runs
        e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, surf=st)
        e.sync()
        assert (bufs["status"].cpu().numpy() == 0).all()
    finally:
        e.close()


# ----------------------------------------------------------------------------------------------------------- public interface
def test_grid_over_the_velocity_through_run_all(ur10):
    """A 3-point grid over surface_schedule.velocity through SimulationManager.run_all: one bucket, results in queue order,
    get_data()["surface_coeffs"] [6, Nsim + 1] = the rows of the moving quadric, the logged errors measured against them, and a
    workpiece that moves takes the tool with it."""
    from robotic_mpc_amd import SimulationManager, analysis, base_params, surface

    base = base_params(simulation_time=0.14 + 1e-9, prediction_horizon=12, solver_options={"nlp_solver_type": "SQP_RTI"},
                       surface_schedule={"kind": "moving", "velocity": [0.0, 0.0, 0.0]})
    vels = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.05], [0.1, -0.1, 0.02]]
    m = SimulationManager(base)
    m.grid_search({"surface_schedule.velocity": vels})
    res = m.run_all()
    assert m.last_run_info["buckets"] == 1 and base["surface_schedule"]["velocity"] == [0.0, 0.0, 0.0]
    assert [r["simulator"].resolved["surface_schedule"]["velocity"] for r in res] == vels
    for r, v in zip(res, vels):
        sim, rows = r["simulator"], r["data"]["surface_coeffs"]
        assert rows.shape == (6, 15) and (sim.solver_status == 0).all()
        t = np.arange(15) * sim.dt
        np.testing.assert_allclose(rows.T, surface.translated(sim.resolved["coeffs"], v[0] * t, v[1] * t, v[2] * t), rtol=0, atol=1e-15)
        sm = sim.simulation_model
        e = analysis.compute_errors(sm._ee_pose_log, sm._ee_velocity_log, rows, sim.translation, sim.px_ref, sim.vy_ref)
        for k in ("e1", "e2", "e3", "e4", "e5"):
            np.testing.assert_allclose(sim.errors[k], e[k], rtol=0, atol=1e-12, err_msg=k)
    assert np.abs(res[0]["data"]["q"] - res[1]["data"]["q"]).max() > 1e-4
    assert np.abs(res[0]["data"]["q"] - res[2]["data"]["q"]).max() > 1e-4
