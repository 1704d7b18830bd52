"""Rollouts with the joint-wise terminal cost on the GPU (mpcb_rollout_term; the configuration key terminal_cost), on both engines.
The yardstick is what defines this rollout: the BatchController loop of test_gpu_rollout_pert.py::_step_loop, over the same nominal
or perturbed plant, that calls ctl.set_terminal_cost(blocks, x_ref[:, t]) before ctl.step(z_t + noise_t, yref = sched[:, t : t + N])
at every step t.  Compared at _compare's tolerances of that file.

Inputs: that file's draws (flat surface, q_0 jitter, the 2-lane serpentine, its perturbations where a case has them on); the LQR
blocks of each simulation's own model, lqr(10, 1, 1) (pqq ~ 456) unless a test says otherwise; the table
x_ref[i, t] = [q_0; 0] + [0.02 (6) | 0.05 (6)] sin(0.4 t + phase), phases from default_rng([seed, 99]) (term_rollout_cases.py).
Every test that compares first asserts from the reference loop alone that every step has status 0 and that the loop without the
terminal cost ends up more than 1e-4 away in z."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import term_rollout_cases as trc  # noqa: E402
import test_gpu_rollout_pert as tp  # noqa: E402

pytestmark = pytest.mark.gpu
INTS = tp.INTS
_dp = C.POINTER(C.c_double)


def _rollout(cfgs, ur10, sched, pert, blocks, x_ref, splits=None):
    """One bucket through setup / rollout(yref=, pert=, term=) / sync.  `pert`: dict of numpy arrays or None (the nominal plant);
    `blocks` [B, 6, 3] (None: no term=).  Returns (results as numpy, launch_info, queue_used of the last launch, kernel_info)."""
    import torch

    from robotic_mpc_amd import engine

    e = engine.MpcBatchEngine(0)
    try:
        pb = e.setup(cfgs, ur10)
        bufs = e.alloc_results(pb)
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
        yt = dev(sched)
        pt = None if pert is None else {k: dev(v) for k, v in pert.items()}
        tt = None if blocks is None else {"blocks": dev(trc.flat18(blocks)), "x_ref": dev(x_ref)}
        bounds = [0] + list(splits or []) + [pb.Nsim]
        for s0, s1 in zip(bounds[:-1], bounds[1:]):
            e.rollout(bufs, s0, s1, yref=yt, pert=pt, term=tt)
            e.sync()
        return {k: v.cpu().numpy() for k, v in bufs.items()}, e.launch_info(), e.queue_used(), e.kernel_info()
    finally:
        e.close()


def _step_loop(orc, raw, sched, pert, blocks, x_ref, eng):
    """The reference: test_gpu_rollout_pert._step_loop with ctl.set_terminal_cost(blocks, x_ref[:, t]) before the step of every t
    (blocks None: without a terminal cost).  `pert`: the arrays of the plant (the nominal ones for the nominal plant)."""
    from robotic_mpc_amd import BatchController

    cfgs = tp._resolve(raw)
    ctl = BatchController(raw, engine=eng)
    B, S, N = len(cfgs), cfgs[0]["Nsim"], max(c["N"] for c in cfgs)
    o = dict(z=np.zeros((B, 12, S + 1)), u=np.zeros((B, 6, S + 1)), cost=np.zeros((B, S)), residuals=np.zeros((B, S, 4)),
             status=np.zeros((B, S), np.int32), sqp_iter=np.zeros((B, S), np.int32), qp_iter=np.zeros((B, S), np.int32))
    z = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    o["z"][:, :, 0] = z
    o["u"][:, :, 0] = np.stack([c["qdot0"] for c in cfgs])
    for t in range(S):
        if blocks is not None:
            ctl.set_terminal_cost(np.ascontiguousarray(blocks), np.ascontiguousarray(x_ref[:, t]))
        r = {n: v.cpu().numpy() for n, v in ctl.step(z + pert["x_noise"][:, t], yref=np.ascontiguousarray(sched[:, t:t + N])).items()}
        for k in ("cost", "residuals") + INTS:
            o[k][:, t] = r[k]
        z = np.stack([orc.plant_step(c["plant_integrator"], pert["wcv"][i], c["dt"], z[i], r["u0"][i] + pert["u_dist"][i, t])
                      for i, c in enumerate(cfgs)])
        o["z"][:, :, t + 1], o["u"][:, :, t + 1] = z, r["u0"]
    return o


def _inputs(raw, seed, weights=trc.STRONG):
    """(cfgs, sched, the plant's arrays for the loop, pert for the rollout (None: nominal), blocks [B, 6, 3], x_ref [B, Nsim, 12])."""
    from robotic_mpc_amd import plant, reference

    cfgs = tp._resolve(raw)
    perturbed = cfgs[0]["plant_perturbation"] is not None
    arrays = plant.stack(cfgs) if perturbed else tp._nominal(cfgs)
    return cfgs, reference.stack(cfgs), arrays, (arrays if perturbed else None), trc.lqr_blocks(cfgs, weights), trc.table(cfgs, seed)


def _guards(orc, raw, sched, arrays, want, eng, check=None):
    """From the reference loop alone: every step has status 0, and the terminal cost matters."""
    idx = list(range(len(raw))) if check is None else list(check)
    assert (want["status"] == 0).all()
    without = _step_loop(orc, raw, sched, arrays, None, None, eng)
    assert np.abs(without["z"][idx] - want["z"][idx]).max() > 1e-4


def _case(orc, ur10, monkeypatch, eng, raw, seed, waves, check=None, weights=trc.STRONG):
    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs, sched, arrays, pert, blocks, x_ref = _inputs(raw, seed, weights)
    want = _step_loop(orc, raw, sched, arrays, blocks, x_ref, eng)
    _guards(orc, raw, sched, arrays, want, eng, check)
    got, info, _, _ = _rollout(cfgs, ur10, sched, pert, blocks, x_ref)
    assert (info["engine"], info["waves_per_sim"]) == ((0, waves) if eng == "latency" else (1, 1)), info
    tp._compare(got, want, sched, cfgs, check)
    return got, want, cfgs


# ------------------------------------------------------------------------------------------------------------ latency engine
@pytest.mark.parametrize("n,N,steps,waves", [(4, 12, 14, 4), (3, 100, 6, 8), (2, 224, 3, 8), (4, 12, 14, 2), (4, 12, 14, 1)])
def test_latency_engine_with_a_terminal_cost_over_the_perturbed_plant(orc, ur10, monkeypatch, n, N, steps, waves):
    if waves < 4:      # <2> and <1>: mpcb_setup never picks them by itself
        monkeypatch.setenv("MPCB_WAVES_PER_SIM", str(waves))
    _case(orc, ur10, monkeypatch, "latency", tp._raw(n, N, steps, seed=1), 1, waves)


def test_latency_engine_with_a_terminal_cost_over_the_nominal_plant(orc, ur10, monkeypatch):
    """pert = None: the nominal plant through the same kernels."""
    _, _, cfgs = _case(orc, ur10, monkeypatch, "latency", tp._raw(4, 12, 14, seed=1, which=None), 1, 4)
    assert all(c["plant_perturbation"] is None for c in cfgs)


def test_latency_engine_two_simulations_per_cu(orc, ur10, monkeypatch):
    n = tp._num_cus() + 64
    _case(orc, ur10, monkeypatch, "latency", tp._raw(n, 12, 5, seed=2), 2, 4, check=range(0, n, 20))


def test_tight_bounds_take_both_qp_paths(orc, ur10, monkeypatch):
    """The bounds of the rti_tight_bounds fixture with the weak weight lqr(0.001, 0.001, 1): steps solved by the fast path (qp_iter
    1) and by the interior point (more) -- the strong weight would leave the interior point nothing."""
    _, want, _ = _case(orc, ur10, monkeypatch, "latency", tp._raw(4, 15, 14, seed=4, which=None, **tp.TIGHT), 4, 4, weights=trc.WEAK)
    assert (want["qp_iter"] > 1).any() and (want["qp_iter"] == 1).any()


# --------------------------------------------------------------------------------------------------------- throughput engine
def test_throughput_engine_with_a_terminal_cost(orc, ur10, monkeypatch):
    _case(orc, ur10, monkeypatch, "stream", tp._raw(6, 12, 14, seed=5), 5, 1)


def test_throughput_engine_ragged_horizons(orc, ur10, monkeypatch):
    """Horizons {5, 9, 12} in one launch: the terminal cost acts at each simulation's own last stage."""
    _, _, cfgs = _case(orc, ur10, monkeypatch, "stream", tp._raw(6, (5, 9, 12), 14, seed=7), 7, 1)
    assert sorted({c["N"] for c in cfgs}) == [5, 9, 12]


def test_throughput_engine_horizon_of_one(orc, ur10, monkeypatch):
    """N = 1: the terminal stage is stage 1, and the task rows of the QP vanish."""
    _case(orc, ur10, monkeypatch, "stream", tp._raw(3, 1, 10, seed=6, which=None), 6, 1)


def test_throughput_engine_work_queue_is_bit_identical_to_the_plain_launch(orc, ur10, monkeypatch):
    """Batch 8, 11 steps, 4 resident wavefronts, chunks of 3 steps: every chunk of every simulation changes hands, and each item
    reads its own rows of the table."""
    monkeypatch.setenv("MPCB_ENGINE", "stream")
    raw = tp._raw(8, 12, 11, seed=8)
    cfgs, sched, arrays, pert, blocks, x_ref = _inputs(raw, 8)
    plain, info, used, _ = _rollout(cfgs, ur10, sched, pert, blocks, x_ref)
    assert info["engine"] == 1 and not used
    monkeypatch.setenv("MPCB_STREAM_SLOTS", "4")
    monkeypatch.setenv("MPCB_STREAM_CHUNK", "3")
    queued, info, used, _ = _rollout(cfgs, ur10, sched, pert, blocks, x_ref)
    assert info["engine"] == 1 and used
    for k in plain:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(plain[k], queued[k], err_msg=k)
    monkeypatch.delenv("MPCB_STREAM_SLOTS")
    monkeypatch.delenv("MPCB_STREAM_CHUNK")
    want = _step_loop(orc, raw, sched, arrays, blocks, x_ref, "stream")
    _guards(orc, raw, sched, arrays, want, "stream")
    tp._compare(queued, want, sched, cfgs)


# ------------------------------------------------------------------------------------------------------------- both engines
@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_launch_split_is_bit_identical(ur10, monkeypatch, eng):
    """Nothing of the terminal cost carries across a launch boundary: the next launch reads its own rows."""
    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs, sched, _, pert, blocks, x_ref = _inputs(tp._raw(4, 12, 12, seed=9), 9)
    assert np.abs(x_ref[:, 4] - x_ref[:, 5]).min() > 0                        # the rows around the boundary differ
    one, info, _, _ = _rollout(cfgs, ur10, sched, pert, blocks, x_ref)
    assert info["engine"] == (0 if eng == "latency" else 1)
    two, _, _, _ = _rollout(cfgs, ur10, sched, pert, blocks, x_ref, splits=[5])
    for k in one:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(one[k], two[k], err_msg=k)


@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_the_rollout_reads_the_row_of_its_step(orc, ur10, monkeypatch, eng):
    """Table against constant: the loop that holds x_ref[:, 0] for every step ends up elsewhere, and the rollout is the table's loop.
    A kernel that ignores the step index fails here."""
    monkeypatch.setenv("MPCB_ENGINE", eng)
    raw = tp._raw(3, 12, 10, seed=13)
    cfgs, sched, arrays, pert, blocks, x_ref = _inputs(raw, 13)
    want = _step_loop(orc, raw, sched, arrays, blocks, x_ref, eng)
    _guards(orc, raw, sched, arrays, want, eng)
    held = _step_loop(orc, raw, sched, arrays, blocks, np.repeat(x_ref[:, :1], x_ref.shape[1], axis=1), eng)
    assert np.abs(held["z"] - want["z"]).max() > 1e-4
    got, info, _, _ = _rollout(cfgs, ur10, sched, pert, blocks, x_ref)
    assert info["engine"] == (0 if eng == "latency" else 1)
    tp._compare(got, want, sched, cfgs)


@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_null_cases(ur10, monkeypatch, eng):
    """term_blocks == NULL is mpcb_rollout_pert bit for bit, on its kernels; all-zero blocks are its results through the kernels of
    this rollout."""
    import torch

    from robotic_mpc_amd import engine

    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs, sched, _, pert, blocks, x_ref = _inputs(tp._raw(4, 12, 14, seed=10), 10)
    ref, info, _, kinfo = tp._rollout(cfgs, ur10, sched, pert)
    assert info["engine"] == (0 if eng == "latency" else 1)
    e = engine.MpcBatchEngine(0)
    try:
        pb = e.setup(cfgs, ur10)
        bufs = e.alloc_results(pb)
        keep = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (sched, pert["wcv"], pert["u_dist"], pert["x_noise"], x_ref)]
        ptr = [C.cast(C.c_void_p(t.data_ptr()), _dp) for t in keep]
        p = engine.MpcbPlantPert(ptr[1], ptr[2], ptr[3])
        r = e._result_struct(bufs)
        assert e.lib.mpcb_rollout_term(e._h, 0, pb.Nsim, C.byref(r), ptr[0], C.byref(p), None, ptr[4], None) == 0
        e.sync()
        for k, v in bufs.items():
            if k not in ("solver_time", "plant_time"):
                np.testing.assert_array_equal(v.cpu().numpy(), ref[k], err_msg=k)
        assert e.kernel_info() == kinfo                                       # (the perturbed rollout's kernel)
    finally:
        e.close()
    got, _, _, _ = _rollout(cfgs, ur10, sched, pert, np.zeros_like(blocks), x_ref)
    for k in ("z", "u", "ee_pose", "ee_rpy", "ee_vel", "errors"):
        np.testing.assert_allclose(got[k], ref[k], atol=1e-9, rtol=0, err_msg=k)
    np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["residuals"], ref["residuals"], atol=1e-9, rtol=1e-6)
    for k in INTS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ur10):
    import torch

    from robotic_mpc_amd import engine

    raw = tp._raw(3, 12, 6, seed=11)
    cfgs, sched, _, pert, blocks, x_ref = _inputs(raw, 11)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
    y = dev(sched)
    pt = {k: dev(v) for k, v in pert.items()}
    tt = {"blocks": dev(trc.flat18(blocks)), "x_ref": dev(x_ref)}
    e = engine.MpcBatchEngine(0)
    try:
        # a controller handle
        pb = e.setup_controller(cfgs, ur10)
        bufs = e.alloc_results(pb)
        with pytest.raises(engine.EngineError, match=r"\(-5\)"):                 # MPCB_ESTATE
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, term=tt)
        # the fp32 leg
        e.setup(tp._resolve(tp._raw(3, 12, 6, seed=11, schedule=None, which=None, riccati_precision="fp32")), ur10)
        with pytest.raises(engine.EngineError, match=r"\(-1\).*fp64"):           # MPCB_EINVAL
            e.rollout(bufs, 0, pb.Nsim, yref=y, term=tt)
        # full SQP
        e.setup(tp._resolve(tp._raw(3, 12, 6, seed=11, solver="SQP")), ur10)
        with pytest.raises(engine.EngineError, match=r"\(-1\).*SQP_RTI"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, term=tt)
        # blocks without x_ref, and without a schedule, at the C level
        e.setup(cfgs, ur10)
        r = e._result_struct(bufs)
        yp, bp, xp = (C.cast(C.c_void_p(t.data_ptr()), _dp) for t in (y, tt["blocks"], tt["x_ref"]))
        assert e.lib.mpcb_rollout_term(e._h, 0, pb.Nsim, C.byref(r), yp, None, bp, None, None) == -1
        assert b"term_xref" in e.lib.mpcb_last_error(e._h)
        assert e.lib.mpcb_rollout_term(e._h, 0, pb.Nsim, C.byref(r), None, None, bp, xp, None) == -1
        # wrong shapes never reach the library (the handle's error text stays that of the call above)
        before = e.lib.mpcb_last_error(e._h)
        with pytest.raises(ValueError, match="x_ref"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, term={**tt, "x_ref": tt["x_ref"][:, :-1].contiguous()})
        with pytest.raises(ValueError, match="blocks"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, term={**tt, "blocks": dev(blocks)})           # [B, 6, 3]
        with pytest.raises(ValueError, match="blocks"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, term={**tt, "blocks": tt["blocks"].float()})
        with pytest.raises(ValueError, match="x_ref"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, term={**tt, "x_ref": tt["x_ref"].cpu()})
        with pytest.raises(ValueError, match="keys"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, term={"blocks": tt["blocks"]})
        with pytest.raises(ValueError, match="yref"):
            e.rollout(bufs, 0, pb.Nsim, pert=pt, term=tt)
        assert e.lib.mpcb_last_error(e._h) == before
        # ... and the handle still runs
        e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, term=tt)
        e.sync()
        assert (bufs["status"].cpu().numpy() == 0).all()
    finally:
        e.close()


# ----------------------------------------------------------------------------------------------------------- public interface
def test_grid_search_over_the_terminal_weight_through_run_all(ur10, monkeypatch, tmp_path):
    """terminal_cost.weight.r_weight x prediction_horizon through SimulationManager, without a schedule (the packed rows): one ragged
    bucket on the throughput engine, results in queue order, the realised table and blocks in `data`, the device summary against the
    host formula over the logged columns, checkpoint and resume."""
    from robotic_mpc_amd import SimulationManager, analysis, base_params, packing, terminal

    monkeypatch.setattr(packing, "RAGGED_MIN_BATCH", 4)
    q0 = np.asarray(base_params()["q_0"], dtype=np.float64)
    rows = np.concatenate([q0, np.zeros(6)])[None, :] + trc.AMPLITUDE[None, :] * np.sin(0.4 * np.arange(14))[:, None]
    base = base_params(simulation_time=0.14 + 1e-9, prediction_horizon=12, solver_options={"nlp_solver_type": "SQP_RTI"},
                       terminal_cost={"weight": {"kind": "lqr", "q_weight": 10.0, "qdot_weight": 1.0, "r_weight": 1.0},
                                      "reference": {"kind": "table", "rows": rows.tolist()}})
    grid = {"terminal_cost.weight.r_weight": [0.5, 1.0, 4.0], "prediction_horizon": [8, 12]}
    path = str(tmp_path / "grid.npz")
    m = SimulationManager(base)
    m.grid_search(grid)
    assert base["terminal_cost"]["weight"]["r_weight"] == 1.0
    res = m.run_all(checkpoint=path)
    assert m.last_run_info["buckets"] == 1 and m.last_run_info["n_resumed"] == 0
    want_order = [(r, N) for r in (0.5, 1.0, 4.0) for N in (8, 12)]
    assert [(r["simulator"].resolved["terminal_cost"]["weight"]["r_weight"], r["simulator"].prediction_horizon) for r in res] == want_order
    for r in res:
        sim = r["simulator"]
        c = sim.resolved
        s = terminal.sample(c)
        np.testing.assert_array_equal(r["data"]["terminal_reference"], rows)
        np.testing.assert_array_equal(r["data"]["terminal_blocks"], s["blocks"])
        assert r["data"]["terminal_reference"].shape == (14, 12) and r["data"]["terminal_blocks"].shape == (6, 3)
        assert (sim.solver_status == 0).all()
        sm = sim.simulation_model
        e = analysis.compute_errors(sm._ee_pose_log, sm._ee_velocity_log, c["coeffs"], c["t_ee"], c["px_ref"], c["vy_ref"])
        for k in ("e1", "e2", "e3", "e4", "e5"):
            np.testing.assert_allclose(sim.errors[k], e[k], atol=1e-12, rtol=0, err_msg=k)
            assert abs(r["summary"][f"rmse_{k}"] - np.sqrt(np.mean(e[k] ** 2))) < 1e-12, k
    # the weight matters, and so does the horizon
    assert np.abs(res[0]["data"]["q"] - res[4]["data"]["q"]).max() > 1e-4
    assert np.abs(res[0]["data"]["q"] - res[1]["data"]["q"]).max() > 1e-4
    # resume: nothing runs again
    m2 = SimulationManager(base)
    m2.grid_search(grid)
    again = m2.run_all(checkpoint=path)
    assert m2.last_run_info["n_resumed"] == 6
    for a, b in zip(res, again):
        for k in ("q", "qdot", "u", "terminal_reference", "terminal_blocks"):
            np.testing.assert_array_equal(a["data"][k], b["data"][k])
        np.testing.assert_array_equal(a["simulator"].errors["e5"], b["simulator"].errors["e5"])
