"""The combined rollout on the GPU (mpcb_rollout_combined; the configuration key combine_features), on both engines: terminal cost,
disturbance observer, scheduled surface and shift warm start live at once, every simulation of a batch using its own subset
(combined_cases.SUBSETS: all four, none, each alone, two pairs).

The yardstick is what defines this rollout: the BatchController(combined=True) loop
    step(z_t + noise_t, yref = sched[:, t:t+N], surface = surf[:, t:t+N], dist = d^_t, shift = (t >= 1 and mode == shift))
with set_terminal_cost(blocks, x_ref[:, t]) before every step, the torch observer recurrence of observer.DisturbanceObserver after it
(with each simulation's gains; zero gains where it has no observer), over the host plant of test_gpu_rollout_pert._step_loop.  Compared
at test_gpu_rollout_pert._compare's tolerances -- atol 1e-9 on the logs, rtol 1e-9 on the cost, atol 1e-9 with rtol 1e-6 on the
residuals, ints equal -- with the error log recomputed on the host (atol 1e-12), and d_hat at atol 1e-9.

Guards (combined_cases.guards), from the reference loops alone and before every comparison: every step has status 0, and for each
feature a simulation with N >= 2 uses, the loop with that one feature off ends more than 1e-4 away in z.  Seeds: those of
test_gpu_rollout_shift.py's cases; they held in emulation (seed 1, (8, 12, 14): the smallest distances 3.1 (term), 0.25 (obs), 1.4e-3
(surf), 5.4e-4 (shift)); one had to be skipped, in the ragged batch (its docstring says which and why)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import combined_cases as cc  # noqa: E402
import test_gpu_rollout_pert as tp  # noqa: E402

pytestmark = pytest.mark.gpu
INTS = tp.INTS
SHIFT = 2


def _rollout(cfgs, ur10, tabs, splits=None, drop=()):
    """One bucket through setup / rollout(combined=True, ...) / sync with the tables of engine.combined_arrays.  `drop`: features
    handed over as None (the library fills their neutral tables).  Returns (results as numpy with d_hat, launch_info, queue_used,
    kernel_info)."""
    import torch

    from robotic_mpc_amd import engine

    e = engine.MpcBatchEngine(0)
    try:
        pb = e.setup(cfgs, ur10)
        bufs = e.alloc_results(pb)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
        d_hat = torch.full((pb.batch, pb.Nsim, 6), float("nan"), dtype=torch.float64, device="cuda:0")
        kw = dict(yref=dev(tabs["yref"]), pert={k: dev(v) for k, v in tabs["pert"].items()},
                  term=None if "term" in drop else {k: dev(v) for k, v in tabs["term"].items()},
                  obs=None if "obs" in drop else {"gain": dev(tabs["gain"]), "d_hat": d_hat},
                  surf=None if "surf" in drop else dev(tabs["surf"]), warm=None if "shift" in drop else dev(tabs["warm"]))
        bounds = [0] + list(splits or []) + [pb.Nsim]
        for s0, s1 in zip(bounds[:-1], bounds[1:]):
            e.rollout(bufs, s0, s1, combined=True, **kw)
            e.sync()
        out = {k: v.cpu().numpy() for k, v in bufs.items()}
        out["d_hat"] = d_hat.cpu().numpy()
        return out, e.launch_info(), e.queue_used(), e.kernel_info()
    finally:
        e.close()


def _step_loop(orc, raw, cfgs, tabs, eng, off=()):
    """The reference loop of the module docstring.  `off`: features switched off (their tables replaced by neutral ones)."""
    import torch

    from robotic_mpc_amd import BatchController

    strip = ("surface_schedule", "warm_start", "terminal_cost", "disturbance_observer", "combine_features")
    ctl = BatchController([{k: v for k, v in r.items() if k not in strip} for r in raw], engine=eng, combined=True)
    B, S, N = len(cfgs), cfgs[0]["Nsim"], max(c["N"] for c in cfgs)
    pert = tabs["pert"]
    gain = np.zeros((B, 12)) if "obs" in off else tabs["gain"]
    blocks = (np.zeros((B, 18)) if "term" in off else tabs["term"]["blocks"]).reshape(B, 3, 6).transpose(0, 2, 1)     # [B, 6, 3]
    P = np.zeros((B, 12, 12))
    for j in range(6):
        P[:, j, j], P[:, j, 6 + j], P[:, 6 + j, j], P[:, 6 + j, 6 + j] = blocks[:, j, 0], blocks[:, j, 1], blocks[:, j, 1], blocks[:, j, 2]
    surf = np.repeat(np.stack([c["coeffs"] for c in cfgs])[:, None, :], S + N, axis=1) if "surf" in off else tabs["surf"]
    mask = np.zeros(B, bool) if "shift" in off else np.asarray(tabs["warm"]) == SHIFT
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    a22 = T(np.stack([np.exp(-np.asarray(c["wcv"], dtype=np.float64) * c["dt"]) for c in cfgs]))
    b2, l1, l2 = 1.0 - a22, T(gain[:, :6]), T(gain[:, 6:])
    o = dict(z=np.zeros((B, 12, S + 1)), u=np.zeros((B, 6, S + 1)), cost=np.zeros((B, S)), residuals=np.zeros((B, S, 4)),
             status=np.zeros((B, S), np.int32), sqp_iter=np.zeros((B, S), np.int32), qp_iter=np.zeros((B, S), np.int32),
             d_hat=np.zeros((B, S, 6)))
    z = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    o["z"][:, :, 0] = z
    o["u"][:, :, 0] = np.stack([c["qdot0"] for c in cfgs])
    v = d = y_prev = None
    u_prev = torch.zeros(B, 6, dtype=torch.float64)
    for t in range(S):
        xhat = z + pert["x_noise"][:, t]
        y = T(xhat[:, 6:]).clone()
        if v is None:
            v, d = y.clone(), torch.zeros_like(y)
        else:                                                      # DisturbanceObserver.update with this simulation's gains
            innov = y_prev - v
            v, d = a22 * v + b2 * (u_prev + d) + l1 * innov, d + l2 * innov
        y_prev = y
        o["d_hat"][:, t] = d.numpy()
        ctl.set_terminal_cost(P, np.ascontiguousarray(tabs["term"]["x_ref"][:, t]))
        r = {n: w.cpu().numpy() for n, w in ctl.step(xhat, yref=np.ascontiguousarray(tabs["yref"][:, t:t + N]),
                                                     surface=np.ascontiguousarray(surf[:, t:t + N]), dist=d.numpy().copy(),
                                                     shift=mask if t >= 1 and mask.any() else False).items()}
        for k in ("cost", "residuals") + INTS:
            o[k][:, t] = r[k]
        z = np.stack([orc.plant_step(c["plant_integrator"], pert["wcv"][i], c["dt"], z[i], r["u0"][i] + pert["u_dist"][i, t])
                      for i, c in enumerate(cfgs)])
        o["z"][:, :, t + 1], o["u"][:, :, t + 1] = z, r["u0"]
        u_prev = T(r["u0"]).clone()
    ctl.close()
    return o


def _compare(got, want, tabs, cfgs, check=None):
    from robotic_mpc_amd import analysis

    idx = list(range(len(cfgs))) if check is None else list(check)
    S = cfgs[0]["Nsim"]
    for k, a in (("z", got["z"]), ("u", got["u"]), ("d_hat", got["d_hat"]), ("cost", got["cost"]), ("residuals", got["residuals"])):
        print(f"[combined] max |{k} - loop| = {np.abs(a[idx] - want[k][idx]).max():.3e}")
    np.testing.assert_allclose(got["z"][idx], want["z"][idx], atol=1e-9, rtol=0)
    np.testing.assert_allclose(got["u"][idx], want["u"][idx], atol=1e-9, rtol=0)
    np.testing.assert_allclose(got["d_hat"][idx], want["d_hat"][idx], atol=1e-9, rtol=0)
    np.testing.assert_allclose(got["cost"][idx], want["cost"][idx], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["residuals"][idx], want["residuals"][idx], atol=1e-9, rtol=1e-6)
    for k in INTS:
        np.testing.assert_array_equal(got[k][idx], want[k][idx], err_msg=k)
    for i in idx:
        c = cfgs[i]
        e = analysis.errors_rows(analysis.compute_errors(got["ee_pose"][i], got["ee_vel"][i], tabs["surf"][i, :S + 1].T, c["t_ee"],
                                                         c["px_ref"], c["vy_ref"], yref=tabs["yref"][i, :S + 1]))
        np.testing.assert_allclose(got["errors"][i], e, atol=1e-12, rtol=0, err_msg=f"errors of simulation {i}")
    assert np.isfinite(got["solver_time"]).all() and (got["solver_time"] > 0).all()


def _case(orc, ur10, monkeypatch, eng, raw, waves, check=None, splits=None):
    from robotic_mpc_amd import engine

    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs = cc.resolve(raw)
    tabs = engine.combined_arrays(cfgs)
    want = _step_loop(orc, raw, cfgs, tabs, eng)
    idx = list(range(len(cfgs))) if check is None else list(check)
    used = {f for i in idx for f in cc.uses(cfgs[i])}
    cc.guards(cfgs, want, {f: _step_loop(orc, raw, cfgs, tabs, eng, off=(f,)) for f in cc.FEATURES if f in used}, check)
    got, info, _, _ = _rollout(cfgs, ur10, tabs, splits)
    assert (info["engine"], info["waves_per_sim"]) == ((0, waves) if eng == "latency" else (1, 1)), info
    _compare(got, want, tabs, cfgs, check)
    return got, want, cfgs, tabs


# ------------------------------------------------------------------------------------------------------------ latency engine
@pytest.mark.parametrize("n,N,steps,waves", [(4, 12, 14, 4), (3, 100, 6, 8), (2, 224, 3, 8), (4, 12, 14, 2), (4, 12, 14, 1)])
def test_latency_engine_combined(orc, ur10, monkeypatch, n, N, steps, waves):
    """(the first n subsets: all four, none, term alone, obs alone)"""
    if waves < 4:      # <2> and <1>: mpcb_setup never picks them by itself
        monkeypatch.setenv("MPCB_WAVES_PER_SIM", str(waves))
    _case(orc, ur10, monkeypatch, "latency", cc.raw(n, N, steps, seed=1), waves)


def test_latency_engine_every_subset(orc, ur10, monkeypatch):
    _, _, cfgs, _ = _case(orc, ur10, monkeypatch, "latency", cc.raw(8, 12, 14, seed=13), 4)
    assert [cc.uses(c) for c in cfgs] == list(cc.SUBSETS)


def test_latency_engine_two_simulations_per_cu(orc, ur10, monkeypatch):
    n = tp._num_cus() + 64
    _case(orc, ur10, monkeypatch, "latency", cc.raw(n, 12, 5, seed=2), 4, check=range(0, n, 24))


def test_tight_bounds_take_both_qp_paths(orc, ur10, monkeypatch):
    _, want, _, _ = _case(orc, ur10, monkeypatch, "latency", cc.raw(4, 15, 14, seed=4, **tp.TIGHT), 4)
    assert (want["qp_iter"] > 1).any() and (want["qp_iter"] == 1).any()


# --------------------------------------------------------------------------------------------------------- throughput engine
def test_throughput_engine_every_subset(orc, ur10, monkeypatch):
    _case(orc, ur10, monkeypatch, "stream", cc.raw(8, 12, 14, seed=5), 1)


def test_throughput_engine_ragged_horizons(orc, ur10, monkeypatch):
    """Horizons {1, 2, 7, 12} in one launch, two simulations each: the terminal cost sits on each simulation's own last stage, the
    shift ends at its own horizon, and the tables have Nsim + 12 rows.  Seed 17: with seed 7 (test_gpu_rollout_shift.py's) the
    all-four simulation with N = 2 ends only 8.3e-5 from its loop without the surface table -- two stages let the table reach u0
    through stage 1 alone -- so that draw was skipped (27 and 37: 6.8e-5, 6.6e-5; 17: 1.5e-4 and 1.2e-4 for the two N = 2
    simulations, measured in emulation)."""
    subsets = (cc.FEATURES,) * 4 + (("term", "shift"), ("obs", "surf"), ("term",), ())
    _, _, cfgs, tabs = _case(orc, ur10, monkeypatch, "stream", cc.raw(8, (1, 2, 7, 12), 14, seed=17, subsets=subsets), 1)
    assert sorted({c["N"] for c in cfgs}) == [1, 2, 7, 12] and tabs["surf"].shape[1] == 14 + 12


def test_throughput_engine_work_queue_is_bit_identical_to_the_plain_launch(orc, ur10, monkeypatch):
    """Batch 8, 11 steps, 4 resident wavefronts, chunks of 3 steps: every chunk changes hands; a chunk that starts at step t >= 1
    publishes d^_t from ST_OBS, shifts with it, and reads row t of the terminal and surface tables."""
    from robotic_mpc_amd import engine

    monkeypatch.setenv("MPCB_ENGINE", "stream")
    raw = cc.raw(8, 12, 11, seed=8)
    cfgs = cc.resolve(raw)
    tabs = engine.combined_arrays(cfgs)
    plain, info, used, _ = _rollout(cfgs, ur10, tabs)
    assert info["engine"] == 1 and not used
    monkeypatch.setenv("MPCB_STREAM_SLOTS", "4")
    monkeypatch.setenv("MPCB_STREAM_CHUNK", "3")
    queued, info, used, _ = _rollout(cfgs, ur10, tabs)
    assert info["engine"] == 1 and used
    for k in plain:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(plain[k], queued[k], err_msg=k)
    monkeypatch.delenv("MPCB_STREAM_SLOTS")
    monkeypatch.delenv("MPCB_STREAM_CHUNK")
    want = _step_loop(orc, raw, cfgs, tabs, "stream")
    cc.guards(cfgs, want, {f: _step_loop(orc, raw, cfgs, tabs, "stream", off=(f,)) for f in cc.FEATURES})
    _compare(queued, want, tabs, cfgs)


# ------------------------------------------------------------------------------------------------------------- both engines
@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_launch_split_is_bit_identical(orc, ur10, monkeypatch, eng):
    """Split at steps 5 and 9 of 12: ST_OBS and the shift cross a launch boundary, the tables are read at the absolute step.  The
    single launch is held to the step loop (guards first), the split one to the single launch bit for bit."""
    from robotic_mpc_amd import engine

    monkeypatch.setenv("MPCB_ENGINE", eng)
    raw = cc.raw(4, 12, 12, seed=9, subsets=(cc.FEATURES, (), ("obs", "surf"), ("term", "shift")))
    cfgs = cc.resolve(raw)
    tabs = engine.combined_arrays(cfgs)
    want = _step_loop(orc, raw, cfgs, tabs, eng)
    cc.guards(cfgs, want, {f: _step_loop(orc, raw, cfgs, tabs, eng, off=(f,)) for f in cc.FEATURES})
    one, info, _, kinfo = _rollout(cfgs, ur10, tabs)
    _compare(one, want, tabs, cfgs)
    assert info["engine"] == (0 if eng == "latency" else 1) and kinfo["vgprs"] > 0
    two, _, _, _ = _rollout(cfgs, ur10, tabs, splits=[5, 9])
    for k in one:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(one[k], two[k], err_msg=k)
    print(f"\n[combined] {eng}: kernel_info {kinfo}")


@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_null_arguments_are_the_neutral_tables(ur10, monkeypatch, eng):
    """No simulation uses any feature: every argument NULL (the library fills the neutral tables) gives what the caller's neutral
    tables give, bit for bit -- and that is the perturbed rollout's closed loop at _compare's tolerances."""
    from robotic_mpc_amd import engine

    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs = cc.resolve(cc.raw(4, 12, 14, seed=10, subsets=((),)))
    tabs = engine.combined_arrays(cfgs)
    assert not tabs["gain"].any() and not tabs["term"]["blocks"].any() and not tabs["warm"].any() and np.ptp(tabs["surf"], axis=1).max() == 0
    mine, _, _, _ = _rollout(cfgs, ur10, tabs)
    null, _, _, _ = _rollout(cfgs, ur10, tabs, drop=cc.FEATURES)
    for k in mine:
        if k not in ("solver_time", "plant_time", "d_hat"):
            np.testing.assert_array_equal(mine[k], null[k], err_msg=k)
    assert (mine["d_hat"] == 0).all()
    ref, _, _, _ = tp._rollout(cfgs, ur10, tabs["yref"], tabs["pert"])
    for k in ("z", "u", "ee_pose", "ee_rpy", "ee_vel", "errors"):
        np.testing.assert_allclose(mine[k], ref[k], atol=1e-9, rtol=0, err_msg=k)
    np.testing.assert_allclose(mine["cost"], ref["cost"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(mine["residuals"], ref["residuals"], atol=1e-9, rtol=1e-6)
    for k in INTS:
        np.testing.assert_array_equal(mine[k], ref[k], err_msg=k)


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ur10):
    import torch

    from robotic_mpc_amd import engine

    cfgs = cc.resolve(cc.raw(3, 12, 6, seed=11))
    tabs = engine.combined_arrays(cfgs)
    y = torch.from_numpy(tabs["yref"]).to("cuda:0")
    e = engine.MpcBatchEngine(0)
    try:
        pb = e.setup_controller(cfgs, ur10)
        bufs = e.alloc_results(pb)
        with pytest.raises(engine.EngineError, match=r"\(-5\)"):                 # MPCB_ESTATE: a controller handle
            e.rollout(bufs, 0, pb.Nsim, yref=y, combined=True)
        e.setup(tp._resolve(tp._raw(3, 12, 6, seed=11, schedule=None, which=None, riccati_precision="fp32")), ur10)
        with pytest.raises(engine.EngineError, match=r"\(-1\).*fp64"):           # MPCB_EINVAL
            e.rollout(bufs, 0, pb.Nsim, yref=y, combined=True)
        e.setup(tp._resolve(tp._raw(3, 12, 6, seed=11, solver="SQP")), ur10)
        with pytest.raises(engine.EngineError, match=r"\(-1\).*SQP_RTI"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, combined=True)
        e.setup(cfgs, ur10)
        with pytest.raises(ValueError, match="yref"):
            e.rollout(bufs, 0, pb.Nsim, combined=True)
        e.rollout(bufs, 0, pb.Nsim, yref=y, combined=True)                       # ... and the handle still runs, all NULL
        e.sync()
        assert (bufs["status"].cpu().numpy() == 0).all()
    finally:
        e.close()
    with pytest.raises(ValueError, match="combined"):
        engine.MpcBatchEngine(0).run_host_buffers(cfgs, ur10)


# ----------------------------------------------------------------------------------------------------------- public interface
def test_grid_over_the_features_through_run_all(ur10):
    """Dotted keys of all four features in one grid through SimulationManager.run_all: ONE bucket and one launch; each member equals
    its own single Simulator.run; get_data() brings d_hat, surface_coeffs and the terminal tables where configured."""
    from robotic_mpc_amd import SimulationManager, Simulator, base_params

    base = base_params(simulation_time=0.14 + 1e-9, prediction_horizon=12, solver_options={"nlp_solver_type": "SQP_RTI"},
                       reference_schedule=tp.SERP, combine_features=True,
                       plant_perturbation={"input_disturbance": {"kind": "step", "start_time": 0.03, "value": 0.05}},
                       terminal_cost={"weight": {"kind": "lqr", "q_weight": 10.0, "qdot_weight": 1.0, "r_weight": 1.0},
                                      "reference": {"kind": "constant", "value": [0.1, -1.4, 1.5, -1.6, -1.5, 0.1] + [0.0] * 6}},
                       disturbance_observer={"pole": 0.2}, surface_schedule={"kind": "moving", "velocity": [0.05, 0.0, 0.0]})
    grid = {"warm_start": ["carry", "shift"], "disturbance_observer.pole": [0.0, 0.2], "terminal_cost.weight.q_weight": [10.0, 5.0]}
    m = SimulationManager(base)
    m.grid_search(grid)
    res = m.run_all()
    assert m.last_run_info["buckets"] == 1 and len(res) == 8
    for r in res:
        sim = r["simulator"]
        assert (sim.solver_status == 0).all()
        d = r["data"]
        assert d["d_hat"].shape == (6, 14) and d["surface_coeffs"].shape == (6, 15) and d["terminal_reference"].shape == (14, 12)
        assert np.abs(d["d_hat"][:, -1]).max() > 1e-3
    assert np.abs(res[0]["data"]["q"] - res[4]["data"]["q"]).max() > 1e-5            # carry / shift
    r = res[5]
    one = Simulator(**r["simulator"].config)
    one.run()
    d1 = one.get_data()
    for k in ("q", "qdot", "u", "d_hat"):
        np.testing.assert_array_equal(r["data"][k], d1[k], err_msg=k)
