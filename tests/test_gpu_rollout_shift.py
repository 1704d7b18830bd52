"""Rollouts with the shift warm start on the GPU (mpcb_rollout_warm; the configuration key warm_start), on both engines.  The
yardstick is what defines this rollout: the BatchController loop of test_gpu_rollout_pert.py::_step_loop, over the same perturbed
plant on the host, whose step t >= 1 is ctl.step(z_t + noise_t, yref = sched[:, t : t + N], shift = the simulations whose mode is
shift) -- step 0 starts from the initial guess and shifts nothing -- with surface = surf[:, t : t + N] where a table is given.
Compared at _compare's tolerances of that file -- atol 1e-9 on the logs, rtol 1e-9 on the cost, atol 1e-9 with rtol 1e-6 on the
residuals, ints equal -- with the error log recomputed on the host (atol 1e-12).

Inputs: that file's draws and perturbations.  Every test that compares first asserts from the reference loops alone that every step
has status 0, that for every checked simulation with N >= 2 that shifts the all-carry loop ends more than 1e-4 away in z, and that
at N = 1 the two loops agree exactly in z."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import test_gpu_rollout_pert as tp  # noqa: E402
import test_gpu_rollout_surf as ts  # noqa: E402

pytestmark = pytest.mark.gpu
INTS = tp.INTS
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
CARRY, SHIFT = 0, 2


def _rollout(cfgs, ur10, sched, pert, warm, surf=None, splits=None):
    """One bucket through setup / rollout(yref=, pert=, surf=, warm=) / sync.  `warm`: [B] ints or None.  Returns (results as
    numpy, launch_info, queue_used of the last launch, kernel_info)."""
    import torch

    from robotic_mpc_amd import engine

    e = engine.MpcBatchEngine(0)
    try:
        pb = e.setup(cfgs, ur10)
        bufs = e.alloc_results(pb)
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
        yt, st = dev(sched), dev(surf)
        wt = None if warm is None else dev(np.asarray(warm, dtype=np.int32))
        pt = None if pert is None else {k: dev(v) for k, v in pert.items()}
        bounds = [0] + list(splits or []) + [pb.Nsim]
        for s0, s1 in zip(bounds[:-1], bounds[1:]):
            e.rollout(bufs, s0, s1, yref=yt, pert=pt, surf=st, warm=wt)
            e.sync()
        return {k: v.cpu().numpy() for k, v in bufs.items()}, e.launch_info(), e.queue_used(), e.kernel_info()
    finally:
        e.close()


def _step_loop(orc, raw, sched, pert, eng, modes, surf=None):
    """The reference: test_gpu_rollout_pert._step_loop with shift = (modes == SHIFT) from step 1 on, and surface = window t of the
    table where one is given."""
    from robotic_mpc_amd import BatchController

    cfgs = tp._resolve(raw)
    ctl = BatchController([{k: v for k, v in r.items() if k not in ("surface_schedule", "warm_start")} for r in raw], engine=eng)
    B, S, N = len(cfgs), cfgs[0]["Nsim"], max(c["N"] for c in cfgs)
    mask = np.asarray(modes) == SHIFT
    o = dict(z=np.zeros((B, 12, S + 1)), u=np.zeros((B, 6, S + 1)), cost=np.zeros((B, S)), residuals=np.zeros((B, S, 4)),
             status=np.zeros((B, S), np.int32), sqp_iter=np.zeros((B, S), np.int32), qp_iter=np.zeros((B, S), np.int32))
    z = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    o["z"][:, :, 0] = z
    o["u"][:, :, 0] = np.stack([c["qdot0"] for c in cfgs])
    for t in range(S):
        kw = {} if surf is None else dict(surface=np.ascontiguousarray(surf[:, t:t + N]))
        r = {n: v.cpu().numpy() for n, v in ctl.step(z + pert["x_noise"][:, t], yref=np.ascontiguousarray(sched[:, t:t + N]),
                                                     shift=mask if t >= 1 and mask.any() else False, **kw).items()}
        for k in ("cost", "residuals") + INTS:
            o[k][:, t] = r[k]
        z = np.stack([orc.plant_step(c["plant_integrator"], pert["wcv"][i], c["dt"], z[i], r["u0"][i] + pert["u_dist"][i, t])
                      for i, c in enumerate(cfgs)])
        o["z"][:, :, t + 1], o["u"][:, :, t + 1] = z, r["u0"]
    ctl.close()
    return o


def _guards(cfgs, modes, want, carry, check=None):
    """From the reference loops alone: status 0 everywhere; a shifting simulation with N >= 2 ends more than 1e-4 from its carry
    twin in z; with N = 1 exactly on it."""
    idx = list(range(len(cfgs))) if check is None else list(check)
    assert (want["status"] == 0).all() and (carry["status"] == 0).all()
    for i in idx:
        if modes[i] != SHIFT:
            np.testing.assert_array_equal(carry["z"][i], want["z"][i])
            continue
        d = np.abs(carry["z"][i] - want["z"][i]).max()
        if cfgs[i]["N"] >= 2:
            assert d > 1e-4, (i, d)
        else:
            assert d == 0.0, (i, d)


def _compare(got, want, sched, cfgs, surf=None, check=None):
    if surf is None:
        tp._compare(got, want, sched, cfgs, check)
    else:
        ts._compare(got, want, sched, surf, cfgs, check)


def _case(orc, ur10, monkeypatch, eng, raw, waves, modes=None, check=None, with_surface=False):
    from robotic_mpc_amd import plant, reference, surface

    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs = tp._resolve(raw)
    modes = np.full(len(cfgs), SHIFT, np.int32) if modes is None else np.asarray(modes, np.int32)
    sched, pert = reference.stack(cfgs), plant.stack(cfgs)
    surf = surface.stack(cfgs) if with_surface else None
    want = _step_loop(orc, raw, sched, pert, eng, modes, surf)
    carry = _step_loop(orc, raw, sched, pert, eng, np.zeros(len(cfgs), np.int32), surf)
    _guards(cfgs, modes, want, carry, check)
    got, info, _, _ = _rollout(cfgs, ur10, sched, pert, modes, surf)
    assert (info["engine"], info["waves_per_sim"]) == ((0, waves) if eng == "latency" else (1, 1)), info
    _compare(got, want, sched, cfgs, surf, check)
    return got, want, cfgs


# ------------------------------------------------------------------------------------------------------------ latency engine
@pytest.mark.parametrize("n,N,steps,waves", [(4, 12, 14, 4), (3, 100, 6, 8), (2, 224, 3, 8), (4, 12, 14, 2), (4, 12, 14, 1)])
def test_latency_engine_with_the_shift_warm_start(orc, ur10, monkeypatch, n, N, steps, waves):
    if waves < 4:      # <2> and <1>: mpcb_setup never picks them by itself
        monkeypatch.setenv("MPCB_WAVES_PER_SIM", str(waves))
    _case(orc, ur10, monkeypatch, "latency", tp._raw(n, N, steps, seed=1), waves)


def test_latency_engine_two_simulations_per_cu(orc, ur10, monkeypatch):
    n = tp._num_cus() + 64
    _case(orc, ur10, monkeypatch, "latency", tp._raw(n, 12, 5, seed=2), 4, check=range(0, n, 20))


def test_tight_bounds_take_both_qp_paths(orc, ur10, monkeypatch):
    """The bounds of the rti_tight_bounds fixture: steps solved by the fast path (qp_iter 1) and by the interior point (more) --
    the multipliers and slacks of the state bounds move with their stages."""
    _, want, _ = _case(orc, ur10, monkeypatch, "latency", tp._raw(4, 15, 14, seed=4, **tp.TIGHT), 4)
    assert (want["qp_iter"] > 1).any() and (want["qp_iter"] == 1).any()


# --------------------------------------------------------------------------------------------------------- throughput engine
def test_throughput_engine_with_the_shift_warm_start(orc, ur10, monkeypatch):
    _case(orc, ur10, monkeypatch, "stream", tp._raw(6, 12, 14, seed=5), 1)


def test_throughput_engine_ragged_horizons(orc, ur10, monkeypatch):
    """Horizons {5, 9, 12} in one launch: every simulation shifts over its own horizon and propagates the tail at its own end."""
    _, _, cfgs = _case(orc, ur10, monkeypatch, "stream", tp._raw(6, (5, 9, 12), 14, seed=7), 1)
    assert sorted({c["N"] for c in cfgs}) == [5, 9, 12]


@pytest.mark.parametrize("N,seed", [(1, 21), (2, 6)])
def test_throughput_engine_short_horizons(orc, ur10, monkeypatch, N, seed):
    """N = 1: the shift moves nothing that reaches u0 -- the one input is held, x_0 is replaced by the feedback state, x_1 is formed
    from the two -- so the guard asserts that the two reference loops agree EXACTLY in z.  They do in exact arithmetic; the step
    forms the new x_0 as x_0 + (x_hat - x_0), which rounds by the x_0 it starts from, so on some draws the loops part by one unit
    in the last place (measured over seeds 6, 16 .. 22 of _raw(3, 1, 10): 0 to 1.1e-16 in z).  Seed 21 is a draw on which they
    are equal to the bit, in z and in u, for all three simulations: another seed, not another bound."""
    _case(orc, ur10, monkeypatch, "stream", tp._raw(3, N, 10, seed=seed), 1)


def test_throughput_engine_work_queue_is_bit_identical_to_the_plain_launch(orc, ur10, monkeypatch):
    """Batch 8, 11 steps, 4 resident wavefronts, chunks of 3 steps: every chunk of every simulation changes hands, and a chunk that
    starts at step t >= 1 shifts first, whichever wavefront ran the one before."""
    from robotic_mpc_amd import plant, reference

    monkeypatch.setenv("MPCB_ENGINE", "stream")
    raw = tp._raw(8, 12, 11, seed=8)
    cfgs = tp._resolve(raw)
    sched, pert = reference.stack(cfgs), plant.stack(cfgs)
    modes = np.full(8, SHIFT, np.int32)
    plain, info, used, _ = _rollout(cfgs, ur10, sched, pert, modes)
    assert info["engine"] == 1 and not used
    monkeypatch.setenv("MPCB_STREAM_SLOTS", "4")
    monkeypatch.setenv("MPCB_STREAM_CHUNK", "3")
    queued, info, used, _ = _rollout(cfgs, ur10, sched, pert, modes)
    assert info["engine"] == 1 and used
    for k in plain:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(plain[k], queued[k], err_msg=k)
    monkeypatch.delenv("MPCB_STREAM_SLOTS")
    monkeypatch.delenv("MPCB_STREAM_CHUNK")
    want = _step_loop(orc, raw, sched, pert, "stream", modes)
    carry = _step_loop(orc, raw, sched, pert, "stream", np.zeros(8, np.int32))
    _guards(cfgs, modes, want, carry)
    _compare(queued, want, sched, cfgs)


# ------------------------------------------------------------------------------------------------------------- both engines
@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_launch_split_is_bit_identical(ur10, monkeypatch, eng):
    """Split at steps 5 and 9 of 12: the first step of a later launch shifts, the run's first step does not."""
    from robotic_mpc_amd import plant, reference

    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs = tp._resolve(tp._raw(4, 12, 12, seed=9))
    sched, pert = reference.stack(cfgs), plant.stack(cfgs)
    modes = np.full(4, SHIFT, np.int32)
    one, info, _, _ = _rollout(cfgs, ur10, sched, pert, modes)
    assert info["engine"] == (0 if eng == "latency" else 1)
    two, _, _, _ = _rollout(cfgs, ur10, sched, pert, modes, splits=[5, 9])
    for k in one:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(one[k], two[k], err_msg=k)
    # (and it is not the carried rollout that both produce)
    ref, _, _, _ = tp._rollout(cfgs, ur10, sched, pert)
    assert np.abs(ref["z"] - one["z"]).max() > 1e-4


@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_mixed_modes_match_their_loop(orc, ur10, monkeypatch, eng):
    """Carry, shift, a value that is neither (it carries), shift: each simulation against its own loop."""
    _case(orc, ur10, monkeypatch, eng, tp._raw(4, 12, 14, seed=13), 4 if eng == "latency" else 1, modes=[CARRY, SHIFT, 7, SHIFT])


@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_shift_over_a_varying_surface_table(orc, ur10, monkeypatch, eng):
    """The surface window slides with the reference window: mpcb_step_surf takes the place of mpcb_step_warm in the loop."""
    _case(orc, ur10, monkeypatch, eng, ts._raw(4, 12, 14, seed=14), 4 if eng == "latency" else 1, modes=[SHIFT, SHIFT, CARRY, SHIFT],
          with_surface=True)


@pytest.mark.parametrize("eng", ["latency", "stream"])
def test_null_cases(ur10, monkeypatch, eng):
    """warm == NULL is mpcb_rollout_surf / mpcb_rollout_pert bit for bit, on their kernels; all-carry through the kernels of this
    rollout gives the perturbed rollout's results."""
    import torch

    from robotic_mpc_amd import engine

    monkeypatch.setenv("MPCB_ENGINE", eng)
    cfgs, sched, _, pert, surf = ts._inputs(ts._raw(4, 12, 14, seed=10))
    ref, info, _, kinfo = tp._rollout(cfgs, ur10, sched, pert)
    assert info["engine"] == (0 if eng == "latency" else 1)
    sref, _, _, ksurf = ts._rollout(cfgs, ur10, sched, pert, surf)
    e = engine.MpcBatchEngine(0)
    try:
        pb = e.setup(cfgs, ur10)
        bufs = e.alloc_results(pb)
        keep = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in (sched, pert["wcv"], pert["u_dist"], pert["x_noise"], surf)]
        ptr = [C.cast(C.c_void_p(t.data_ptr()), _dp) for t in keep]
        p = engine.MpcbPlantPert(ptr[1], ptr[2], ptr[3])
        r = e._result_struct(bufs)
        for sp, want, kw in ((None, ref, kinfo), (ptr[4], sref, ksurf)):
            assert e.lib.mpcb_rollout_warm(e._h, 0, pb.Nsim, C.byref(r), ptr[0], C.byref(p), sp, None, None) == 0
            e.sync()
            for k, v in bufs.items():
                if k not in ("solver_time", "plant_time"):
                    np.testing.assert_array_equal(v.cpu().numpy(), want[k], err_msg=k)
            assert e.kernel_info() == kw                                      # (the kernel of the entry it hands on to)
    finally:
        e.close()
    got, _, _, kshift = _rollout(cfgs, ur10, sched, pert, np.zeros(4, np.int32))
    for k in ("z", "u", "ee_pose", "ee_rpy", "ee_vel", "errors"):
        np.testing.assert_allclose(got[k], ref[k], atol=1e-9, rtol=0, err_msg=k)
    np.testing.assert_allclose(got["cost"], ref["cost"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(got["residuals"], ref["residuals"], atol=1e-9, rtol=1e-6)
    for k in INTS:
        np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
    assert kshift["vgprs"] > 0                                                # (this rollout's kernel reports itself)
    same = all(np.array_equal(got[k], ref[k]) for k in got if k not in ("solver_time", "plant_time"))
    print(f"\n[shift] {eng}: all-carry through the new kernels is {'bit-identical to' if same else 'NOT bit-identical to'} the perturbed "
          f"rollout; kernel_info perturbed {kinfo}, shift {kshift}")


# ----------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(ur10):
    import torch

    from robotic_mpc_amd import engine, plant, reference

    raw = tp._raw(3, 12, 6, seed=11)
    cfgs = tp._resolve(raw)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
    y = dev(reference.stack(cfgs))
    pt = {k: dev(v) for k, v in plant.stack(cfgs).items()}
    wt = dev(np.full(3, SHIFT, np.int32))
    e = engine.MpcBatchEngine(0)
    try:
        # a controller handle
        pb = e.setup_controller(cfgs, ur10)
        bufs = e.alloc_results(pb)
        with pytest.raises(engine.EngineError, match=r"\(-5\)"):                 # MPCB_ESTATE
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, warm=wt)
        # the fp32 leg
        e.setup(tp._resolve(tp._raw(3, 12, 6, seed=11, schedule=None, which=None, riccati_precision="fp32")), ur10)
        with pytest.raises(engine.EngineError, match=r"\(-1\).*fp64"):           # MPCB_EINVAL
            e.rollout(bufs, 0, pb.Nsim, yref=y, warm=wt)
        # full SQP
        e.setup(tp._resolve(tp._raw(3, 12, 6, seed=11, solver="SQP")), ur10)
        with pytest.raises(engine.EngineError, match=r"\(-1\).*SQP_RTI"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, warm=wt)
        # without a reference schedule, at the C level; the step-range rules of mpcb_rollout
        e.setup(cfgs, ur10)
        r = e._result_struct(bufs)
        yp = C.cast(C.c_void_p(y.data_ptr()), _dp)
        wp = C.cast(C.c_void_p(wt.data_ptr()), _ip)
        assert e.lib.mpcb_rollout_warm(e._h, 0, pb.Nsim, C.byref(r), None, None, None, wp, None) == -1
        assert b"schedule" in e.lib.mpcb_last_error(e._h)
        assert e.lib.mpcb_rollout_warm(e._h, 2, pb.Nsim, C.byref(r), yp, None, None, wp, None) == -5
        assert e.lib.mpcb_rollout_warm(e._h, 0, pb.Nsim + 1, C.byref(r), yp, None, None, wp, None) == -1
        # wrong shapes and combinations never reach the library (the handle's error text stays that of the call above)
        before = e.lib.mpcb_last_error(e._h)
        with pytest.raises(ValueError, match="warm"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, warm=wt[:-1].contiguous())
        with pytest.raises(ValueError, match="warm"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, warm=wt.long())
        with pytest.raises(ValueError, match="warm"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, warm=wt.cpu())
        with pytest.raises(ValueError, match="yref"):
            e.rollout(bufs, 0, pb.Nsim, pert=pt, warm=wt)
        with pytest.raises(ValueError, match="obs"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, warm=wt, obs={})
        with pytest.raises(ValueError, match="term"):
            e.rollout(bufs, 0, pb.Nsim, yref=y, warm=wt, term={})
        assert e.lib.mpcb_last_error(e._h) == before
        # ... and the handle still runs
        e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pt, warm=wt)
        e.sync()
        assert (bufs["status"].cpu().numpy() == 0).all()
    finally:
        e.close()
    with pytest.raises(ValueError, match="warm"):
        engine.MpcBatchEngine(0).run_host_buffers(tp._resolve(tp._raw(3, 12, 6, seed=11, schedule=None, which=None, warm_start="shift")), ur10)


# ----------------------------------------------------------------------------------------------------------- public interface
def test_grid_over_the_warm_start_through_run_all(ur10):
    """warm_start x w_u through SimulationManager.run_all: ONE bucket and one launch (the mode is per simulation), results in queue
    order; a shift member ends more than 1e-4 from its carry twin in q; each member equals its own single Simulator.run."""
    from robotic_mpc_amd import SimulationManager, Simulator, base_params

    base = base_params(simulation_time=0.14 + 1e-9, prediction_horizon=12, solver_options={"nlp_solver_type": "SQP_RTI"},
                       reference_schedule=tp.SERP)
    grid = {"warm_start": ["carry", "shift"], "w_u": [0.01, 0.002]}
    m = SimulationManager(base)
    m.grid_search(grid)
    res = m.run_all()
    assert m.last_run_info["buckets"] == 1 and base.get("warm_start", "carry") == "carry"
    order = [(w, u) for w in ("carry", "shift") for u in (0.01, 0.002)]
    assert [(r["simulator"].resolved["warm_start"], r["simulator"].resolved["w_u"]) for r in res] == order
    for r in res:
        assert (r["simulator"].solver_status == 0).all()
    for j in range(2):
        assert np.abs(res[j]["data"]["q"] - res[2 + j]["data"]["q"]).max() > 1e-4, j
    assert np.abs(res[2]["data"]["q"] - res[3]["data"]["q"]).max() > 1e-4        # (and the weight matters)
    for r, (w, u) in zip(res, order):
        sim = Simulator(**{**base, "warm_start": w, "w_u": u})
        sim.run()
        d = sim.get_data()
        # a carry member alone takes the scheduled rollout's kernels, in the grid those of this rollout: the same closed loop at
        # the tolerances of _compare; a shift member runs the same kernels both times
        for k in ("q", "qdot", "u"):
            np.testing.assert_allclose(r["data"][k], d[k], atol=1e-9 if w == "carry" else 0, rtol=0, err_msg=f"{w} {u} {k}")
