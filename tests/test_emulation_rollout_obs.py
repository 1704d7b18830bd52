"""Host emulation of the rollout with an on-device disturbance observer (Engine<.., 0, DIST_SHARED>::rollout<true, true, true>, the
device code behind mpcb_rollout_obs on the latency engine) against what defines it: the loop of test_emulation_rollout_pert.py whose
step is the emulated controller step WITH an input disturbance (Engine<.., 0, true>::control_step), given at every step t the
estimate of the torch DisturbanceObserver (robotic_mpc_amd/observer.py) that measured z_t + noise_t and the commanded u_{t-1}.  Both
sides run the same passes on the same data, and the observer's two recurrences differ in the order of a few operations (the kernel
forms the next estimate one step early, with fused multiply-adds): they agree to 1e-12, the emulation tier's bound, on every log and
on d_hat.  A larger distance is a wiring bug.

4 simulations, N = 12, 14 steps; bandwidth scale 0.8, a step disturbance from step 3, Gaussian measurement noise; poles 0 and 0.2.
Before it compares, every test asserts from the reference loop alone that every step has status 0, that d_hat leaves zero and that
the loop without the observer ends up more than 1e-4 away in z."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import test_emulation_rollout_pert as tp  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

B, N, STEPS, START = 4, 12, 14, 3
POLES = (0.0, 0.2, 0.2, 0.0)
WAVES = (4, 8, 2, 1)
INTS = tp.INTS
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rollout_obs_closed_loop.txt")


def _cfgs(observer=True):
    from robotic_mpc_amd import config

    out = []
    for i in range(B):
        q0 = np.asarray(config.BASE_PARAMS["q_0"]) + 0.01 * np.array([5, -4, 3, 2, -3, 4]) * (1 + i)
        val = [[0.05] * 6, [0.05, -0.05, 0.05, 0.0, 0.05, -0.05], [-0.03] * 6, [0.02, 0.04, -0.06, 0.05, -0.01, 0.03]][i]
        pert = {"wcv_scale": 0.8, "input_disturbance": {"kind": "step", "start_time": 0.01 * START, "value": val},
                "measurement_noise": {"kind": "gaussian", "sigma_q": 1e-3, "sigma_qdot": 1e-2, "seed": 40 + i}}
        out.append(config.resolve_config(config.base_params(
            prediction_horizon=N, simulation_time=0.01 * STEPS + 1e-9, solver_options={"nlp_solver_type": "SQP_RTI"}, q_0=q0,
            w_u=0.01 if i % 2 == 0 else 0.002, reference_schedule=tp.SERPENTINE, plant_perturbation=pert,
            disturbance_observer={"pole": POLES[i]} if observer else None)))
    return out


def _loop(cfgs, chain, sched, pert, waves, observer=True):
    """The yardstick: the emulated controller step with dist = d_hat_t of the torch observer (or without one), from z + x_noise[t],
    over the perturbed plant step on the host."""
    import torch

    import emu_rollobs
    from robotic_mpc_amd.observer import DisturbanceObserver

    ctl = emu_rollobs.Controller(cfgs, chain, waves=waves)
    obs = [DisturbanceObserver(c["wcv"], c["dt"], c["disturbance_observer"]["pole"]) for c in cfgs] if observer else None
    zt = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    o = dict(z=np.zeros((B, 12, STEPS + 1)), u=np.zeros((B, 6, STEPS + 1)), cost=np.zeros((B, STEPS)), residuals=np.zeros((B, STEPS, 4)),
             status=np.zeros((B, STEPS), np.int32), sqp_iter=np.zeros((B, STEPS), np.int32), qp_iter=np.zeros((B, STEPS), np.int32),
             d_hat=np.zeros((B, STEPS, 6)))
    o["z"][:, :, 0] = zt
    o["u"][:, :, 0] = np.stack([c["qdot0"] for c in cfgs])
    u_prev = np.zeros((B, 6))
    for t in range(STEPS):
        xhat = zt + pert["x_noise"][:, t]
        kw = {}
        if observer:
            d = np.stack([ob.update(torch.from_numpy(xhat[i:i + 1]), torch.from_numpy(u_prev[i:i + 1])).numpy()[0] for i, ob in enumerate(obs)])
            o["d_hat"][:, t] = d
            kw["dist"] = d
        out = ctl.step(xhat, yref=sched[:, t:t + N], ref_changed=True, predict=False, **kw)
        for k in ("cost", "residuals") + INTS:
            o[k][:, t] = out[k]
        zt = np.stack([emu_rollobs.plant_rk(c, pert["wcv"][i], zt[i], out["u0"][i] + pert["u_dist"][i, t]) for i, c in enumerate(cfgs)])
        o["z"][:, :, t + 1] = zt
        o["u"][:, :, t + 1] = out["u0"]
        u_prev = out["u0"].copy()
    return o


_CACHE = {}


def _inputs(ur10, waves):
    """(cfgs, sched, pert, gain, the reference loop at `waves`): computed once per geometry, shared, never written to."""
    from robotic_mpc_amd import observer, plant, reference

    if waves not in _CACHE:
        cfgs = _cfgs()
        sched, pert = reference.stack(cfgs), plant.stack(cfgs)
        _CACHE[waves] = (cfgs, sched, pert, observer.stack(cfgs), _loop(cfgs, ur10, sched, pert, waves))
    return _CACHE[waves]


def _rollout(ur10, waves, **kw):
    import emu_rollobs

    cfgs, sched, pert, gain, _ = _inputs(ur10, waves)
    return emu_rollobs.rollout(cfgs, ur10, sched, gain, **pert, waves=waves, **kw)


def test_the_case_is_the_one_described():
    from robotic_mpc_amd import plant

    cfgs = _cfgs()
    pert = plant.stack(cfgs)
    assert len(cfgs) == 4 and all(c["N"] == 12 and c["Nsim"] == 14 for c in cfgs)
    assert sorted({c["disturbance_observer"]["pole"] for c in cfgs}) == [0.0, 0.2]
    assert (pert["u_dist"][:, :START] == 0).all() and (np.abs(pert["u_dist"][:, START:]).max(axis=(1, 2)) > 0).all()
    np.testing.assert_allclose(pert["wcv"], 0.8 * np.stack([c["wcv"] for c in cfgs]))
    assert np.abs(pert["x_noise"]).min() > 0


@pytest.mark.parametrize("waves", WAVES)
def test_emulated_rollout_with_an_observer_is_the_loop_of_the_disturbed_step(ur10, waves):
    cfgs, sched, pert, gain, want = _inputs(ur10, waves)
    assert (want["status"] == 0).all()
    # it does something: the estimate leaves zero, and the loop without it ends up elsewhere
    assert (want["d_hat"][:, 0] == 0).all() and (np.abs(want["d_hat"][:, -1]).max(axis=1) > 1e-3).all()
    without = _loop(cfgs, ur10, sched, pert, waves, observer=False)
    assert np.abs(without["z"] - want["z"]).max() > 1e-4
    got = _rollout(ur10, waves)
    tp._compare(got, want, cfgs, sched)
    np.testing.assert_allclose(got["d_hat"], want["d_hat"], rtol=0, atol=1e-12)


def test_observer_replayed_on_the_logs_gives_the_logged_estimates(ur10):
    """Independent of the step loop: DisturbanceObserver over the rollout's own logged z + noise and u reproduces d_hat."""
    import torch

    from robotic_mpc_amd.observer import DisturbanceObserver

    cfgs, _, pert, _, _ = _inputs(ur10, 4)
    got = _rollout(ur10, 4)
    assert np.isfinite(got["d_hat"]).all() and np.abs(got["d_hat"]).max() > 1e-3
    for i, c in enumerate(cfgs):
        ob = DisturbanceObserver(c["wcv"], c["dt"], c["disturbance_observer"]["pole"])
        for t in range(STEPS):
            x = torch.from_numpy((got["z"][i, :, t] + pert["x_noise"][i, t])[None])
            u = torch.from_numpy(got["u"][i, :, t][None].copy()) if t else torch.zeros(1, 6, dtype=torch.float64)
            np.testing.assert_allclose(ob.update(x, u).numpy()[0], got["d_hat"][i, t], rtol=0, atol=1e-12, err_msg=f"sim {i} step {t}")


def test_emulated_rollout_does_not_depend_on_the_launch_boundary(ur10):
    """Chunks of 3 steps: from step 3 on the disturbance acts, so ST_OBS carries a non-zero estimate across every later boundary."""
    a = _rollout(ur10, 4)
    assert np.abs(a["d_hat"][:, 6]).min(axis=0).max() > 0 and np.abs(a["d_hat"][:, 9]).max() > 1e-3
    b = _rollout(ur10, 4, step_chunk=3)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_zero_disturbance_gain_is_the_perturbed_rollout(ur10):
    """l2 = 0: d_hat stays zero and the logs are the perturbed rollout's."""
    import emu_rollobs
    import emu_rollpert

    cfgs, sched, pert, gain, _ = _inputs(ur10, 4)
    g0 = gain.copy()
    g0[:, 6:] = 0.0
    got = emu_rollobs.rollout(cfgs, ur10, sched, g0, **pert, waves=4)
    want = emu_rollpert.rollout(cfgs, ur10, sched, **pert, waves=4)
    assert (got["d_hat"] == 0).all()
    for k in ("z", "u", "ee_pose", "ee_rpy", "ee_vel", "errors", "cost", "residuals"):
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-12, err_msg=k)
    for k in INTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


def test_compensation_ratio_over_the_rollouts_own_plant(ur10, capsys):
    """The figures of tests/step_dist_closed_loop.py (N = 10, 4 simulations that differ in a constant d alone, uniform +-0.1, seed
    970; pole 0.2; 3 K steps), over the rollout's own RK4 plant with the model's bandwidths: the deviation of the task errors from
    the nominal run over the last third, with the observer and without.  Asserted: ratio < 1.  The measured value is printed and
    kept in profiles/rollout_obs_closed_loop.txt."""
    import emu_rollobs
    import emu_rollpert
    import step_dist_closed_loop as cl
    from robotic_mpc_amd import config, observer, reference
    from robotic_mpc_amd.observer import DisturbanceObserver

    raw = cl.raw_config()
    c0 = config.resolve_config(raw)
    K = cl.settle_steps(DisturbanceObserver(np.asarray(c0["wcv"], float), c0["dt"], pole=cl.POLE))
    steps = 3 * K
    d = cl.disturbance()
    raw = {**raw, "simulation_time": c0["dt"] * steps + 1e-9, "disturbance_observer": {"pole": cl.POLE}}
    cfgs = [config.resolve_config(raw) for _ in range(cl.B)]
    assert cfgs[0]["Nsim"] == steps and cfgs[0]["N"] == cl.N
    rows = steps + cl.N
    sched = np.stack([reference.packed_rows(c, rows) for c in cfgs])
    u_dist = np.repeat(d[:, None, :], steps, axis=1)
    nom = emu_rollpert.rollout(cfgs, ur10, sched, waves=4)
    unc = emu_rollpert.rollout(cfgs, ur10, sched, u_dist=u_dist, waves=4)
    comp = emu_rollobs.rollout(cfgs, ur10, sched, observer.stack(cfgs), u_dist=u_dist, waves=4)
    assert (nom["status"] == 0).all() and (unc["status"] == 0).all() and (comp["status"] == 0).all()
    last = slice(steps + 1 - steps // 3, steps + 1)
    e = lambda o: o["errors"][:, :5, last]   # noqa: E731
    dev_comp, dev_unc = float(np.abs(e(comp) - e(nom)).max()), float(np.abs(e(unc) - e(nom)).max())
    d_err = float(np.abs(comp["d_hat"][:, K:] - d[:, None, :]).max())
    ratio = dev_comp / dev_unc
    with capsys.disabled():
        print(f"\nrollout_obs closed loop: K = {K}, steps = {steps}, max|d_hat - d| from step K on = {d_err:.3e}, "
              f"dev_comp = {dev_comp:.6e}, dev_unc = {dev_unc:.6e}, ratio = {ratio:.4f}")
    assert dev_unc > 0 and ratio < 1.0
    if os.path.exists(PROFILE):
        assert "ratio" in open(PROFILE).read()
