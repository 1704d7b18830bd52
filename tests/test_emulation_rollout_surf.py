"""Host emulation of the rollout over a scheduled, stage-varying surface (Engine<.., 0, 0, 1>::rollout<true, true>, the device code
behind mpcb_rollout_surf on the latency engine) against what defines it: the loop of test_emulation_rollout_pert.py whose step is
the emulated controller step WITH a surface window (Engine<.., 0, 0, 1>::control_step), given at every step t rows [t, t + N) of
the table.  Both sides run the same passes on the same data: they agree to 1e-12, the emulation tier's bound, on every log, and the
error log is the host's recomputation from surface row t and reference row t.  A larger distance is a wiring bug.

4 simulations, N = 12, 14 steps; bandwidth scale 0.8, a step disturbance from step 3, Gaussian measurement noise; tables that vary
curvature, slope and height over the rows (tests/step_surf_cases.py variation).  Before it compares, every test asserts from the
reference loop alone that every step has status 0 and that the loop on the constant surface ends up more than 1e-4 away in z."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import step_surf_cases as ss  # noqa: E402
import test_emulation_rollout_pert as tp  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

B, N, STEPS, START = 4, 12, 14, 3
WAVES = (4, 8, 2, 1)
INTS = tp.INTS


def _cfgs(constant=False):
    from robotic_mpc_amd import config

    out = []
    for i in range(B):
        q0 = np.asarray(config.BASE_PARAMS["q_0"]) + 0.01 * np.array([5, -4, 3, 2, -3, 4]) * (1 + i)
        val = [[0.05] * 6, [0.05, -0.05, 0.05, 0.0, 0.05, -0.05], [-0.03] * 6, [0.02, 0.04, -0.06, 0.05, -0.01, 0.03]][i]
        pert = {"wcv_scale": 0.8, "input_disturbance": {"kind": "step", "start_time": 0.01 * START, "value": val},
                "measurement_noise": {"kind": "gaussian", "sigma_q": 1e-3, "sigma_qdot": 1e-2, "seed": 40 + i}}
        base = np.array([config.DEFAULT_SURFACE_COEFFS[k] for k in "abcdef"])
        tab = np.tile(base, (STEPS + N, 1)) if constant else base[None] + ss.variation(STEPS + N, 3000 + i)
        out.append(config.resolve_config(config.base_params(
            prediction_horizon=N, simulation_time=0.01 * STEPS + 1e-9, solver_options={"nlp_solver_type": "SQP_RTI"}, q_0=q0,
            w_u=0.01 if i % 2 == 0 else 0.002, reference_schedule=tp.SERPENTINE, plant_perturbation=pert,
            surface_schedule={"kind": "table", "rows": tab.tolist()})))
    return out


def _loop(cfgs, chain, sched, pert, surf, waves):
    """The yardstick: the emulated controller step with surface = rows [t, t + N) of the table (surf None: the plain step on the
    packed surface), from z + x_noise[t], over the perturbed plant step on the host."""
    import emu_rollsurf

    ctl = emu_rollsurf.Controller(cfgs, chain, waves=waves)
    zt = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    o = dict(z=np.zeros((B, 12, STEPS + 1)), u=np.zeros((B, 6, STEPS + 1)), cost=np.zeros((B, STEPS)), residuals=np.zeros((B, STEPS, 4)),
             status=np.zeros((B, STEPS), np.int32), sqp_iter=np.zeros((B, STEPS), np.int32), qp_iter=np.zeros((B, STEPS), np.int32))
    o["z"][:, :, 0] = zt
    o["u"][:, :, 0] = np.stack([c["qdot0"] for c in cfgs])
    for t in range(STEPS):
        kw = {} if surf is None else dict(surface=surf[:, t:t + N])
        out = ctl.step(zt + pert["x_noise"][:, t], yref=sched[:, t:t + N], ref_changed=True, predict=False, **kw)
        for k in ("cost", "residuals") + INTS:
            o[k][:, t] = out[k]
        zt = np.stack([emu_rollsurf.plant_rk(c, pert["wcv"][i], zt[i], out["u0"][i] + pert["u_dist"][i, t]) for i, c in enumerate(cfgs)])
        o["z"][:, :, t + 1] = zt
        o["u"][:, :, t + 1] = out["u0"]
    return o


def _compare(got, want, cfgs, sched, surf):
    """test_emulation_rollout_pert._compare with the error log measured against surface row t as well."""
    from robotic_mpc_amd import analysis

    np.testing.assert_allclose(got["cost"], want["cost"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["residuals"], want["residuals"], rtol=0, atol=1e-12)
    for k in INTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    np.testing.assert_allclose(got["z"], want["z"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["u"], want["u"], rtol=0, atol=1e-12)
    for i, c in enumerate(cfgs):
        e = analysis.errors_rows(analysis.compute_errors(got["ee_pose"][i], got["ee_vel"][i], surf[i, :STEPS + 1].T, c["t_ee"], c["px_ref"],
                                                         c["vy_ref"], yref=sched[i, :STEPS + 1]))
        np.testing.assert_allclose(got["errors"][i], e, rtol=0, atol=1e-12)
        # ... and not against the packed coefficients
        p = analysis.errors_rows(analysis.compute_errors(got["ee_pose"][i], got["ee_vel"][i], c["coeffs"], c["t_ee"], c["px_ref"],
                                                         c["vy_ref"], yref=sched[i, :STEPS + 1]))
        assert np.abs(p - e).max() > 1e-4


_CACHE = {}


def _inputs(ur10, waves):
    """(cfgs, sched, pert, surf, the reference loop at `waves`): computed once per geometry, shared, never written to."""
    from robotic_mpc_amd import plant, reference, surface

    if waves not in _CACHE:
        cfgs = _cfgs()
        sched, pert, surf = reference.stack(cfgs), plant.stack(cfgs), surface.stack(cfgs)
        _CACHE[waves] = (cfgs, sched, pert, surf, _loop(cfgs, ur10, sched, pert, surf, waves))
    return _CACHE[waves]


def _rollout(ur10, waves, **kw):
    import emu_rollsurf

    cfgs, sched, pert, surf, _ = _inputs(ur10, waves)
    return emu_rollsurf.rollout(cfgs, ur10, sched, surf, **pert, waves=waves, **kw)


def test_the_case_is_the_one_described():
    from robotic_mpc_amd import surface

    cfgs = _cfgs()
    surf = surface.stack(cfgs)
    assert surf.shape == (B, STEPS + N, 6) and all(c["N"] == N and c["Nsim"] == STEPS for c in cfgs)
    assert (np.ptp(surf, axis=1) > 1e-3).all()               # every coefficient of every simulation moves: curvature, slope, height
    np.testing.assert_array_equal(surface.log_rows(cfgs[1]), surf[1, :STEPS + 1])


@pytest.mark.parametrize("waves", WAVES)
def test_emulated_rollout_over_a_scheduled_surface_is_the_loop_of_its_step(ur10, waves):
    cfgs, sched, pert, surf, want = _inputs(ur10, waves)
    assert (want["status"] == 0).all()
    without = _loop(cfgs, ur10, sched, pert, None, waves)
    assert np.abs(without["z"] - want["z"]).max() > 1e-4
    got = _rollout(ur10, waves)
    _compare(got, want, cfgs, sched, surf)


def test_emulated_rollout_does_not_depend_on_the_launch_boundary(ur10):
    """Chunks of 3 steps: a launch finds its rows by the absolute step number."""
    a = _rollout(ur10, 4)
    b = _rollout(ur10, 4, step_chunk=3)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_all_equal_schedule_is_the_perturbed_rollout(ur10):
    """The packed coefficients on every row: the logs are the perturbed rollout's, through the new code."""
    import emu_rollpert
    import emu_rollsurf
    from robotic_mpc_amd import plant, reference, surface

    cfgs = _cfgs(constant=True)
    sched, pert, surf = reference.stack(cfgs), plant.stack(cfgs), surface.stack(cfgs)
    assert (surf == np.stack([c["coeffs"] for c in cfgs])[:, None]).all()
    got = emu_rollsurf.rollout(cfgs, ur10, sched, surf, **pert, waves=4)
    want = emu_rollpert.rollout(cfgs, ur10, sched, **pert, waves=4)
    assert (want["status"] == 0).all()
    for k in ("z", "u", "ee_pose", "ee_rpy", "ee_vel", "errors", "cost", "residuals"):
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-12, err_msg=k)
    for k in INTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
