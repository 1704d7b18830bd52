"""Host emulation of the rollout against a task reference schedule (Engine::rollout<true>, the device code behind mpcb_rollout_ref
on the latency engine) against what defines it: a loop of the emulated controller step (Engine::control_step) with the window of
the step and ref_changed = 1, over the rollout's own plant step (nlp::plant_rk).  Both sides run the same passes on the same data,
so they agree to rounding of the few operations that differ in order (1e-12): a larger distance is a wiring bug."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

SERPENTINE = {"kind": "serpentine", "lanes": 2, "lane_pitch": 0.03, "lane_time": 0.02, "turn_time": 0.03}
# horizon, steps, solver, fast path, pool (0: a whole CU's), wavefronts: one case per sweep of the interior-point solve (asserted
# below from the engine's own predicates), SQP_RTI, plus one full-SQP case
CASES = [
    (20, 7, "SQP_RTI", True, 0, 4), (23, 7, "SQP_RTI", False, 2048, 2), (100, 4, "SQP_RTI", True, 9156, 4), (224, 3, "SQP_RTI", True, 0, 8),
    (12, 4, "SQP", True, 0, 2),
]


def _cfgs(N, steps, solver, fast):
    from robotic_mpc_amd import config

    q0 = np.asarray(config.BASE_PARAMS["q_0"]) + np.array([0.05, -0.04, 0.03, 0.02, -0.03, 0.04])
    kw = dict(prediction_horizon=N, simulation_time=0.01 * steps + 1e-9, solver_options={"nlp_solver_type": solver}, qp_fast_path=fast,
              reference_schedule=SERPENTINE)
    return [config.resolve_config(config.base_params(**kw, q_0=q0)),
            config.resolve_config(config.base_params(**kw, w_u=0.002, px_ref=0.38))]


def test_cases_cover_every_sweep():
    import emu

    rti = [c for c in CASES if c[2] == "SQP_RTI"]
    sweeps = [emu.emu_paths(N, pool if pool else emu.pool_doubles(1), waves)["sweep"] for N, _, _, _, pool, waves in rti]
    assert sorted(sweeps) == sorted(emu.SWEEPS), sweeps
    assert [c[2] for c in CASES].count("SQP") == 1


@pytest.mark.parametrize("N,steps,solver,fast,pool,waves", CASES)
def test_emulated_scheduled_rollout_is_the_step_loop_over_the_builtin_plant(ur10, N, steps, solver, fast, pool, waves):
    import emu_rollref
    from robotic_mpc_amd import analysis, reference

    cfgs = _cfgs(N, steps, solver, fast)
    assert cfgs[0]["Nsim"] == steps
    sched = reference.stack(cfgs)                                          # [B, Nsim + N, 5]
    assert np.abs(sched[0] - sched[1]).max() > 1e-3                        # the rows differ between the simulations
    assert (sched[0, :steps + N, 4] > 0).any() and (sched[0, :steps + N, 4] < 0).any()   # the turn lies inside run + horizon
    got = emu_rollref.rollout(cfgs, ur10, sched, pool_doubles=pool, waves=waves)

    ctl = emu_rollref.Controller(cfgs, ur10, pool_doubles=pool, waves=waves)
    B = len(cfgs)
    x = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    z = np.zeros((B, 12, steps + 1))
    u = np.zeros((B, 6, steps + 1))
    z[:, :, 0] = x
    u[:, :, 0] = np.stack([c["qdot0"] for c in cfgs])                      # u[:, 0] = qdot_0 (simulator.py:81)
    for t in range(steps):
        out = ctl.step(x, yref=sched[:, t:t + N], ref_changed=True, predict=False)
        where = f"step {t}"
        np.testing.assert_allclose(got["cost"][:, t], out["cost"], rtol=1e-12, atol=1e-12, err_msg=where)
        np.testing.assert_allclose(got["residuals"][:, t], out["residuals"], rtol=0, atol=1e-12, err_msg=where)
        for k in ("status", "sqp_iter", "qp_iter"):
            np.testing.assert_array_equal(got[k][:, t], out[k], err_msg=f"{where} {k}")
        x = np.stack([emu_rollref.plant_rk(c, x[i], out["u0"][i]) for i, c in enumerate(cfgs)])
        z[:, :, t + 1] = x
        u[:, :, t + 1] = out["u0"]
    np.testing.assert_allclose(got["z"], z, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["u"], u, rtol=0, atol=1e-12)
    # the error log: column t against schedule row t, from the rollout's own pose / velocity logs
    for i, c in enumerate(cfgs):
        want = analysis.errors_rows(analysis.compute_errors(got["ee_pose"][i], got["ee_vel"][i], c["coeffs"], c["t_ee"], c["px_ref"],
                                                            c["vy_ref"], yref=sched[i, :steps + 1]))
        np.testing.assert_allclose(got["errors"][i], want, rtol=0, atol=1e-12)
    # a rollout that ignored the schedule would log the errors of the packed reference
    packed = analysis.errors_rows(analysis.compute_errors(got["ee_pose"][0], got["ee_vel"][0], cfgs[0]["coeffs"], cfgs[0]["t_ee"],
                                                          cfgs[0]["px_ref"], cfgs[0]["vy_ref"]))
    assert np.abs(packed - got["errors"][0]).max() > 1e-3


def test_emulated_scheduled_rollout_does_not_depend_on_the_launch_boundary(ur10):
    import emu_rollref
    from robotic_mpc_amd import reference

    cfgs = _cfgs(20, 7, "SQP_RTI", True)
    sched = reference.stack(cfgs)
    a = emu_rollref.rollout(cfgs, ur10, sched, waves=4)
    b = emu_rollref.rollout(cfgs, ur10, sched, step_chunk=3, waves=4)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
