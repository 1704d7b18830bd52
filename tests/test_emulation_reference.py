"""Host emulation of the controller step against a task reference (Engine::control_step with StepIO::yref / ref_changed, the
device code behind mpcb_step_ref): a constant reference against the oracle solved with that reference packed, the RTI step
after a reference change against the exact Gauss-Newton QP step, and full SQP against a dense solve of the NLP."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import reference_checks as rc  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")


def _cfg(**kw):
    from robotic_mpc_amd import config

    return config.resolve_config(config.base_params(**kw))


def _q0():
    from robotic_mpc_amd import config

    return np.asarray(config.BASE_PARAMS["q_0"]) + np.array([0.05, -0.04, 0.03, 0.02, -0.03, 0.04])


def _plant(orc, cfg, rng):
    wcv = np.asarray(cfg["wcv"]) * 0.8

    def plant(z, u):
        return orc.plant_step(0, wcv, cfg["dt"], z, u) + rng.uniform(-1e-3, 1e-3, 12)
    return plant


@pytest.mark.parametrize("N,steps,solver,fast,waves", [(20, 8, "SQP_RTI", True, 4), (20, 5, "SQP", True, 2),
                                                       (23, 8, "SQP_RTI", False, 1), (30, 4, "SQP", False, 8)])
def test_constant_reference_matches_oracle_with_that_reference_packed(orc, ur10, ur10_rb, N, steps, solver, fast, waves):
    import emu_ref

    kw = dict(prediction_horizon=N, simulation_time=0.01 * steps, solver_options={"nlp_solver_type": solver}, qp_fast_path=fast,
              q_0=_q0())
    cfgs = [_cfg(**kw), _cfg(**kw, w_u=0.002)]                           # packed px_ref 0.40, vy_ref 0.05
    target = [_cfg(**kw, px_ref=0.33, vy_ref=0.02), _cfg(**kw, w_u=0.002, px_ref=0.33, vy_ref=0.02)]
    ctl = emu_ref.Controller(cfgs, ur10, waves=waves)
    refs = [orc.Solver(ur10_rb, orc.make_params(c)) for c in target]
    y = np.array([0.0, 1.0, 0.0, 0.33, 0.02])
    rng = np.random.default_rng(11)
    plants = [_plant(orc, c, rng) for c in cfgs]
    x = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    for k in range(steps):
        out = ctl.step(x, yref=y, ref_changed=(k == 0))
        for i, ref in enumerate(refs):
            r = ref.step(x[i])
            xr, ur, _ = ref.iterate()
            where = f"step {k} sim {i}"
            np.testing.assert_allclose(out["u0"][i], r["u0"], atol=1e-11, rtol=0, err_msg=where)
            np.testing.assert_allclose(out["x_pred"][i], xr, atol=1e-11, rtol=0, err_msg=where)
            np.testing.assert_allclose(out["u_pred"][i], ur, atol=1e-11, rtol=0, err_msg=where)
            np.testing.assert_allclose(out["cost"][i], r["cost"], atol=1e-10, rtol=1e-10, err_msg=where)
            np.testing.assert_allclose(out["residuals"][i], r["res"], atol=1e-11, rtol=1e-9, err_msg=where)
            assert (out["status"][i], out["sqp_iter"][i], out["qp_iter"][i]) == (r["status"], r["sqp_iter"], r["qp_iter"]), where
        x = np.stack([plants[i](x[i], out["u0"][i]) for i in range(len(cfgs))])


def test_rti_step_after_a_reference_change_is_the_exact_qp_step(orc, ur10, ur10_rb):
    """Every step gets a new per-stage reference: the step must linearise against it (not reuse the carried linearisation,
    formed against the previous one), so the new iterate is the old one plus the Gauss-Newton QP step under the new reference."""
    import emu_ref

    N, steps = 20, 12
    # qp_tol 1e-14: an interior-point step (fast path rejected) stops with its active components qp_tol / lam off their bounds,
    # which the 1e-10 below has to cover for multipliers down to 1e-4
    so = {"nlp_solver_type": "SQP_RTI", "qp_tol": 1e-14, "qp_solver_iter_max": 200}
    cfgs = [_cfg(prediction_horizon=N, simulation_time=0.01 * steps, q_0=_q0(), solver_options=so),
            _cfg(prediction_horizon=N, simulation_time=0.01 * steps, w_u=0.002, solver_options=so)]
    ctl = emu_ref.Controller(cfgs, ur10, waves=4)
    rng = np.random.default_rng(5)
    plants = [_plant(orc, c, rng) for c in cfgs]
    x = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    ya = np.stack([rc.ramp_reference(c, N) for c in cfgs])
    prev = None
    checked = 0
    for k in range(steps):
        y = ya if k < 4 else np.stack([rc.ramp_reference(c, N, k0=k, px0=0.36 + 0.004 * k) for c in cfgs])
        out = ctl.step(x, yref=y, ref_changed=(k == 0 or k >= 4))
        if prev is not None and k >= 4:
            for i, c in enumerate(cfgs):
                if out["qp_iter"][i] != 1:
                    # the fast path rejected: an interior-point solve, held against the exact active-set certificate of the
                    # independently assembled QP (tests/dense_qp.py)
                    want = rc.gn_qp_step(orc, ur10_rb, c, prev["x_pred"][i], prev["u_pred"][i], x[i], y[i], backend="dense",
                                         chain=ur10, candidate=(out["x_pred"][i], out["u_pred"][i]))
                else:
                    want = rc.gn_qp_step(orc, ur10_rb, c, prev["x_pred"][i], prev["u_pred"][i], x[i], y[i])
                    assert want is not None, f"step {k} sim {i}: the engine took the fast path, the oracle's rejects"
                np.testing.assert_allclose(out["x_pred"][i], want[0], atol=1e-10, rtol=0, err_msg=f"step {k} sim {i}")
                np.testing.assert_allclose(out["u_pred"][i], want[1], atol=1e-10, rtol=0, err_msg=f"step {k} sim {i}")
                checked += 1
        prev = out
        x = np.stack([plants[i](x[i], out["u0"][i]) for i in range(len(cfgs))])
    assert checked == (steps - 4) * len(cfgs)


def test_full_sqp_converges_to_the_nlp_of_the_reference(orc, ur10, ur10_rb):
    """Full SQP at a tight tolerance lands on the NLP solution under a per-stage ramp; a dense least-squares solve over the
    inputs (states eliminated) pins row k of the reference to stage k."""
    import emu_ref

    N = 12
    cfg = _cfg(prediction_horizon=N, simulation_time=0.05, q_0=_q0(),
               solver_options={"nlp_solver_type": "SQP", "nlp_solver_max_iter": 100, "nlp_solver_tol_stat": 1e-10,
                               "nlp_solver_tol_eq": 1e-10, "nlp_solver_tol_ineq": 1e-10, "nlp_solver_tol_comp": 1e-10})
    ctl = emu_ref.Controller([cfg], ur10, waves=2)
    x = np.concatenate([cfg["q0"], cfg["qdot0"]])[None]
    y = rc.ramp_reference(cfg, N, px0=0.37, dpx=0.003, vy0=0.02, dvy=0.01)[None]
    out = ctl.step(x, yref=y, ref_changed=True)
    assert out["status"][0] == 0, out
    u = rc.dense_nlp_solve(orc, ur10_rb, cfg, x[0], y[0], out["u_pred"][0])
    np.testing.assert_allclose(out["u_pred"][0], u, atol=1e-6, rtol=0)
    # the bounds are inactive at this solution (the dense solve ignores them)
    assert (out["u_pred"][0] > np.asarray(cfg["umin"]) + 1e-3).all() and (out["u_pred"][0] < np.asarray(cfg["umax"]) - 1e-3).all()
    # and the ramp matters: the packed reference gives another solution
    other = rc.dense_nlp_solve(orc, ur10_rb, cfg, x[0], np.tile(rc.g_ref(cfg), (N, 1)), out["u_pred"][0])
    assert np.abs(other - u).max() > 1e-3


def test_null_reference_reproduces_the_plain_step_bit_for_bit(ur10):
    import emu_ref
    import emu_step

    N = 20
    cfgs = [_cfg(prediction_horizon=N, simulation_time=0.06, q_0=_q0()), _cfg(prediction_horizon=N, simulation_time=0.06)]
    a, b = emu_step.Controller(cfgs, ur10, waves=4), emu_ref.Controller(cfgs, ur10, waves=4)
    rng = np.random.default_rng(2)
    x = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    for k in range(6):
        oa, ob = a.step(x), b.step(x, yref=None, ref_changed=False)
        for key in oa:
            np.testing.assert_array_equal(oa[key], ob[key], err_msg=key)
        x = x + rng.uniform(-1e-3, 1e-3, x.shape)
