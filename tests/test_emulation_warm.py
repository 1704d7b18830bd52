"""Host emulation of the controller step with a per-simulation warm start (Engine::control_step<true> with StepIO::warm, the device
code behind mpcb_step_warm) on the latency engine: a shifted RTI step against the exact Gauss-Newton QP step from the previous
prediction shifted in numpy, the three modes side by side in one batch, the path without modes, and full SQP from a shifted start."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import reference_checks as rc  # noqa: E402
import warm_checks as wc  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

# qp_tol 1e-14 / 200 iterations: the reasoning of test_gpu_controller_reference.py (an interior-point step leaves its active
# components qp_tol / lam off their bounds, which the 1e-10 below has to cover)
TIGHT_QP = {"nlp_solver_type": "SQP_RTI", "qp_tol": 1e-14, "qp_solver_iter_max": 200}


def _cfg(**kw):
    from robotic_mpc_amd import config

    return config.resolve_config(config.base_params(**kw))


def _q0(d=0.0):
    from robotic_mpc_amd import config

    return np.asarray(config.BASE_PARAMS["q_0"]) + np.array([0.05, -0.04, 0.03, 0.02, -0.03, 0.04]) + d


def _plant(orc, cfg, rng):
    wcv = np.asarray(cfg["wcv"]) * 0.8

    def plant(z, u):
        return orc.plant_step(0, wcv, cfg["dt"], z, u) + rng.uniform(-1e-3, 1e-3, 12)
    return plant


def _x0(cfgs):
    return np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])


@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("N", [1, 2, 3, 20])
def test_shifted_rti_step_is_the_exact_qp_step_from_the_shifted_iterate(orc, ur10, ur10_rb, N, waves):
    """The schedule slides one stage per step and every step but the first shifts: the new iterate is the previous prediction,
    shifted by the rule of include/mpcbatch.h, plus the Gauss-Newton QP step there -- and not the QP step from the unshifted
    prediction, which the reference alone shows to be another point (a shift that did nothing would land there)."""
    import emu_warm

    steps = 12
    cfgs = [_cfg(prediction_horizon=N, simulation_time=0.01 * steps, q_0=_q0(), solver_options=TIGHT_QP),
            _cfg(prediction_horizon=N, simulation_time=0.01 * steps, w_u=0.002, solver_options=TIGHT_QP)]
    ctl = emu_warm.Controller(cfgs, ur10, waves=waves)
    rng = np.random.default_rng(5)
    plants = [_plant(orc, c, rng) for c in cfgs]
    x = _x0(cfgs)
    prev, checked, apart = None, 0, []
    for k in range(steps):
        y = np.stack([rc.ramp_reference(c, N, k0=k) for c in cfgs])
        out = ctl.step(x, yref=y, ref_changed=True, warm=[wc.SHIFT] * len(cfgs))
        assert (out["status"] == 0).all(), f"step {k}"
        if prev is not None:
            for i, c in enumerate(cfgs):
                where = f"step {k} sim {i}"
                Xs, Us = wc.shift_iterate(orc, c, prev["x_pred"][i], prev["u_pred"][i])
                want = wc.qp_step(orc, ur10_rb, ur10, c, Xs, Us, x[i], y[i], (out["x_pred"][i], out["u_pred"][i], out["qp_iter"][i]))
                assert want is not None, f"{where}: the engine took the fast path, the oracle's rejects"
                d = max(np.abs(out["x_pred"][i] - want[0]).max(), np.abs(out["u_pred"][i] - want[1]).max())
                print(f"N {N} waves {waves} {where}: |engine - shifted QP step| = {d:.2e}")
                np.testing.assert_allclose(out["x_pred"][i], want[0], atol=1e-10, rtol=0, err_msg=where)
                np.testing.assert_allclose(out["u_pred"][i], want[1], atol=1e-10, rtol=0, err_msg=where)
                # from the reference alone: carrying instead of shifting gives another iterate
                carried = wc.qp_step(orc, ur10_rb, ur10, c, prev["x_pred"][i], prev["u_pred"][i], x[i], y[i])
                shifted = wc.qp_step(orc, ur10_rb, ur10, c, Xs, Us, x[i], y[i])
                if carried is not None and shifted is not None:
                    apart.append(max(np.abs(carried[0] - shifted[0]).max(), np.abs(carried[1] - shifted[1]).max()))
                checked += 1
        prev = out
        x = np.stack([plants[i](x[i], out["u0"][i]) for i in range(len(cfgs))])
    assert checked == (steps - 1) * len(cfgs)
    print(f"N {N}: |QP step from the carried - from the shifted iterate| = {min(apart):.2e} .. {max(apart):.2e} over {len(apart)} steps")
    assert len(apart) >= checked // 2
    if N == 1:
        # One stage: x_0 is fixed to the feedback state and the cost rows that see u_0 are linear in it, so the QP does not depend on
        # the point it is linearised at and the two steps coincide (measured: 1e-16 .. 2e-16).  Nothing here can tell a shift from
        # a carry; N = 1 checks that the pass is legal there (nothing moves in u, x_1 is propagated again) and the step exact.
        assert max(apart) < 1e-12
    else:
        assert min(apart) > 1e-6


@pytest.mark.parametrize("solver,waves", [("SQP_RTI", 4), ("SQP_RTI", 1), ("SQP", 2)])
def test_modes_are_independent_in_one_batch(orc, ur10, solver, waves):
    """warm = [carry, reset, shift, carry, reset, shift] in one batch: every simulation equals, bit for bit, the same simulation in
    a batch where all take its mode -- a fresh controller's first step for the reset ones."""
    import emu_warm

    N, B = 20, 6
    so = {"nlp_solver_type": solver}
    cfgs = [_cfg(prediction_horizon=N, simulation_time=0.1, q_0=_q0(0.01 * i), solver_options=so) for i in range(B)]
    modes = np.array([wc.CARRY, wc.RESET, wc.SHIFT] * 2, dtype=np.int32)
    mixed, carry, shift = (emu_warm.Controller(cfgs, ur10, waves=waves) for _ in range(3))
    rng = np.random.default_rng(3)
    x = _x0(cfgs)
    for k in range(4):                                          # a common history: everyone carries
        y = np.stack([rc.ramp_reference(c, N, k0=k) for c in cfgs])
        for ctl in (mixed, carry, shift):
            out = ctl.step(x, yref=y, ref_changed=True, warm=[wc.CARRY] * B)
        x = x + rng.uniform(-2e-3, 2e-3, x.shape)
    y = np.stack([rc.ramp_reference(c, N, k0=4) for c in cfgs])
    om = mixed.step(x, yref=y, ref_changed=True, warm=modes)
    oc = carry.step(x, yref=y, ref_changed=True, warm=[wc.CARRY] * B)
    os_ = shift.step(x, yref=y, ref_changed=True, warm=[wc.SHIFT] * B)
    of = emu_warm.Controller(cfgs, ur10, waves=waves).step(x, yref=y, ref_changed=True)
    for i, (m, want) in enumerate(zip(modes, (oc, of, os_) * 2)):
        for key in om:
            if key != "solver_time":
                np.testing.assert_array_equal(om[key][i], want[key][i], err_msg=f"sim {i} mode {m} {key}")
    # (and the modes do differ)
    assert np.abs(oc["u_pred"] - os_["u_pred"]).max() > 1e-6 and np.abs(oc["u_pred"] - of["u_pred"]).max() > 1e-6
    # the step after: the reset simulations go on as the fresh controller does
    x2 = x + rng.uniform(-2e-3, 2e-3, x.shape)
    y2 = np.stack([rc.ramp_reference(c, N, k0=5) for c in cfgs])
    om2 = mixed.step(x2, yref=y2, ref_changed=True, warm=[wc.CARRY] * B)
    fresh = emu_warm.Controller(cfgs, ur10, waves=waves)
    fresh.step(x, yref=y, ref_changed=True)
    of2 = fresh.step(x2, yref=y2, ref_changed=True, warm=[wc.CARRY] * B)
    for i in (1, 4):
        for key in ("u0", "x_pred", "u_pred", "cost", "residuals", "status", "qp_iter"):
            np.testing.assert_array_equal(om2[key][i], of2[key][i], err_msg=f"sim {i} {key}")


def test_unknown_modes_carry_and_a_carry_array_is_the_plain_step(ur10):
    import emu_ref
    import emu_warm

    N = 20
    cfgs = [_cfg(prediction_horizon=N, simulation_time=0.06, q_0=_q0()), _cfg(prediction_horizon=N, simulation_time=0.06)]
    a, b = emu_ref.Controller(cfgs, ur10, waves=4), emu_warm.Controller(cfgs, ur10, waves=4)
    rng = np.random.default_rng(2)
    x = _x0(cfgs)
    for k in range(5):
        oa, ob = a.step(x), b.step(x, warm=[wc.CARRY, 7 if k % 2 else -1])
        for key in oa:
            np.testing.assert_array_equal(oa[key], ob[key], err_msg=key)
        x = x + rng.uniform(-1e-3, 1e-3, x.shape)


def test_no_modes_reproduce_the_reference_step_bit_for_bit(ur10):
    import emu_ref
    import emu_warm

    N = 20
    cfgs = [_cfg(prediction_horizon=N, simulation_time=0.06, q_0=_q0()), _cfg(prediction_horizon=N, simulation_time=0.06)]
    a, b = emu_ref.Controller(cfgs, ur10, waves=4), emu_warm.Controller(cfgs, ur10, waves=4)
    rng = np.random.default_rng(2)
    x = _x0(cfgs)
    for k in range(6):
        y = None if k < 2 else np.stack([rc.ramp_reference(c, N, k0=k) for c in cfgs])
        oa, ob = a.step(x, yref=y, ref_changed=k >= 2), b.step(x, yref=y, ref_changed=k >= 2, warm=None)
        for key in oa:
            np.testing.assert_array_equal(oa[key], ob[key], err_msg=key)
        x = x + rng.uniform(-1e-3, 1e-3, x.shape)


def test_shift_with_a_small_pool_moves_the_same_records(ur10):
    """The shift stages blocks of stages through the chunk pool: the smallest pool (several blocks per group) and the default one
    (one block) give the same step, at every number of wavefronts.  (Pool size and wavefronts also pick the solve sweeps, which
    sum in different orders: 1e-11, the bar the emulation tests hold against the oracle.)"""
    import emu_warm

    N = 30
    cfgs = [_cfg(prediction_horizon=N, simulation_time=0.05, q_0=_q0())]
    outs = []
    for pool, waves in ((0, 1), (2048, 1), (2048, 2), (2048, 4), (0, 8)):
        ctl = emu_warm.Controller(cfgs, ur10, pool_doubles=pool, waves=waves)
        x = _x0(cfgs)
        for k in range(3):
            o = ctl.step(x, yref=rc.ramp_reference(cfgs[0], N, k0=k)[None], ref_changed=True, warm=[wc.SHIFT])
            x = x + 1e-3
        outs.append((pool, waves, o))
    for pool, waves, o in outs[1:]:
        for key in ("x_pred", "u_pred", "u0"):
            np.testing.assert_allclose(o[key], outs[0][2][key], atol=1e-11, rtol=0, err_msg=f"pool {pool} waves {waves} {key}")


def test_full_sqp_from_a_shifted_start_converges_to_the_nlp(orc, ur10, ur10_rb):
    """Full SQP at a tight tolerance, second step shifted: status 0 at the NLP solution of the moved schedule (dense least squares
    over the inputs); the shifted multipliers and merit weights are only a start."""
    import emu_warm

    N = 12
    cfg = _cfg(prediction_horizon=N, simulation_time=0.05, q_0=_q0(),
               solver_options={"nlp_solver_type": "SQP", "nlp_solver_max_iter": 100, "nlp_solver_tol_stat": 1e-10,
                               "nlp_solver_tol_eq": 1e-10, "nlp_solver_tol_ineq": 1e-10, "nlp_solver_tol_comp": 1e-10})
    ctl = emu_warm.Controller([cfg], ur10, waves=2)
    x = _x0([cfg])
    kw = dict(px0=0.37, dpx=0.003, vy0=0.02, dvy=0.01)
    out = ctl.step(x, yref=rc.ramp_reference(cfg, N, **kw)[None], ref_changed=True)
    assert out["status"][0] == 0, out
    first_iters = out["sqp_iter"][0]
    x1 = orc.plant_step(0, np.asarray(cfg["wcv"]), cfg["dt"], x[0], out["u0"][0])[None]
    y1 = rc.ramp_reference(cfg, N, k0=1, **kw)[None]
    out = ctl.step(x1, yref=y1, ref_changed=True, warm=[wc.SHIFT])
    assert out["status"][0] == 0, out
    u = rc.dense_nlp_solve(orc, ur10_rb, cfg, x1[0], y1[0], out["u_pred"][0])
    np.testing.assert_allclose(out["u_pred"][0], u, atol=1e-6, rtol=0)
    # the bounds are inactive at this solution (the dense solve ignores them)
    assert (out["u_pred"][0] > np.asarray(cfg["umin"]) + 1e-3).all() and (out["u_pred"][0] < np.asarray(cfg["umax"]) - 1e-3).all()
    print(f"SQP iterations: first step {first_iters}, shifted second step {out['sqp_iter'][0]}")
