"""The controller step with a per-simulation warm start on the GPU (mpcb_step_warm, BatchController.step(shift=...) / reset(mask)), on
both kernel families: a shifted RTI step against the exact Gauss-Newton QP step from the previous prediction shifted in numpy, the
three modes in one launch, a ragged batch that shifts every second simulation, reset(mask) on a side stream, the two engines
against each other on a large shifted tracking batch, and the refusal of a handle that is no controller."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reference_checks as rc  # noqa: E402
import warm_checks as wc  # noqa: E402

pytestmark = pytest.mark.gpu

# qp_tol 1e-14 / 200 iterations: the reasoning of test_gpu_controller_reference.py
TIGHT_QP = {"qp_tol": 1e-14, "qp_solver_iter_max": 200}


def _raw(B, N, steps, seed=0, solver="SQP_RTI", so=None, **kw):
    from robotic_mpc_amd import config

    rng = np.random.default_rng(seed)
    Ns = N if isinstance(N, (list, tuple)) else [N] * B
    return [config.base_params(prediction_horizon=int(Ns[i]), simulation_time=0.01 * steps,
                               q_0=config.BASE_PARAMS["q_0"] + rng.uniform(-0.1, 0.1, 6),
                               solver_options=dict({"nlp_solver_type": solver}, **(so or {})), **kw)
            for i in range(B)]


def _resolve(raw):
    from robotic_mpc_amd import config

    return [config.resolve_config(r) for r in raw]


def _plant(orc, cfgs, x, u, rng):
    wcv = np.stack([c["wcv"] for c in cfgs]) * 0.8
    xn = np.stack([orc.plant_step(0, wcv[i], cfgs[i]["dt"], x[i], u[i]) for i in range(len(cfgs))])
    return xn + rng.uniform(-1e-3, 1e-3, x.shape)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _x0(cfgs):
    return np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])


def _schedule(cfgs, N, k):
    """The sliding schedule: row j of step k is stage k + j of one ramp."""
    return np.stack([rc.ramp_reference(c, N, k0=k) for c in cfgs])


@pytest.mark.parametrize("engine", ["latency", "stream"])
@pytest.mark.parametrize("N,B,waves", [(1, 8, None), (2, 8, None), (20, 8, None), (100, 8, 8), (40, 6, 4), (12, 3, 2), (12, 3, 1)])
def test_shifted_rti_step_is_the_exact_qp_step_from_the_shifted_iterate(orc, ur10_rb, monkeypatch, engine, N, B, waves):
    from robotic_mpc_amd import BatchController, robots

    if waves is not None and waves < 4:      # <2> and <1>: mpcb_setup never picks them by itself
        monkeypatch.setenv("MPCB_WAVES_PER_SIM", str(waves))
    steps = 12
    raw = _raw(B, N, steps, seed=4, so=TIGHT_QP)
    cfgs = _resolve(raw)
    ctl = BatchController(raw, engine=engine)
    if engine == "latency" and waves is not None:
        assert ctl.launch_info()["waves_per_sim"] == waves
    ur10 = robots.builtin_chain("ur10")
    rng = np.random.default_rng(5)
    x = _x0(cfgs)
    prev, checked, apart = None, 0, []
    for k in range(steps):
        y = _schedule(cfgs, N, k)
        out = _np(ctl.step(x, predict=True, yref=y, shift=True))
        assert np.isfinite(out["u0"]).all() and (out["status"] == 0).all()
        if prev is not None:
            for i, c in enumerate(cfgs):
                where = f"step {k} sim {i}"
                Xs, Us = wc.shift_iterate(orc, c, prev["x_pred"][i], prev["u_pred"][i])
                want = wc.qp_step(orc, ur10_rb, ur10, c, Xs, Us, x[i], y[i], (out["x_pred"][i], out["u_pred"][i], out["qp_iter"][i]))
                assert want is not None, where
                d = max(np.abs(out["x_pred"][i] - want[0]).max(), np.abs(out["u_pred"][i] - want[1]).max())
                print(f"{engine} N {N} {where}: |engine - shifted QP step| = {d:.2e} (qp_iter {out['qp_iter'][i]})")
                np.testing.assert_allclose(out["x_pred"][i], want[0], atol=1e-10, rtol=0, err_msg=where)
                np.testing.assert_allclose(out["u_pred"][i], want[1], atol=1e-10, rtol=0, err_msg=where)
                checked += 1
                # from the reference alone: carrying instead of shifting gives another iterate (two simulations carry the check)
                if i < 2:
                    carried = wc.qp_step(orc, ur10_rb, ur10, c, prev["x_pred"][i], prev["u_pred"][i], x[i], y[i])
                    shifted = want if out["qp_iter"][i] == 1 else wc.qp_step(orc, ur10_rb, ur10, c, Xs, Us, x[i], y[i])
                    if carried is not None and shifted is not None:
                        apart.append(max(np.abs(carried[0] - shifted[0]).max(), np.abs(carried[1] - shifted[1]).max()))
        prev = out
        x = _plant(orc, cfgs, x, out["u0"], rng)
    assert checked == (steps - 1) * B
    print(f"{engine} N {N}: |QP step from the carried - from the shifted iterate| = {min(apart):.2e} .. {max(apart):.2e} ({len(apart)})")
    assert len(apart) >= steps - 1
    if N == 1:
        assert max(apart) < 1e-12      # one stage: the QP does not depend on where it is linearised (test_emulation_warm.py)
    else:
        assert min(apart) > 1e-6


@pytest.mark.parametrize("engine", ["latency", "stream"])
@pytest.mark.parametrize("solver", ["SQP_RTI", "SQP"])
def test_mixed_modes_in_one_launch(orc, engine, solver):
    """warm = [carry, reset, shift, carry, reset, shift]: every simulation equals, bit for bit, the same simulation of a controller
    where all take its mode -- a fresh controller's first step for the reset ones."""
    import torch

    from robotic_mpc_amd import BatchController

    N, B = 40, 6
    raw = _raw(B, N, 10, seed=21, solver=solver)
    cfgs = _resolve(raw)
    mixed, carry, shift, fresh = (BatchController(raw, engine=engine) for _ in range(4))
    rng = np.random.default_rng(22)
    x = _x0(cfgs)
    for k in range(4):
        y = _schedule(cfgs, N, k)
        for ctl in (mixed, carry, shift):
            ctl.step(x, yref=y)
        x = x + rng.uniform(-2e-3, 2e-3, x.shape)
    y = _schedule(cfgs, N, 4)
    resets = np.array([False, True, False] * 2)
    shifts = torch.tensor([False, False, True] * 2, device="cuda")
    mixed.reset(resets)
    om = _np(mixed.step(x, predict=True, yref=y, shift=shifts))
    oc = _np(carry.step(x, predict=True, yref=y))
    os_ = _np(shift.step(x, predict=True, yref=y, shift=True))
    of = _np(fresh.step(x, predict=True, yref=y))
    for i, want in enumerate((oc, of, os_) * 2):
        for key in ("u0", "x_pred", "u_pred", "cost", "residuals", "status", "sqp_iter", "qp_iter"):
            np.testing.assert_array_equal(om[key][i], want[key][i], err_msg=f"sim {i} {key}")
    assert np.abs(oc["u_pred"] - os_["u_pred"]).max() > 1e-6 and np.abs(oc["u_pred"] - of["u_pred"]).max() > 1e-6
    # the masks were for that step alone
    x2, y2 = x + rng.uniform(-2e-3, 2e-3, x.shape), _schedule(cfgs, N, 5)
    om2, of2 = _np(mixed.step(x2, predict=True, yref=y2)), _np(fresh.step(x2, predict=True, yref=y2))
    for i in (1, 4):
        np.testing.assert_array_equal(om2["u_pred"][i], of2["u_pred"][i], err_msg=f"sim {i}")


def test_ragged_batch_shifts_every_second_simulation(orc, ur10_rb):
    from robotic_mpc_amd import BatchController, robots

    horizons = list(range(1, 61))
    raw = _raw(60, horizons, 8, seed=6, so=TIGHT_QP)
    cfgs = _resolve(raw)
    ctl, carry = BatchController(raw, engine="stream"), BatchController(raw, engine="stream")
    ur10 = robots.builtin_chain("ur10")
    N, B = ctl.N, len(raw)
    rng = np.random.default_rng(7)
    x = _x0(cfgs)
    past = np.arange(N)[None, :] >= np.array(horizons)[:, None]
    mask = np.arange(B) % 2 == 1
    prev, checked = None, 0
    for k in range(8):
        y = _schedule(cfgs, N, k)
        y[past] = np.nan
        out = _np(ctl.step(x, predict=True, yref=y, shift=mask))
        ref = _np(carry.step(x, predict=True, yref=y))
        assert np.isfinite(out["u0"]).all() and np.isfinite(out["cost"]).all() and np.isfinite(out["residuals"]).all()
        for i, c in enumerate(cfgs):
            Ni, where = horizons[i], f"step {k} sim {i}"
            assert np.isfinite(out["u_pred"][i][:Ni]).all() and np.isnan(out["u_pred"][i][Ni:]).all(), where
            assert np.isfinite(out["x_pred"][i][:Ni + 1]).all() and np.isnan(out["x_pred"][i][Ni + 1:]).all(), where
            if not mask[i]:
                continue
            if prev is not None and out["qp_iter"][i] == 1:
                Xs, Us = wc.shift_iterate(orc, c, prev["x_pred"][i][:Ni + 1], prev["u_pred"][i][:Ni])
                want = rc.gn_qp_step(orc, ur10_rb, c, Xs, Us, x[i], y[i][:Ni])
                assert want is not None, where
                np.testing.assert_allclose(out["x_pred"][i][:Ni + 1], want[0], atol=1e-10, rtol=0, err_msg=where)
                np.testing.assert_allclose(out["u_pred"][i][:Ni], want[1], atol=1e-10, rtol=0, err_msg=where)
                checked += 1
        # the simulations that carry: what they are in a controller where everyone carries (their history has no shift in it)
        for key in ("u0", "x_pred", "u_pred", "cost", "residuals", "status", "qp_iter"):
            np.testing.assert_array_equal(out[key][~mask], ref[key][~mask], err_msg=f"step {k} {key}")
        prev = out
        x = _plant(orc, cfgs, x, out["u0"], rng)
    assert checked >= 7 * 30 // 2, checked


def test_reset_mask_on_a_side_stream_keeps_the_others_and_the_reference():
    import torch

    from robotic_mpc_amd import BatchController

    raw = _raw(8, 40, 6, seed=14)
    cfgs = _resolve(raw)
    x0 = torch.tensor(_x0(cfgs), device="cuda")
    x1 = x0 + 1e-3
    y = np.tile(np.array([0.0, 1.0, 0.0, 0.33, 0.02]), (8, 1))
    mask = torch.tensor([True, False, False, True, False, False, False, True], device="cuda")
    for engine in ("latency", "stream"):
        ctl, other, fresh = (BatchController(raw, engine=engine) for _ in range(3))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        ctl.set_reference(y)
        other.set_reference(y)
        with torch.cuda.stream(side):
            for _ in range(3):
                ctl.step(x0)
            ctl.reset(np.zeros(8, dtype=bool))                 # an empty mask first: masks accumulate
            ctl.reset(mask)
            a = {k: v.clone() for k, v in ctl.step(x1, predict=True).items()}
        side.synchronize()
        for _ in range(3):
            other.step(x0)
        b = other.step(x1, predict=True)                        # nobody reset
        f = fresh.step(x1, predict=True, yref=y)                # everybody fresh, same reference
        m = mask.cpu().numpy()
        for key in ("u0", "x_pred", "u_pred", "cost"):
            assert torch.equal(a[key][mask], f[key][mask]), (engine, key)
            assert torch.equal(a[key][~mask], b[key][~mask]), (engine, key)
        assert not torch.equal(a["u0"][mask], b["u0"][mask])
        plain = BatchController(raw, engine=engine).step(x1)    # (the packed reference gives another input: the set one was kept)
        assert not torch.equal(a["u0"][mask], plain["u0"][mask]), m


def test_engines_agree_on_a_large_shifted_tracking_batch(orc):
    from robotic_mpc_amd import BatchController

    raw = _raw(1280, 100, 12, seed=10)
    cfgs = _resolve(raw)
    lat, stm = BatchController(raw, engine="latency"), BatchController(raw, engine="stream")
    rng = np.random.default_rng(12)
    x = _x0(cfgs)
    for k in range(12):
        y = _schedule(cfgs, 100, k)
        a, b = _np(lat.step(x, yref=y, shift=True)), _np(stm.step(x, yref=y, shift=True))
        print(f"step {k}: max |u0 stream - latency| = {np.abs(b['u0'] - a['u0']).max():.2e}")
        np.testing.assert_allclose(b["u0"], a["u0"], atol=1e-9, rtol=0, err_msg=f"step {k}")
        np.testing.assert_array_equal(b["status"], a["status"])
        x = _plant(orc, cfgs, x, a["u0"], rng)


def test_step_warm_refuses_a_handle_that_is_no_controller(ur10):
    """MPCB_ESTATE, as mpcb_step gives such a handle, and nothing is launched."""
    import torch

    from robotic_mpc_amd import engine

    cfgs = _resolve(_raw(2, 10, 5))
    eng = engine.MpcBatchEngine(0)
    eng.setup(cfgs, ur10)                                       # a rollout handle
    io = engine.MpcbStepIO()
    warm = torch.zeros(2, dtype=torch.int32, device="cuda")
    wp = C.cast(C.c_void_p(warm.data_ptr()), C.POINTER(C.c_int))
    rc_warm = eng.lib.mpcb_step_warm(eng._h, C.byref(io), None, 0, wp, 0, None)
    rc_plain = eng.lib.mpcb_step(eng._h, C.byref(io), 0, None)
    assert rc_warm == rc_plain == -5                           # MPCB_ESTATE
    assert b"mpcb_setup_controller" in eng.lib.mpcb_last_error(eng._h)
    eng.close()
