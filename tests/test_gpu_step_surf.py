"""BatchController over a scheduled, stage-varying surface on the device (mpcb_step_surf on both engines) against the dense KKT
reference with per-stage coefficients (tests/dense_qp_surf.py): the run list of tests/test_gpu_step_dist.py -- reset steps at the
default and at forced launch geometries, a ragged throughput-engine batch -- three chained steps (carried and shifted, the window
sliding one row per step), the constant window against the plain step relinearised, the f-shift equivalence against mpcb_step_ref on
the same engine, and what the C entry refuses.  Bounds: 10 x the committed oracle-vs-dense distance of the case, floor 1e-12
(tests/step_surf_cases.py ORACLE_VS_DENSE_SURF)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import dense_qp as dq  # noqa: E402
import step_surf_cases as ss  # noqa: E402
import test_gpu_step_dist as gd  # noqa: E402  (its run list, geometry forcing and helpers)
from test_boundaries import BOUNDARIES, geo_name  # noqa: E402
from test_step_dist_cases import chained_tolerance  # noqa: E402

pytestmark = pytest.mark.gpu

BY_ID = ss.by_id()
GROUPS, RUNS = gd.GROUPS, gd.RUNS


def controller(cases, engine, surf=True):
    from robotic_mpc_amd import BatchController

    ctl = BatchController([c["raw"] for c in cases], engine=engine)
    if surf:
        N = max(c["N"] for c in cases)
        w = np.zeros((len(cases), N, 6))
        for i, c in enumerate(cases):
            w[i, :c["N"]] = c["surf"]
            w[i, c["N"]:] = 1e3               # rows past a simulation's own horizon are never read: a surface nothing could track
        ctl.set_surface(w)
    return ctl


def test_run_list_is_the_disturbance_tests():
    assert sorted(c for ids in GROUPS.values() for c in ids) == sorted(BY_ID) and len(RUNS) == 2 * len(GROUPS) + 3 * len(gd.FORCED)


@pytest.mark.parametrize("engine,geo,N", RUNS, ids=[gd._run_id(r) for r in RUNS])
def test_reset_step_against_dense(monkeypatch, engine, geo, N):
    """1. The reset step minus the initial guess solves the QP on the window; cost is dense_qp_surf.nlp_cost at the returned iterate
    (rtol 1e-9); the getter returns what was set."""
    gd._clean(monkeypatch, geo)
    cases = [BY_ID[c] for c in GROUPS[N]]
    ctl = controller(cases, engine)
    np.testing.assert_array_equal(ctl.surface().cpu().numpy(), np.stack([c["surf"] for c in cases]))
    out = gd.numpy_step(ctl, np.stack([c["xhat"] for c in cases]), predict=True)
    info = ctl.launch_info()
    ctl.close()
    assert info["engine"] == (1 if engine == "stream" else 0), info
    if geo is not None:
        assert info["waves_per_sim"] == geo[0] and info["pool_bytes"] == 8 * BOUNDARIES[geo[:2]]["pool"], info
    for i, c in enumerate(cases):
        ss.check_step(c, out, i, "%s%s" % (engine, "" if geo is None else "-" + geo_name(geo)), rtol_cost=1e-9)


def test_ragged_batch_on_the_stream_engine():
    """2. Horizons {1, 7, 20, 80, 130} in one batch, a window per simulation strided by the longest horizon (absurd rows past each
    simulation's own: never read); NaN past each horizon in the prediction."""
    cases = [BY_ID["N%d-rand-dist" % N] for N in (1, 7, 20, 80, 130)]
    ctl = controller(cases, "stream")
    out = gd.numpy_step(ctl, np.stack([c["xhat"] for c in cases]), predict=True)
    assert ctl.launch_info()["engine"] == 1
    ctl.close()
    for i, c in enumerate(cases):
        assert np.isnan(out["x_pred"][i][c["N"] + 1:]).all() and np.isnan(out["u_pred"][i][c["N"]:]).all()
        ss.check_step(c, out, i, "stream-ragged", rtol_cost=1e-9)


@pytest.mark.parametrize("shift", [False, True], ids=["carry", "shift"])
@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_three_chained_steps_against_dense(monkeypatch, engine, shift):
    """3. Carried and shifted, the window sliding one row per step, each step certified against the dense QP at the iterate it
    started from on that step's window."""
    gd._clean(monkeypatch)
    case = BY_ID[ss.CHAINED_CASE]
    ctl = controller([case], engine, surf=False)

    def step(x, sh, w):
        out = gd.numpy_step(ctl, x[None], predict=True, shift=bool(sh), surface=w[None])
        assert out["status"][0] == 0
        return out["x_pred"][0], out["u_pred"][0]

    d = ss.chained(case, step, shift=shift)
    ctl.close()
    print(f"\n[surf] chained {'shift' if shift else 'carry'} {engine}: |device - dense| = {d}")
    for k, v in enumerate(d):
        assert v <= chained_tolerance(shift, k), (k, v)


@pytest.mark.parametrize("N", [20, 130])
@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_constant_window_is_the_plain_step_relinearised(monkeypatch, engine, N):
    """4. The packed coefficients on every row through the new kernels, set again every step, against the plain controller given
    yref = the packed row every step, so that both linearise again: one reset step and two carried ones; u0, x_pred, u_pred, cost
    at rtol 1e-12, qp_iter equal."""
    gd._clean(monkeypatch)
    c = BY_ID["N%d-rand-dist" % N]
    xs = [c["xhat"] + 1e-3 * k for k in range(3)]
    plain = controller([c], engine, surf=False)
    yref = plain.default_reference().cpu().numpy()
    want = [gd.numpy_step(plain, x[None], predict=True, yref=yref) for x in xs]
    plain.close()
    const = controller([c], engine, surf=False)
    worst = 0.0
    for x, w in zip(xs, want):
        got = gd.numpy_step(const, x[None], predict=True, surface=np.tile(c["cfg"]["coeffs"], (1, N, 1)))
        np.testing.assert_array_equal(got["qp_iter"], w["qp_iter"])
        for k in ("u0", "x_pred", "u_pred", "cost"):
            worst = max(worst, float(np.abs(got[k] - w[k]).max() / np.abs(w[k]).max()))
            np.testing.assert_allclose(got[k], w[k], rtol=1e-12, atol=1e-12 * np.abs(w[k]).max(), err_msg=k)
    const.close()
    print(f"\n[surf] constant window {engine} N{N}: worst relative difference {worst:.1e}")


@pytest.mark.parametrize("N", [20, 130])
@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_f_shift_equivalence(monkeypatch, engine, N):
    """5. f enters g1 alone: a window that varies only in f against mpcb_step_ref on the packed surface with yref[..., 0] lowered by
    the same amounts, on the same engine; a different shift every step; rtol 1e-12, qp_iter equal."""
    gd._clean(monkeypatch)
    c = BY_ID["N%d-rand-dist" % N]
    cfg = c["cfg"]
    a, b = controller([c], engine, surf=False), controller([c], engine, surf=False)
    worst = 0.0
    for k in range(3):
        x = (c["xhat"] + 1e-3 * k)[None]
        df = 0.01 * np.sin(0.3 * (np.arange(N) + k) + 0.5)
        surf = np.tile(cfg["coeffs"], (N, 1))
        surf[:, 5] += df
        yref = np.tile(dq.packed_reference(cfg), (N, 1))
        yref[:, 0] -= df
        ga = gd.numpy_step(a, x, predict=True, surface=surf[None])
        gb = gd.numpy_step(b, x, predict=True, yref=yref[None])
        assert ga["status"][0] == 0
        np.testing.assert_array_equal(ga["qp_iter"], gb["qp_iter"])
        for key in ("u0", "x_pred", "u_pred", "cost"):
            worst = max(worst, float(np.abs(ga[key] - gb[key]).max() / np.abs(gb[key]).max()))
            np.testing.assert_allclose(ga[key], gb[key], rtol=1e-12, atol=1e-12 * np.abs(gb[key]).max(), err_msg=key)
    a.close()
    b.close()
    print(f"\n[surf] f-shift {engine} N{N}: worst relative difference {worst:.1e}")


def test_the_c_entry_and_the_controller_refuse_what_the_header_says(monkeypatch):
    """6. MPCB_ESTATE on a handle that is no controller; MPCB_EINVAL for a window on a full-SQP controller; the controller's
    ValueErrors for the combinations that are not offered."""
    import ctypes as C

    import torch

    from robotic_mpc_amd import BatchController, base_params, engine

    gd._clean(monkeypatch)
    lib = engine.load_library()
    h = C.c_void_p()
    assert lib.mpcb_create(C.byref(h), 0) == 0
    t = torch.zeros((1, 5, 6), dtype=torch.float64, device="cuda")
    tp = C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_double))
    assert lib.mpcb_step_surf(h, None, None, 0, None, 0, tp, 1, None) == -5          # MPCB_ESTATE
    lib.mpcb_destroy(h)
    x = np.zeros((1, 12))
    sqp = BatchController([base_params(prediction_horizon=5, solver_options={"nlp_solver_type": "SQP"})])
    io = dict(sqp._buffers(False), xhat=sqp._xhat(x))
    with pytest.raises(engine.EngineError, match="full SQP"):
        sqp.engine.step_surf(io, surf=t, surf_changed=True)
    with pytest.raises(ValueError, match="SQP_RTI"):
        sqp.set_surface(np.zeros((5, 6)))
    sqp.close()
    rti = BatchController([base_params(prediction_horizon=5, solver_options={"nlp_solver_type": "SQP_RTI"})])
    with pytest.raises(ValueError, match="shape"):
        rti.set_surface(np.zeros((4, 6)))
    rti.set_surface(np.tile(rti.configs[0]["coeffs"], (5, 1)))
    with pytest.raises(ValueError, match="surface window"):
        rti.step(x, sens=True)
    with pytest.raises(ValueError, match="surface window"):
        rti.set_input_disturbance(np.zeros(6))
    with pytest.raises(ValueError, match="surface window"):
        rti.set_terminal_cost(np.zeros((6, 3)), np.zeros(12))
    rti.set_surface(None)
    assert rti.surface() is None
    rti.set_input_disturbance(np.zeros(6))
    with pytest.raises(ValueError, match="input disturbance"):
        rti.set_surface(np.zeros((5, 6)))
    rti.close()
