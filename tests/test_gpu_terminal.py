"""BatchController with a joint-wise terminal cost on the device (mpcb_step_term on both engines) against the dense KKT reference
of tests/dense_qp_terminal.py: reset steps at the default and at forced launch geometries, a ragged throughput-engine batch, the
zero terminal cost, a fixed point, chained steps (carried and shifted), active bounds and the interior-point cases.  Bounds: 10 x
the committed oracle-vs-dense distance of the case, floor 1e-12 (tests/test_terminal_cases.py ORACLE_VS_DENSE_TERM).

TERMINAL_DUMP=<file> collects the measured distances (tests/tools/terminal_profile.py)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import dense_qp as dq  # noqa: E402
import dense_qp_cases as dc  # noqa: E402
import dense_qp_terminal as dqt  # noqa: E402
import terminal_cases as tc  # noqa: E402
from test_boundaries import BOUNDARIES, PICKED_4_2, _named, force_geometry, geo_name  # noqa: E402
from test_gpu_dense_qp import GEOMETRY_HORIZONS  # noqa: E402
from test_terminal_cases import BY_ID, CASES, chained_tolerance, check_step, record  # noqa: E402

pytestmark = pytest.mark.gpu

# the cases of one horizon run as one batch (the fast path on and off, tight bounds: per-simulation parameters)
GROUPS = {}
for _c in CASES:
    GROUPS.setdefault(_c["N"], []).append(_c["id"])
# forced latency geometries: N = 20, both sides of the geometry's first sweep switch, N = 300 where test_gpu_dense_qp lists it
FORCED = {geo: (20, BOUNDARIES[geo]["sweep"][1][0] - 1, BOUNDARIES[geo]["sweep"][1][0]) + ((300,) if 300 in Ns else ())
          for geo, Ns in GEOMETRY_HORIZONS.items()}
RUNS = [(e, None, N) for e in ("stream", "latency") for N in sorted(GROUPS)] + \
       [("latency", geo, N) for geo in sorted(FORCED) for N in FORCED[geo]]
PICKED = [("latency", PICKED_4_2, 20)]      # beside the table that test_run_list_is_complete counts


def _run_id(r):
    return "%s%s-N%d" % (r[0], "" if r[1] is None else "-" + geo_name(r[1]), r[2])


def _clean(monkeypatch, geo=None):
    for k in ("MPCB_WAVES_PER_SIM", "MPCB_SIMS_PER_CU", "MPCB_ENGINE"):
        monkeypatch.delenv(k, raising=False)
    if geo is not None:
        force_geometry(monkeypatch, geo)


def controller(cases, engine, terminal=True):
    from robotic_mpc_amd import BatchController

    ctl = BatchController([c["raw"] for c in cases], engine=engine)
    if terminal:
        ctl.set_terminal_cost(np.stack([c["blocks"] for c in cases]), np.stack([c["x_e"] for c in cases]))
    return ctl


def numpy_step(ctl, x, **kw):
    return {k: v.cpu().numpy() for k, v in ctl.step(np.ascontiguousarray(x), **kw).items()}


def test_run_list_is_complete():
    assert sorted(c for ids in GROUPS.values() for c in ids) == sorted(BY_ID)
    assert sorted(FORCED) == sorted(BOUNDARIES) and len(RUNS) == 2 * len(GROUPS) + sum(len(v) for v in FORCED.values())
    for geo, Ns in FORCED.items():
        assert all(N in GROUPS for N in Ns), (geo, Ns)
        assert {_named(geo, N)[0] for N in Ns[1:3]} == {s for _, s in BOUNDARIES[geo]["sweep"][:2]}      # the two sides differ
    assert {BY_ID[c]["active"] for c in GROUPS[20]} == {False, True} and {BY_ID[c]["fast"] for c in GROUPS[20]} == {False, True}


@pytest.mark.parametrize("engine,geo,N", RUNS + PICKED, ids=[_run_id(r) for r in RUNS + PICKED])
def test_reset_step_against_dense(monkeypatch, engine, geo, N):
    _clean(monkeypatch, geo)
    cases = [BY_ID[c] for c in GROUPS[N]]
    ctl = controller(cases, engine)
    out = numpy_step(ctl, np.stack([c["xhat"] for c in cases]), predict=True)
    info = ctl.launch_info()
    ctl.close()
    assert info["engine"] == (1 if engine == "stream" else 0), info
    if geo is not None:
        assert info["waves_per_sim"] == geo[0] and info["pool_bytes"] == 8 * BOUNDARIES[geo[:2]]["pool"], info
    for i, c in enumerate(cases):
        check_step(c, out, i, "%s%s" % (engine, "" if geo is None else "-" + geo_name(geo)), rtol_cost=1e-9)


def test_ragged_batch_on_the_stream_engine():
    """Horizons {1, 7, 20, 80, 130} in one batch: the terminal cost acts at each simulation's own horizon end; NaN past it."""
    cases = [BY_ID["N%d-rand-term" % N] for N in (1, 7, 20, 80, 130)]
    ctl = controller(cases, "stream")
    out = numpy_step(ctl, np.stack([c["xhat"] for c in cases]), predict=True)
    assert ctl.launch_info()["engine"] == 1
    ctl.close()
    for i, c in enumerate(cases):
        assert np.isnan(out["x_pred"][i][c["N"] + 1:]).all() and np.isnan(out["u_pred"][i][c["N"]:]).all()
        check_step(c, out, i, "stream-ragged", rtol_cost=1e-9)


@pytest.mark.parametrize("N", [20, 130])
@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_zero_terminal_cost_is_no_terminal_cost(monkeypatch, engine, N):
    """set_terminal_cost(zeros, arbitrary x_ref) against no terminal cost, one reset step and two carried ones: equal bit for bit;
    and set_terminal_cost(None) after a non-zero one returns to the same values."""
    _clean(monkeypatch)
    c = BY_ID["N%d-rand-term" % N]
    keys = ("u0", "x_pred", "u_pred", "cost", "qp_iter")
    xs = [c["xhat"] + 1e-3 * k for k in range(3)]
    plain = controller([c], engine, terminal=False)
    want = [numpy_step(plain, x[None], predict=True) for x in xs]
    plain.close()
    zero = controller([c], engine, terminal=False)
    zero.set_terminal_cost(np.zeros((6, 3)), np.linspace(-3.0, 4.0, 12))
    for x, w in zip(xs, want):
        got = numpy_step(zero, x[None], predict=True)
        for k in keys:
            np.testing.assert_array_equal(got[k], w[k], err_msg=k)
    zero.close()
    back = controller([c], engine)
    moved = numpy_step(back, xs[0][None], predict=True)
    assert np.abs(moved["u0"] - want[0]["u0"]).max() > 1e-3            # the non-zero terminal cost was in force
    back.set_terminal_cost(None)
    assert back.terminal_cost() is None
    back.reset()
    for x, w in zip(xs, want):
        got = numpy_step(back, x[None], predict=True)
        for k in keys:
            np.testing.assert_array_equal(got[k], w[k], err_msg=k)
    back.close()


@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_fixed_point_is_stationary_for_the_terminal_problem(monkeypatch, engine):
    """N = 7, the feedback state held, 12 carried steps: the RTI iteration settles; then the stationarity residual is <= 1e-7 and
    the dense terminal QP assembled at the returned iterate has a step of <= 1e-6 -- while |P (x_N - x_e)| >= 1e-2 there, so a
    stage-N gradient without the terminal term would fail both."""
    _clean(monkeypatch)
    c = BY_ID["N7-rand-term"]
    ctl = controller([c], engine)
    for _ in range(12):
        out = numpy_step(ctl, c["xhat"][None], predict=True)
        assert out["status"][0] == 0
    ctl.close()
    X, U = out["x_pred"][0], out["u_pred"][0]
    assert np.abs(c["P"] @ (X[-1] - c["x_e"])).max() >= 1e-2
    print(f"\n[terminal] fixed point {engine}: residuals {out['residuals'][0]}")
    assert out["residuals"][0, 0] <= 1e-7
    sol = dq.solve_equality(dqt.assemble(dc.chain_of(c), c["cfg"], X, U, c["xhat"], c["P"], c["x_e"], c["yref"]))
    print(f"[terminal] fixed point {engine}: max |w| of the dense QP there = {np.abs(sol['w']).max():.2e}")
    assert np.abs(sol["w"]).max() <= 1e-6
    want = dqt.nlp_cost(dc.chain_of(c), c["cfg"], X, U, c["P"], c["x_e"], c["yref"])
    np.testing.assert_allclose(out["cost"][0], want, rtol=1e-9, atol=0)


@pytest.mark.parametrize("shift", [False, True], ids=["carry", "shift"])
@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_three_chained_steps_against_dense(monkeypatch, engine, shift):
    _clean(monkeypatch)
    case = BY_ID[tc.CHAINED_CASE]
    ctl = controller([case], engine)

    def step(x, sh):
        out = numpy_step(ctl, x[None], predict=True, shift=bool(sh))
        assert out["status"][0] == 0
        return out["x_pred"][0], out["u_pred"][0]

    d, _ = tc.chained(case, step, shift=shift)
    ctl.close()
    print(f"\n[terminal] chained {'shift' if shift else 'carry'} {engine}: |device - dense| = {d}")
    for k, v in enumerate(d):
        record("chained-%s-step%d" % ("shift" if shift else "carry", k), engine, v)
        assert v <= chained_tolerance(shift, k), (k, v)


def test_terminal_cost_getter_and_persistence_across_reset(monkeypatch):
    _clean(monkeypatch)
    c = BY_ID["N20-rand-term"]
    ctl = controller([c], "latency")
    t = ctl.terminal_cost()
    np.testing.assert_array_equal(t["blocks"].cpu().numpy()[0], c["blocks"])
    np.testing.assert_array_equal(t["x_ref"].cpu().numpy()[0], c["x_e"])
    a = numpy_step(ctl, c["xhat"][None], predict=True)
    ctl.reset()
    b = numpy_step(ctl, c["xhat"][None], predict=True)
    for k in ("u0", "x_pred", "u_pred", "cost"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    with pytest.raises(ValueError):
        ctl.step(c["xhat"][None], sens_w=True)
    ctl.close()


def test_the_c_entry_refuses_what_the_header_says(monkeypatch):
    """MPCB_ESTATE on a handle that is no controller; MPCB_EINVAL for a terminal cost on a full-SQP controller and for du0_dxe
    without sens or without term."""
    import ctypes as C

    import torch

    from robotic_mpc_amd import BatchController, base_params, engine

    _clean(monkeypatch)
    lib = engine.load_library()
    h = C.c_void_p()
    assert lib.mpcb_create(C.byref(h), 0) == 0
    t = torch.zeros((1, 30), dtype=torch.float64, device="cuda")
    tp = C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_double))
    assert lib.mpcb_step_term(h, None, None, 0, None, 0, None, tp, 1, None, None) == -5          # MPCB_ESTATE
    lib.mpcb_destroy(h)
    x = np.zeros((1, 12))
    sqp = BatchController([base_params(prediction_horizon=5, solver_options={"nlp_solver_type": "SQP"})])
    io = dict(sqp._buffers(False), xhat=sqp._xhat(x))
    with pytest.raises(engine.EngineError, match="full SQP"):
        sqp.engine.step_sens(io, term=t, term_changed=True)
    sqp.close()
    rti = BatchController([base_params(prediction_horizon=5, solver_options={"nlp_solver_type": "SQP_RTI"})])
    io = dict(rti._buffers(False), xhat=rti._xhat(x))
    dxe = torch.zeros((1, 6, 12), dtype=torch.float64, device="cuda")
    with pytest.raises(engine.EngineError, match="du0_dxe"):
        rti.engine.step_sens(io, term=t, du0_dxe=dxe)                                            # no sens
    sens = dict(du0_dx=torch.zeros((1, 6, 12), dtype=torch.float64, device="cuda"), valid=torch.zeros(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(engine.EngineError, match="du0_dxe"):
        rti.engine.step_sens(io, sens=sens, du0_dxe=dxe)                                         # no term
    rti.close()
