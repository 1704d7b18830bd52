"""BatchController(combined=True) on the device (mpcb_step_combined on both engines): terminal cost, input disturbance, surface window
and shift in one step, against the dense KKT reference that composes the three assemblies (tests/dense_qp_combined.py).  The run list
of tests/test_gpu_step_dist.py -- reset steps at the default and at every forced launch geometry of test_boundaries.BOUNDARIES, a
ragged throughput-engine batch -- three chained steps (carried and shifted, each with a new d, window and x_e), and neutrality
against mpcb_step_term / _dist / _surf / _warm on the device (rtol 1e-12, qp_iter equal).  Bounds: 10 x the committed
oracle-vs-dense distance of the case, floor 1e-12 (tests/step_combined_cases.py ORACLE_VS_DENSE_COMBINED)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import step_combined_cases as sc  # noqa: E402
import test_gpu_step_dist as gd  # noqa: E402  (its run list, geometry forcing and helpers)
from test_boundaries import BOUNDARIES, geo_name  # noqa: E402
from test_emulation_step_combined import chained_tolerance  # noqa: E402

pytestmark = pytest.mark.gpu

BY_ID = sc.by_id()
RUNS = gd.RUNS
GROUPS = {N: [c.replace("-dist", "-comb") for c in ids] for N, ids in gd.GROUPS.items()}


def controller(cases, engine, combined=True, live=("term", "dist", "surf")):
    from robotic_mpc_amd import BatchController

    ctl = BatchController([c["raw"] for c in cases], engine=engine, combined=combined)
    N = max(c["N"] for c in cases)
    if "surf" in live:
        w = np.zeros((len(cases), N, 6))
        for i, c in enumerate(cases):
            w[i, :c["N"]] = c["surf"]
            w[i, c["N"]:] = 1e3               # rows past a simulation's own horizon are never read
        ctl.set_surface(w)
    if "dist" in live:
        ctl.set_input_disturbance(np.stack([c["d"] for c in cases]))
    if "term" in live:
        ctl.set_terminal_cost(np.stack([c["blocks"] for c in cases]), np.stack([c["x_e"] for c in cases]))
    return ctl


def test_run_list_is_the_disturbance_tests():
    assert sorted(c for ids in GROUPS.values() for c in ids) == sorted(BY_ID)


@pytest.mark.parametrize("engine,geo,N", RUNS, ids=[gd._run_id(r) for r in RUNS])
def test_reset_step_against_dense(monkeypatch, engine, geo, N):
    gd._clean(monkeypatch, geo)
    cases = [BY_ID[c] for c in GROUPS[N]]
    ctl = controller(cases, engine)
    out = gd.numpy_step(ctl, np.stack([c["xhat"] for c in cases]), predict=True)
    info = ctl.launch_info()
    ctl.close()
    assert info["engine"] == (1 if engine == "stream" else 0), info
    if geo is not None:
        assert info["waves_per_sim"] == geo[0] and info["pool_bytes"] == 8 * BOUNDARIES[geo[:2]]["pool"], info
    for i, c in enumerate(cases):
        sc.check_step(c, out, i, "%s%s" % (engine, "" if geo is None else "-" + geo_name(geo)), rtol_cost=1e-9)


def test_ragged_batch_on_the_stream_engine():
    """Horizons {1, 7, 20, 80, 130} in one batch: the terminal cost on each simulation's own last stage, a window per simulation
    strided by the longest horizon; NaN past each horizon in the prediction."""
    cases = [BY_ID["N%d-rand-comb" % N] for N in (1, 7, 20, 80, 130)]
    ctl = controller(cases, "stream")
    out = gd.numpy_step(ctl, np.stack([c["xhat"] for c in cases]), predict=True)
    assert ctl.launch_info()["engine"] == 1
    ctl.close()
    for i, c in enumerate(cases):
        assert np.isnan(out["x_pred"][i][c["N"] + 1:]).all() and np.isnan(out["u_pred"][i][c["N"]:]).all()
        sc.check_step(c, out, i, "stream-ragged", rtol_cost=1e-9)


@pytest.mark.parametrize("shift", [False, True], ids=["carry", "shift"])
@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_three_chained_steps_against_dense(monkeypatch, engine, shift):
    gd._clean(monkeypatch)
    case = BY_ID[sc.CHAINED_CASE]
    ctl = controller([case], engine, live=())

    def step(x, sh, w, d, xe):
        ctl.set_terminal_cost(case["blocks"], xe)
        out = gd.numpy_step(ctl, x[None], predict=True, shift=bool(sh), surface=w[None], dist=d[None])
        assert out["status"][0] == 0
        return out["x_pred"][0], out["u_pred"][0]

    d, _ = sc.chained(case, step, shift=shift)
    ctl.close()
    print(f"\n[combined] chained {'shift' if shift else 'carry'} {engine}: |device - dense| = {d}")
    for k, v in enumerate(d):
        assert v <= chained_tolerance(shift, k), (k, v)


@pytest.mark.parametrize("feature", ["term", "dist", "surf", "shift"])
@pytest.mark.parametrize("engine,N", [("latency", 20), ("latency", 130), ("stream", 20)])
def test_one_live_feature_is_the_single_feature_step(monkeypatch, engine, N, feature):
    """The combined kernels with the other features neutral (the library's tables) against the single-feature kernels: a reset step
    and two more (shifted where the feature is the shift), everything set again every step so that both sides linearise again."""
    gd._clean(monkeypatch)
    c = BY_ID["N%d-rand-comb" % N]
    xs = [c["xhat"] + 1e-3 * k for k in range(3)]
    live = () if feature == "shift" else (feature,)
    one, comb = controller([c], engine, combined=False, live=()), controller([c], engine, live=())
    yref = one.default_reference().cpu().numpy()
    worst = 0.0
    for k, x in enumerate(xs):
        res = []
        for ctl in (one, comb):
            kw = {}
            if "term" in live:
                ctl.set_terminal_cost(c["blocks"], c["x_e"])
            if "dist" in live:
                kw["dist"] = c["d"][None]
            if "surf" in live:
                kw["surface"] = c["surf"][None]
            res.append(gd.numpy_step(ctl, x[None], predict=True, yref=yref, shift=(feature == "shift" and k > 0), **kw))
        w, g = res
        assert w["status"][0] == 0
        np.testing.assert_array_equal(g["qp_iter"], w["qp_iter"])
        for key in ("u0", "x_pred", "u_pred", "cost"):
            worst = max(worst, float(np.abs(g[key] - w[key]).max() / np.abs(w[key]).max()))
            np.testing.assert_allclose(g[key], w[key], rtol=1e-12, atol=1e-12 * np.abs(w[key]).max(), err_msg=key)
    one.close()
    comb.close()
    print(f"\n[combined] neutrality {feature} {engine} N{N}: worst relative difference {worst:.1e}")


def test_refusals(monkeypatch):
    import ctypes as C

    from robotic_mpc_amd import BatchController, base_params, engine

    gd._clean(monkeypatch)
    lib = engine.load_library()
    h = C.c_void_p()
    assert lib.mpcb_create(C.byref(h), 0) == 0
    assert lib.mpcb_step_combined(h, None, None, 0, None, 0, None, 0, None, 0, None, 0, None) == -5      # MPCB_ESTATE
    lib.mpcb_destroy(h)
    with pytest.raises(ValueError, match="SQP_RTI"):
        BatchController([base_params(prediction_horizon=5, solver_options={"nlp_solver_type": "SQP"})], combined=True)
    sqp = BatchController([base_params(prediction_horizon=5, solver_options={"nlp_solver_type": "SQP"})])
    io = dict(sqp._buffers(False), xhat=sqp._xhat(np.zeros((1, 12))))
    with pytest.raises(engine.EngineError, match="full SQP"):
        sqp.engine.step_combined(io)
    sqp.close()
    rti = BatchController([base_params(prediction_horizon=5, solver_options={"nlp_solver_type": "SQP_RTI"})], combined=True)
    with pytest.raises(ValueError, match="combined controller"):
        rti.step(np.zeros((1, 12)), sens=True)
    with pytest.raises(ValueError, match="combined controller"):
        rti.step(np.zeros((1, 12)), sens_w=True)
    rti.close()
