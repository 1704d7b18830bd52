"""BatchController.set_weights and step(sens_w=True) on the device (mpcb_set_weights, mpcb_step_sens_w on both engines): du0_dw
against the oracle-free dense reference of tests/sensw_checks.py under the bound of tests/sensw_cases.py, run-time weights against
the dense solve at the new weights, the carried step after a weight change, the cases without sensitivities, the steps after a
sens_w step, and robotic_mpc_amd.autograd with weights on the device.

SENSW_DUMP=<file> collects the measured distances (profiles/step_sensw_distances.txt)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import dense_qp_cases as dc  # noqa: E402
import sens_cases as scs  # noqa: E402
import sensw_cases as swc  # noqa: E402
import sensw_checks as sw  # noqa: E402
from test_boundaries import BOUNDARIES, PICKED_4_2, force_geometry, geo_name  # noqa: E402

pytestmark = pytest.mark.gpu

# (engine, forced (wavefronts per simulation, simulations per CU) or None, cases of one batch): the table of the sens test
RUNS = [("latency", None, ("N1-rand",)), ("latency", None, ("N9-rand",)), ("latency", None, ("N80-rand",)), ("latency", None, ("N130-rand",)),
        ("stream", None, ("N1-rand",)), ("stream", None, ("N7-rand",)), ("stream", None, ("N40-rand",)),
        ("stream", None, ("N3-rand", "N12-rand", "N40-rand"))] + \
       [("latency", geo, ("N%d-rand" % N,)) for geo in sorted(BOUNDARIES) for N in (20, 130)] + [("latency", PICKED_4_2, ("N20-rand",))]
_MEASURED = {}


def _run_id(r):
    return "%s%s-%s" % (r[0], "" if r[1] is None else "-" + geo_name(r[1]), "+".join(r[2]))


def _dump():
    if os.environ.get("SENSW_DUMP"):
        swc.dump(os.environ["SENSW_DUMP"], _MEASURED)


def _clean(monkeypatch, geo=None):
    for k in ("MPCB_WAVES_PER_SIM", "MPCB_SIMS_PER_CU", "MPCB_ENGINE"):
        monkeypatch.delenv(k, raising=False)
    if geo is not None:
        force_geometry(monkeypatch, geo)


def _controller(cases, engine):
    from robotic_mpc_amd import BatchController

    return BatchController([c["raw"] for c in cases], engine=engine)


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _step(ctl, cases, **kw):
    return _np(ctl.step(np.stack([c["xhat"] for c in cases]), **kw))


@pytest.mark.parametrize("engine,geo,cids", RUNS, ids=[_run_id(r) for r in RUNS])
def test_reset_step_weight_sensitivity_against_dense(monkeypatch, engine, geo, cids):
    _clean(monkeypatch, geo)
    cases = [scs.case(c) for c in cids]
    ctl = _controller(cases, engine)
    out = _step(ctl, cases, sens_w=True)
    info = ctl.launch_info()
    ctl.close()
    assert info["engine"] == (1 if engine == "stream" else 0), info
    if geo is not None:
        assert info["waves_per_sim"] == geo[0] and info["pool_bytes"] == 8 * BOUNDARIES[geo[:2]]["pool"], info
    assert out["du0_dw"].shape == (len(cases), 7, 6)
    tag = "%s%s" % (engine, "" if geo is None else "-" + geo_name(geo)) + ("-ragged" if len(cases) > 1 else "")
    try:
        for i, c in enumerate(cases):
            assert out["status"][i] == 0 and out["qp_iter"][i] == 1 and out["sens_valid"][i] == 1, (c["id"], out["qp_iter"][i])
            scs.check(c["id"], out["du0_dx"][i], out["du0_dyref"][i], tag)
            swc.check(c["id"], out["du0_dw"][i], tag, _MEASURED)
    finally:
        _dump()


@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_set_weights_then_a_reset_step_against_dense_at_the_new_weights(monkeypatch, engine):
    _clean(monkeypatch)
    cids = ("N20-rand", "N20-rand", "N20-rand") if engine == "latency" else ("N7-rand", "N20-rand", "N40-rand")
    cases = [scs.case(c) for c in cids]
    rng = np.random.default_rng(8100)
    th = np.stack([swc.random_weights(c["cfg"], rng, zero=2 if i == 1 else None) for i, c in enumerate(cases)])
    ctl = _controller(cases, engine)
    np.testing.assert_array_equal(ctl.weights().cpu().numpy(), ctl.packed_weights())
    ctl.set_weights(th)
    np.testing.assert_array_equal(ctl.weights().cpu().numpy(), th)
    out = _step(ctl, cases, sens_w=True)
    ctl.close()
    try:
        for i, c in enumerate(cases):
            assert out["status"][i] == 0 and out["qp_iter"][i] == 1 and out["sens_valid"][i] == 1, (c["id"], out["qp_iter"][i])
            X, U = dc.guess(c)
            ref = sw.dense_weight_jacobian(dc.chain_of(c), sw.with_weights(c["cfg"], th[i]), X, U, c["xhat"], c["yref"])
            d = np.abs(out["u0"][i] - ref["u0"]).max()
            print(f"\n[sensw] {engine} set_weights sim {i} {c['id']}: |u0 - dense| = {d:.2e} (bound {swc.u0_bound(c['id']):.1e})")
            assert d <= swc.u0_bound(c["id"])
            swc.check_against(ref, scs.eps(c["id"]), out["du0_dw"][i], engine + "-setw%d" % i, c["id"], _MEASURED)
    finally:
        _dump()


@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_a_weight_change_on_a_carried_step_is_the_relinearisation_of_a_new_reference(monkeypatch, engine):
    """Step, set_weights, step without reset: bit for bit the second step of a controller that took the same first step and then
    got the unchanged reference set again plus the same weights -- the relinearisation is the ref_changed one, everything else
    carries.  set_weights(None) then restores the packed behaviour."""
    _clean(monkeypatch)
    c = scs.case(dc.CHAINED_CASE)
    th = swc.random_weights(c["cfg"], np.random.default_rng(8200))
    a, b, f = _controller([c], engine), _controller([c], engine), _controller([c], engine)
    x2 = c["xhat"] + np.random.default_rng(3).uniform(-5e-3, 5e-3, 12)
    oa, ob = _step(a, [c]), _step(b, [c])
    np.testing.assert_array_equal(oa["u0"], ob["u0"])
    a.set_weights(th)
    b.set_reference(b.default_reference())
    b.set_weights(th[None].repeat(1, 0))
    oa2, ob2 = _np(a.step(x2[None])), _np(b.step(x2[None]))
    assert oa2["qp_iter"][0] == 1 and ob2["qp_iter"][0] == 1 and oa2["status"][0] == 0
    for k in ("u0", "status", "sqp_iter", "qp_iter", "residuals", "cost"):
        np.testing.assert_array_equal(oa2[k], ob2[k], err_msg=k)
    # the weights did change the step
    n = _controller([c], engine)
    _step(n, [c])
    on2 = _np(n.step(x2[None]))
    assert np.abs(on2["u0"] - oa2["u0"]).max() > 1e-6
    # back to the packed weights: a reset step is the reset step of a fresh controller
    a.set_weights(None)
    np.testing.assert_array_equal(a.weights().cpu().numpy(), a.packed_weights())
    a.reset()
    oa3, of = _step(a, [c]), _step(f, [c])
    for k in ("u0", "status", "qp_iter", "residuals", "cost"):
        np.testing.assert_array_equal(oa3[k], of[k], err_msg=k)
    for ctl in (a, b, f, n):
        ctl.close()


@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_all_42_entries_are_nan_exactly_where_there_are_no_sensitivities(monkeypatch, engine):
    _clean(monkeypatch)
    cases = [scs.case("N20-rand"), scs.case("N20-tight"), scs.case("N20-rand-ipm")]
    ctl = _controller(cases, engine)
    out = _step(ctl, cases, sens_w=True)
    ctl.close()
    assert (out["status"] == 0).all() and list(out["sens_valid"]) == [1, 0, 0]
    assert np.isfinite(out["du0_dw"][0]).all() and np.isnan(out["du0_dw"][1]).all() and np.isnan(out["du0_dw"][2]).all()
    swc.check("N20-rand", out["du0_dw"][0], engine + "-mixed", _MEASURED)
    _dump()


@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_steps_after_a_sens_w_step_are_those_of_a_controller_that_never_asked(monkeypatch, engine):
    _clean(monkeypatch)
    c = scs.case(dc.CHAINED_CASE)
    a, b = _controller([c], engine), _controller([c], engine)
    rng = np.random.default_rng(3)
    x2, x3 = c["xhat"] + rng.uniform(-5e-3, 5e-3, 12), c["xhat"] + rng.uniform(-5e-3, 5e-3, 12)
    oa, ob = _step(a, [c], sens_w=True, predict=True), _step(b, [c], sens=True, predict=True)
    for k in ("u0", "du0_dx", "du0_dyref", "sens_valid", "x_pred", "u_pred", "cost", "residuals"):
        np.testing.assert_array_equal(oa[k], ob[k], err_msg=k)
    oa2, ob2 = _np(a.step(x2[None], sens=True, predict=True)), _np(b.step(x2[None], sens=True, predict=True))
    oa3, ob3 = _np(a.step(x3[None], predict=True)), _np(b.step(x3[None], predict=True))
    a.close(), b.close()
    assert "du0_dw" not in oa2 and "du0_dx" not in oa3
    for p, q in ((oa2, ob2), (oa3, ob3)):
        for k in p:
            if k != "solver_time":
                np.testing.assert_array_equal(p[k], q[k], err_msg=k)


@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_differentiable_step_with_weights_on_the_device(monkeypatch, engine):
    import torch

    from robotic_mpc_amd.autograd import differentiable_step

    _clean(monkeypatch)
    cases = [scs.case("N20-rand"), scs.case("N20-tight")]
    ctl = _controller(cases, engine)
    dev = torch.device("cuda", ctl.device)
    x = torch.from_numpy(np.stack([c["xhat"] for c in cases])).to(dev)
    w = ctl.weights().requires_grad_(True)
    u0 = differentiable_step(ctl, x, weights=w, invalid="zero")
    (gw,) = torch.autograd.grad(u0.sum(), (w,))
    ctl.reset()
    out = {k: v.clone() for k, v in ctl.step(x, sens_w=True).items()}
    ctl.close()
    # two fp64 summations of the same n = 6 terms differ by at most 2 (n - 1) eps sum |J_u| (tests/test_gpu_controller_sens.py);
    # the Jacobians themselves are the same bits: a reset step is deterministic
    eps = 2.0 ** -53
    jw = out["du0_dw"][0]
    e = (gw[0] - jw.sum(1)).abs()
    print(f"\n[sensw] {engine} autograd: |grad - column sums| = {float(e.max()):.2e}")
    assert bool((e <= 10 * eps * jw.abs().sum(1)).all())
    assert float(jw.abs().sum(1).max()) > 1e-6                     # (the bound is not met by zeros)
    assert (gw[1] == 0).all() and int(out["sens_valid"][1]) == 0 and bool(torch.isnan(out["du0_dw"][1]).all())
