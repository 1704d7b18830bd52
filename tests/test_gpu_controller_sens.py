"""BatchController.step(sens=True) on the device (mpcb_step_sens on both engines): the feedback gain and the reference sensitivity
of u0 against central differences of the oracle-free dense KKT solve (tests/sens_checks.py), under the bound of
tests/test_emulation_sens.py; self-consistency between two controllers; ragged rows; the cases without sensitivities; sens=False
after sens=True; robotic_mpc_amd.autograd on the device.

SENS_DUMP=<file> collects the measured distances."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import dense_qp_cases as dc  # noqa: E402
import sens_cases as scs  # noqa: E402
import sens_checks as sc  # noqa: E402
from test_boundaries import BOUNDARIES, PICKED_4_2, force_geometry, geo_name  # noqa: E402

pytestmark = pytest.mark.gpu

# (engine, forced (wavefronts per simulation, simulations per CU) or None, cases of one batch)
RUNS = [("latency", None, ("N1-rand",)), ("latency", None, ("N9-rand",)), ("latency", None, ("N80-rand",)), ("latency", None, ("N130-rand",)),
        ("stream", None, ("N1-rand",)), ("stream", None, ("N7-rand",)), ("stream", None, ("N40-rand",)),
        ("stream", None, ("N3-rand", "N12-rand", "N40-rand"))] + \
       [("latency", geo, ("N%d-rand" % N,)) for geo in sorted(BOUNDARIES) for N in (20, 130)] + [("latency", PICKED_4_2, ("N20-rand",))]
_MEASURED = {}


def _run_id(r):
    return "%s%s-%s" % (r[0], "" if r[1] is None else "-" + geo_name(r[1]), "+".join(r[2]))


def _dump():
    if os.environ.get("SENS_DUMP"):
        with open(os.environ["SENS_DUMP"], "w") as f:
            for (tag, cid), v in sorted(_MEASURED.items()):
                f.write("%-28s %-12s distance %.2e  bound %.1e  d_ref %.1e  max|J| %.2e\n" % ((tag, cid) + v))


def _clean(monkeypatch, geo=None):
    for k in ("MPCB_WAVES_PER_SIM", "MPCB_SIMS_PER_CU", "MPCB_ENGINE"):
        monkeypatch.delenv(k, raising=False)
    if geo is not None:
        force_geometry(monkeypatch, geo)


def _controller(cases, engine):
    from robotic_mpc_amd import BatchController

    return BatchController([c["raw"] for c in cases], engine=engine)


def _reference_of(ctl, cases):
    if not any(c["yref"] is not None for c in cases):
        return None
    y = ctl.default_reference().cpu().numpy()
    for i, c in enumerate(cases):
        if c["yref"] is not None:
            y[i, :c["N"]] = c["yref"]
    return y


def _step(ctl, cases, **kw):
    kw.setdefault("yref", _reference_of(ctl, cases))
    return {k: v.cpu().numpy() for k, v in ctl.step(np.stack([c["xhat"] for c in cases]), **kw).items()}


def _all_nan(out, i):
    return out["sens_valid"][i] == 0 and np.isnan(out["du0_dx"][i]).all() and np.isnan(out["du0_dyref"][i]).all()


@pytest.mark.parametrize("engine,geo,cids", RUNS, ids=[_run_id(r) for r in RUNS])
def test_reset_step_sensitivities_against_dense(monkeypatch, engine, geo, cids):
    _clean(monkeypatch, geo)
    cases = [scs.case(c) for c in cids]
    ctl = _controller(cases, engine)
    out = _step(ctl, cases, sens=True)
    info = ctl.launch_info()
    ctl.close()
    assert info["engine"] == (1 if engine == "stream" else 0), info
    if geo is not None:
        assert info["waves_per_sim"] == geo[0] and info["pool_bytes"] == 8 * BOUNDARIES[geo[:2]]["pool"], info
    Nmax = max(c["N"] for c in cases)
    assert out["du0_dx"].shape == (len(cases), 6, 12) and out["du0_dyref"].shape == (len(cases), Nmax, 5, 6)
    tag = "%s%s" % (engine, "" if geo is None else "-" + geo_name(geo)) + ("-ragged" if len(cases) > 1 else "")
    for i, c in enumerate(cases):
        assert out["status"][i] == 0 and out["qp_iter"][i] == 1 and out["sens_valid"][i] == 1, (c["id"], out["qp_iter"][i])
        # (rows past the simulation's own horizon are exactly zero: checked inside)
        scs.check(c["id"], out["du0_dx"][i], out["du0_dyref"][i], tag, _MEASURED)
    _dump()


@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_two_controllers_are_consistent_with_the_jacobians(monkeypatch, engine):
    """A second controller of the same configuration stepped at (xhat + delta, yref + eta) returns u0 + J_x delta + sum_k J_y[k]'
    eta_k of the first: the map is affine, so this holds for any size of the offsets, within the bound scaled by them."""
    _clean(monkeypatch)
    c = scs.case("N20-ramp")
    rng = np.random.default_rng(9)
    delta, eta = rng.uniform(-1e-2, 1e-2, 12), rng.uniform(-1e-2, 1e-2, (20, 5))
    a, b = _controller([c], engine), _controller([c], engine)
    oa = _step(a, [c], sens=True)
    ob = {k: v.cpu().numpy() for k, v in b.step((c["xhat"] + delta)[None], yref=(c["yref"] + eta)[None]).items()}
    a.close(), b.close()
    assert oa["sens_valid"][0] == 1 and ob["qp_iter"][0] == 1 and ob["status"][0] == 0
    want = oa["u0"][0] + oa["du0_dx"][0] @ delta + np.einsum("kcu,kc->u", oa["du0_dyref"][0], eta)
    ref = scs.reference("N20-ramp")
    # (... plus what the two u0 themselves may be off their exact values: 10 x the case's committed distance each)
    bound = sc.bound(ref, scs.eps("N20-ramp")) * (np.abs(delta).sum() + np.abs(eta).sum()) + 2 * dc.tolerance(scs.ORACLE_VS_DENSE, "N20-ramp")
    d = np.abs(ob["u0"][0] - want).max()
    print(f"\n[sens] {engine} two controllers: |u0' - (u0 + J delta)| = {d:.2e} (bound {bound:.1e})")
    assert d <= bound


@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_no_sensitivities_where_the_qp_was_not_the_fast_path(monkeypatch, engine):
    _clean(monkeypatch)
    cases = [scs.case("N20-rand"), scs.case("N20-tight"), scs.case("N20-rand-ipm")]
    ctl = _controller(cases, engine)
    out = _step(ctl, cases, sens=True)
    assert (out["status"] == 0).all() and out["qp_iter"][0] == 1 and out["qp_iter"][1] > 1 and out["qp_iter"][2] > 1
    assert out["sens_valid"][0] == 1 and _all_nan(out, 1) and _all_nan(out, 2)
    scs.check("N20-rand", out["du0_dx"][0], out["du0_dyref"][0], engine + "-mixed", _MEASURED)
    alone = _controller(cases[:1], engine)
    oa = _step(alone, cases[:1], sens=True)
    alone.close()
    for k in ("u0", "du0_dx", "du0_dyref", "sens_valid"):
        np.testing.assert_array_equal(out[k][0], oa[k][0], err_msg=k)
    # the next step of the rejected simulation is suspended by the back-off: no attempt, no sensitivities
    x2 = np.stack([c["xhat"] for c in cases])
    x2[1] = np.concatenate([cases[1]["cfg"]["q0"], np.zeros(6)])
    out2 = {k: v.cpu().numpy() for k, v in ctl.step(x2, sens=True).items()}
    ctl.close()
    assert out2["status"][1] == 0 and _all_nan(out2, 1) and _all_nan(out2, 2) and out2["sens_valid"][0] == 1
    _dump()


@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_sens_false_after_sens_true_is_a_controller_that_never_asked(monkeypatch, engine):
    _clean(monkeypatch)
    c = scs.case(dc.CHAINED_CASE)
    a, b = _controller([c], engine), _controller([c], engine)
    x2 = c["xhat"] + np.random.default_rng(3).uniform(-5e-3, 5e-3, 12)
    _step(a, [c], sens=True, predict=True), _step(b, [c], predict=True)
    oa = {k: v.cpu().numpy() for k, v in a.step(x2[None], predict=True).items()}
    ob = {k: v.cpu().numpy() for k, v in b.step(x2[None], predict=True).items()}
    a.close(), b.close()
    assert "du0_dx" not in oa
    for k in ("u0", "status", "sqp_iter", "qp_iter", "residuals", "cost", "x_pred", "u_pred"):
        np.testing.assert_array_equal(oa[k], ob[k], err_msg=k)


@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_differentiable_step_on_the_device(monkeypatch, engine):
    import torch

    from robotic_mpc_amd.autograd import differentiable_step

    _clean(monkeypatch)
    cases = [scs.case("N20-rand"), scs.case("N20-tight")]
    ctl = _controller(cases, engine)
    dev = torch.device("cuda", ctl.device)
    x = torch.from_numpy(np.stack([c["xhat"] for c in cases])).to(dev).requires_grad_(True)
    y = ctl.default_reference().requires_grad_(True)
    u0 = differentiable_step(ctl, x, y, invalid="zero")
    gx, gy = torch.autograd.grad(u0.sum(), (x, y))
    ctl.reset()
    out = {k: v.clone() for k, v in ctl.step(x.detach(), yref=y.detach(), sens=True).items()}
    ctl.close()
    # The backward pass forms each entry as a sum of six products g_u J_u with g = 1, .sum() forms the same six terms in an order of
    # its own: two fp64 summations of n = 6 terms differ by at most 2 (n - 1) eps sum |J_u| (the standard bound of recursive
    # summation, either order), eps = 2^-53 the unit roundoff.  The Jacobians themselves are the same bits: a reset step is
    # deterministic (test_sens_false_after_sens_true..., the emulation's bit-for-bit tests).
    eps = 2.0 ** -53
    jx, jy = out["du0_dx"][0], out["du0_dyref"][0]
    ex, ey = (gx[0] - jx.sum(0)).abs(), (gy[0] - jy.sum(2)).abs()
    print(f"\n[sens] {engine} autograd: |grad - column sums| = {float(ex.max()):.2e}, {float(ey.max()):.2e}")
    assert bool((ex <= 10 * eps * jx.abs().sum(0)).all()) and bool((ey <= 10 * eps * jy.abs().sum(2)).all())
    assert float(jx.abs().sum(0).min()) > 1e-3                     # (the bound is not met by zeros: the gain's columns are O(1))
    assert (gx[1] == 0).all() and (gy[1] == 0).all() and int(out["sens_valid"][1]) == 0
