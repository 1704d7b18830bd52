"""Host emulation of the controller step that returns the sensitivity of u0 to the seven cost weights
(Engine::control_step<true, true, true> with Engine::sens_pass<true>, the device code behind mpcb_step_sens_w) and of the run-time
weight update (mpcb_set_weights) on the latency engine, at 1, 2, 4 and 8 wavefronts: against the oracle-free dense reference of
tests/sensw_checks.py, the exact zeros, the cases without sensitivities, and the step's independence of the new output.

The throughput engine is device code only (no host build): its pass is covered on the device (tests/test_gpu_controller_sensw.py,
the ragged batch included).

Measured: every row of every case is 1e-16 to 3e-14 of the row's max |J| from the dense reference, at most 0.31 of its bound (row
0 of N1-rand, whose bound is the eps(case) A_p term: 2.1e-17 against 6.7e-17).  Row 1 (w_qddot) of N1-rand is the least accurate
relative to its size, 4.9e-15 of 3.8e-02: at N = 1 the optimal u0 is within 1e-3 of the measured joint velocity, (u+ - v+) cancels
three digits and a one-ulp difference of u0 shows; the re-assembled reference has the same cancellation and reports it
(d_ref 1.2e-14).

SENSW_DUMP=<file> collects the measured distances (profiles/step_sensw_distances.txt)."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_qp_cases as dc  # noqa: E402
import sens_cases as scs  # noqa: E402
import sensw_cases as swc  # noqa: E402
import sensw_checks as sw  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

WAVES = (1, 2, 4, 8)
POOL = 19392
RESET = ("N1-rand", "N3-rand", "N9-rand", "N20-rand", "N40-rand", "N20-ramp")

_MEASURED = {}


def _dump():
    if os.environ.get("SENSW_DUMP"):
        swc.dump(os.environ["SENSW_DUMP"], _MEASURED)


def _ctl(cases, waves, pool=POOL):
    import emu_sensw

    return emu_sensw.Controller([c["cfg"] for c in cases], dc.chain_of(cases[0]), pool_doubles=pool, waves=waves)


def _step(ctl, cases, **kw):
    y = None
    if any(c["yref"] is not None for c in cases):
        assert len(cases) == 1
        y = cases[0]["yref"][None]
    return ctl.step(np.stack([c["xhat"] for c in cases]), yref=y, ref_changed=y is not None, **kw)


@pytest.mark.parametrize("cid", swc.CASES)
def test_the_reference_agrees_with_central_differences_of_the_full_dense_solve(cid):
    """Guards against a sign error in the reference, not precision: 1e-6 of the row's max."""
    c = scs.case(cid)
    X, U = dc.guess(c)
    ref = swc.reference(cid)
    sw.bounds(ref, scs.eps(cid))                                   # the condition: every row's bound <= 1e-6 of its scale
    cd = sw.central_differences(dc.chain_of(c), c["cfg"], X, U, c["xhat"], c["yref"])
    d = np.abs(cd - ref["J"]).max(axis=1)
    print(f"\n[sensw] {cid}: |central differences - J| = {d.max():.2e}")
    assert (d <= sw.CD_AGREE * ref["scale"]).all(), (d, ref["scale"])
    if c["N"] == 1:
        assert (ref["J"][2:] == 0.0).all()


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("cid", RESET)
def test_reset_step_weight_sensitivity_against_dense(cid, waves):
    c = scs.case(cid)
    out = _step(_ctl([c], waves), [c])
    assert out["status"][0] == 0 and out["qp_iter"][0] == 1 and out["sens_valid"][0] == 1
    scs.check(cid, out["du0_dx"][0], out["du0_dyref"][0], "emu-w%d" % waves)
    try:
        swc.check(cid, out["du0_dw"][0], "emu-w%d" % waves, _MEASURED)
    finally:
        _dump()


@pytest.mark.parametrize("waves", WAVES)
def test_without_du0_dyref_the_recursion_still_runs(waves):
    c = scs.case("N9-rand")
    out = _step(_ctl([c], waves), [c], sens="dx")
    assert out["sens_valid"][0] == 1
    swc.check("N9-rand", out["du0_dw"][0], "emu-nody-w%d" % waves)


@pytest.mark.parametrize("waves", WAVES)
def test_set_weights_with_distinct_task_weights_and_a_zero(waves):
    """Through the set-weights path: distinct task weights, one of them 0 (its derivative exists: nothing divides by a weight),
    w_u and w_qddot moved; u0 and du0_dw against the dense solve at the new weights."""
    c = scs.case("N12-rand")
    th = swc.random_weights(c["cfg"], np.random.default_rng(8000), zero=2)
    assert th[4] == 0.0 and len(set(th[2:])) == 5
    ctl = _ctl([c], waves)
    ctl.set_weights(th)
    out = _step(ctl, [c])
    assert out["status"][0] == 0 and out["qp_iter"][0] == 1 and out["sens_valid"][0] == 1
    X, U = dc.guess(c)
    ref = sw.dense_weight_jacobian(dc.chain_of(c), sw.with_weights(c["cfg"], th), X, U, c["xhat"], c["yref"])
    np.testing.assert_allclose(out["u0"][0], ref["u0"], atol=swc.u0_bound("N12-rand"), rtol=0)
    try:
        swc.check_against(ref, scs.eps("N12-rand"), out["du0_dw"][0], "emu-setw-w%d" % waves, "N12-rand", _MEASURED)
    finally:
        _dump()
    # the packed weights give another control
    base = _step(_ctl([c], waves), [c])
    assert np.abs(base["u0"][0] - out["u0"][0]).max() > 1e-6


@pytest.mark.parametrize("waves", WAVES)
def test_no_weight_sensitivity_where_the_qp_was_not_the_fast_path(waves):
    """Active bounds (the attempt is rejected) and the fast path off: valid 0 and all 42 entries NaN; a valid neighbour in the same
    batch is what it is alone, bit for bit."""
    good, tight, ipm = scs.case("N20-rand"), scs.case("N20-tight"), scs.case("N20-rand-ipm")
    cases = [good, tight, ipm]
    out = _step(_ctl(cases, waves), cases)
    assert (out["status"] == 0).all() and out["qp_iter"][0] == 1 and out["qp_iter"][1] > 1 and out["qp_iter"][2] > 1
    assert list(out["sens_valid"]) == [1, 0, 0]
    assert np.isnan(out["du0_dw"][1]).all() and np.isnan(out["du0_dw"][2]).all()
    swc.check("N20-rand", out["du0_dw"][0], "emu-mixed-w%d" % waves)
    alone = _step(_ctl([good], waves), [good])
    np.testing.assert_array_equal(out["du0_dw"][0], alone["du0_dw"][0])


@pytest.mark.parametrize("waves", WAVES)
def test_the_new_output_leaves_the_step_alone_and_a_chained_step_matches_dense(waves):
    """With du0_dw, with the sensitivities alone and without any: identical u0, statistics and prediction, on the reset step and on
    the next one; du0_dx / du0_dyref bit-identical with and without du0_dw.  The second step -- carried linearisation, fast path
    accepted -- against the dense reference built at the carried iterate."""
    c = scs.case(dc.CHAINED_CASE)
    a, b, n = _ctl([c], waves), _ctl([c], waves), _ctl([c], waves)
    oa, ob, on = _step(a, [c]), _step(b, [c], sens_w=False), _step(n, [c], sens=False)
    x2 = c["xhat"] + np.random.default_rng(3).uniform(-5e-3, 5e-3, 12)
    prev = (oa["x_pred"][0].copy(), oa["u_pred"][0].copy())
    oa2, ob2, on2 = a.step(x2[None]), b.step(x2[None], sens_w=False), n.step(x2[None], sens=False)
    for p, q, r in ((oa, ob, on), (oa2, ob2, on2)):
        assert "du0_dw" not in q and "du0_dx" not in r
        for k in ("u0", "status", "sqp_iter", "qp_iter", "residuals", "cost", "x_pred", "u_pred"):
            np.testing.assert_array_equal(p[k], q[k], err_msg=k)
            np.testing.assert_array_equal(p[k], r[k], err_msg=k)
        for k in ("du0_dx", "du0_dyref", "sens_valid"):
            np.testing.assert_array_equal(p[k], q[k], err_msg=k)
    assert oa2["qp_iter"][0] == 1 and oa2["sens_valid"][0] == 1
    ref = sw.dense_weight_jacobian(dc.chain_of(c), c["cfg"], prev[0], prev[1], x2, c["yref"])
    np.testing.assert_allclose(oa2["u0"][0], ref["u0"], atol=1e-12, rtol=0)
    try:
        swc.check_against(ref, scs.CHAINED_ORACLE_VS_DENSE[1], oa2["du0_dw"][0], "emu-w%d" % waves, "chained-step1", _MEASURED)
    finally:
        _dump()


@pytest.mark.parametrize("waves", (1, 4))
def test_set_weights_on_a_carried_step_relinearises_and_everything_else_carries(waves):
    """Step, set_weights, step without reset: the second step is the step of a controller whose second step got ref_changed with
    the same weights in its records from the start of that step -- and against dense at the carried iterate with the new weights."""
    c = scs.case(dc.CHAINED_CASE)
    th = sw.theta(c["cfg"]) * np.array([1.5, 0.7, 1.2, 0.5, 2.0, 1.0, 0.9])
    a = _ctl([c], waves)
    oa = _step(a, [c])
    prev = (oa["x_pred"][0].copy(), oa["u_pred"][0].copy())
    a.set_weights(th)
    oa2 = a.step(c["xhat"][None])
    assert oa2["status"][0] == 0 and oa2["qp_iter"][0] == 1 and oa2["sens_valid"][0] == 1
    ref = sw.dense_weight_jacobian(dc.chain_of(c), sw.with_weights(c["cfg"], th), prev[0], prev[1], c["xhat"], c["yref"])
    np.testing.assert_allclose(oa2["u0"][0], ref["u0"], atol=1e-12, rtol=0)
    swc.check_against(ref, scs.CHAINED_ORACLE_VS_DENSE[1], oa2["du0_dw"][0], "emu-carry-setw-w%d" % waves, "chained-step1")
