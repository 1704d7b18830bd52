"""Host emulation of the controller step that returns the feedback gain and the reference sensitivity of u0
(Engine::control_step<true, true> with Engine::sens_pass, the device code behind mpcb_step_sens) on the latency engine, at 1, 2, 4
and 8 wavefronts: against central differences of the oracle-free dense KKT solve (tests/sens_checks.py), the exact zeros, the
cases without sensitivities, and the step's independence of the pass.

SENS_DUMP=<file> collects the measured distances (profiles/step_sens_distances.txt)."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_qp_cases as dc  # noqa: E402
import sens_cases as scs  # noqa: E402
import sens_checks as sc  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

WAVES = (1, 2, 4, 8)
POOL = 19392
# N = 1, 2, 9, 30 and the reference ramp / tool offset / Levenberg-Marquardt cases at every wave count ...
BASIC = ("N1-rand", "N2-rand", "N9-rand", "N30-rand", "N20-ramp", "N20-tool", "N20-lm")
# ... and both sides of the resident -> streaming switches that tests/test_boundaries.py pins (one wavefront: 42 | 43 with half a
# CU's pool, 140 | 141 with a whole one; two wavefronts: 37 | 38), plus one horizon of the register and of the segment family, whose
# gains come from G4 as the streaming family's do: (case, wavefronts, pool, sweep family)
SWITCH = [("N42-rand", 1, 9152, "resident"), ("N43-rand", 1, 9152, "streaming"), ("N37-rand", 2, 9152, "resident"),
          ("N38-rand", 2, 9152, "streaming"), ("N140-rand", 1, 19392, "resident"), ("N141-rand", 1, 19392, "streaming"),
          ("N26-rand", 4, 9152, "register"), ("N126-rand", 8, 19392, "segment")]

_MEASURED = {}


def _dump():
    if os.environ.get("SENS_DUMP"):
        with open(os.environ["SENS_DUMP"], "w") as f:
            for (tag, cid), v in sorted(_MEASURED.items()):
                f.write("%-28s %-12s distance %.2e  bound %.1e  d_ref %.1e  max|J| %.2e\n" % ((tag, cid) + v))


def _ctl(cases, waves, pool=POOL):
    import emu_sens

    return emu_sens.Controller([c["cfg"] for c in cases], dc.chain_of(cases[0]), pool_doubles=pool, waves=waves)


def _step(ctl, cases, **kw):
    y = None
    if any(c["yref"] is not None for c in cases):
        assert len(cases) == 1
        y = cases[0]["yref"][None]
    return ctl.step(np.stack([c["xhat"] for c in cases]), yref=y, ref_changed=y is not None, **kw)


def _all_nan(out, i):
    return out["sens_valid"][i] == 0 and np.isnan(out["du0_dx"][i]).all() and np.isnan(out["du0_dyref"][i]).all()


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("cid", BASIC)
def test_reset_step_sensitivities_against_dense(cid, waves):
    c = scs.case(cid)
    out = _step(_ctl([c], waves), [c])
    assert out["status"][0] == 0 and out["qp_iter"][0] == 1 and out["sens_valid"][0] == 1
    scs.check(cid, out["du0_dx"][0], out["du0_dyref"][0], "emu-w%d" % waves, _MEASURED)
    if c["N"] == 1:
        assert (out["du0_dyref"][0] == 0.0).all()
    _dump()


@pytest.mark.parametrize("cid,waves,pool,sweep", SWITCH, ids=["%s-w%d-p%d-%s" % s for s in SWITCH])
def test_both_sides_of_the_sweep_switches(cid, waves, pool, sweep):
    import emu

    c = scs.case(cid)
    assert emu.emu_paths(c["N"], pool, waves)["sweep"] == sweep
    out = _step(_ctl([c], waves, pool), [c])
    assert out["status"][0] == 0 and out["qp_iter"][0] == 1 and out["sens_valid"][0] == 1
    scs.check(cid, out["du0_dx"][0], out["du0_dyref"][0], "emu-w%d-p%d-%s" % (waves, pool, sweep), _MEASURED)
    _dump()


@pytest.mark.parametrize("waves", WAVES)
def test_without_du0_dyref_the_gain_alone(waves):
    c = scs.case("N9-rand")
    out = _step(_ctl([c], waves), [c], sens="dx")
    assert out["sens_valid"][0] == 1
    assert np.abs(out["du0_dx"][0] - scs.reference("N9-rand")["Jx"]).max() <= sc.bound(scs.reference("N9-rand"), scs.eps("N9-rand"))


@pytest.mark.parametrize("waves", WAVES)
def test_no_sensitivities_where_the_qp_was_not_the_fast_path(waves):
    """Active bounds (the attempt is rejected), the fast path off, and the step after a rejected attempt, whose attempt the
    back-off suspends: valid 0 and NaN everywhere; a valid neighbour in the same batch is what it is alone, bit for bit."""
    good, tight, ipm = scs.case("N20-rand"), scs.case("N20-tight"), scs.case("N20-rand-ipm")
    cases = [good, tight, ipm]
    ctl = _ctl(cases, waves)
    out = _step(ctl, cases)
    assert (out["status"] == 0).all() and out["qp_iter"][0] == 1 and out["qp_iter"][1] > 1 and out["qp_iter"][2] > 1
    assert out["sens_valid"][0] == 1 and _all_nan(out, 1) and _all_nan(out, 2)
    scs.check("N20-rand", out["du0_dx"][0], out["du0_dyref"][0], "emu-mixed-w%d" % waves)
    alone = [_step(_ctl([c], waves), [c]) for c in cases]
    for i in range(3):
        for k in ("u0", "x_pred", "u_pred", "du0_dx", "du0_dyref", "sens_valid", "qp_iter", "cost", "residuals"):
            np.testing.assert_array_equal(out[k][i], alone[i][k][0], err_msg=f"{k} sim {i}")
    # second step: the rejected attempt of step 1 suspends the attempt of this one (its QP count has no fast-path try in it:
    # the interior point alone), whatever the state -- here one that would be accepted
    x2 = np.stack([c["xhat"] for c in cases])
    x2[1] = np.concatenate([tight["cfg"]["q0"], np.zeros(6)])
    out2 = ctl.step(x2)
    assert out2["status"][1] == 0 and _all_nan(out2, 1) and _all_nan(out2, 2)
    assert out2["sens_valid"][0] == 1 and out2["qp_iter"][0] == 1


@pytest.mark.parametrize("waves", WAVES)
def test_the_pass_leaves_the_step_alone_and_a_chained_step_matches_dense(waves):
    """With and without the pass: identical u0, statistics and prediction, on the reset step and on the next one (the solver memory
    is untouched).  The second step -- carried linearisation, fast path accepted -- against the dense reference built at the
    carried iterate."""
    c = scs.case(dc.CHAINED_CASE)
    a, b = _ctl([c], waves), _ctl([c], waves)
    oa, ob = _step(a, [c]), _step(b, [c], sens=False)
    x2 = c["xhat"] + np.random.default_rng(3).uniform(-5e-3, 5e-3, 12)
    prev = (oa["x_pred"][0].copy(), oa["u_pred"][0].copy())
    oa2, ob2 = a.step(x2[None]), b.step(x2[None], sens=False)
    for p, q in ((oa, ob), (oa2, ob2)):
        assert "du0_dx" not in q
        for k in ("u0", "status", "sqp_iter", "qp_iter", "residuals", "cost", "x_pred", "u_pred"):
            np.testing.assert_array_equal(p[k], q[k], err_msg=k)
    assert oa2["qp_iter"][0] == 1 and oa2["sens_valid"][0] == 1
    ref = sc.dense_jacobians(dc.chain_of(c), c["cfg"], prev[0], prev[1], x2, c["yref"])
    bound = sc.bound(ref, scs.CHAINED_ORACLE_VS_DENSE[1])
    d = sc.distance(ref, oa2["du0_dx"][0], oa2["du0_dyref"][0])
    print(f"\n[sens] emu-w{waves} chained step: |J - J_dense| = {d:.2e} (bound {bound:.1e})")
    _MEASURED[("emu-w%d" % waves, "chained-step1")] = (d, bound, ref["d_ref"], ref["scale"])
    assert d <= bound and (oa2["du0_dyref"][0, 0] == 0.0).all()
    np.testing.assert_allclose(oa2["u0"][0], ref["u0"], atol=1e-12, rtol=0)
    _dump()
