"""Sensitivities of u0 with the joint-wise terminal cost in force (mpcb_step_term with sens) on the emulated latency engine:
du0_dx, du0_dyref and du0_dxe = d u0 / d x_e against central differences of the dense KKT solve of the terminal QP
(tests/dense_qp_terminal.py dense_jacobians), on the reset step and on a stage-varying iterate.  The bound is sens_checks.bound: 10 x
max(the reference's own noise, the case's committed solver-vs-dense distance x max |J|)."""
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)

import dense_qp as dq  # noqa: E402
import dense_qp_cases as dc  # noqa: E402
import dense_qp_terminal as dqt  # noqa: E402
import sens_checks as sc  # noqa: E402
import terminal_cases as tc  # noqa: E402
from test_terminal_cases import BY_ID, CHAINED_ORACLE_VS_DENSE_TERM, ORACLE_VS_DENSE_TERM, emulated, record  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

RESET_HORIZONS = (1, 2, 7, 20)
# (wavefronts, pool) of tests/test_boundaries.py: one, four and eight wavefronts, a whole and half a CU's pool
GEOMETRIES = ((1, 19392), (4, 19392), (8, 9152))

_REFS = {}


def reset_reference(cid):
    """dense_jacobians of the case's reset-step QP, once per session."""
    if cid not in _REFS:
        c = BY_ID[cid]
        X, U = dc.guess(c)
        _REFS[cid] = dqt.dense_jacobians(dc.chain_of(c), c["cfg"], X, U, c["xhat"], c["P"], c["x_e"], c["yref"])
    return _REFS[cid]


def check_sens(ref, out, i, eps, tag, cid):
    assert out["sens_valid"][i] == 1
    N = ref["Jy"].shape[0]
    d = dqt.distance(ref, out["du0_dx"][i], out["du0_dyref"][i], out["du0_dxe"][i])
    b = sc.bound(ref, eps)
    print(f"\n[terminal-sens] {tag} {cid}: distance {d:.2e} bound {b:.1e} d_ref {ref['d_ref']:.1e} max|J| {ref['scale']:.2e} "
          f"max|Jxe| {np.abs(ref['Jxe']).max():.2e}")
    record(cid + "-sens", tag, d)
    assert d <= b, (tag, cid, d, b)
    # stage 0's reference row and the rows past the horizon are exactly zero
    assert (out["du0_dyref"][i][0] == 0.0).all() and (out["du0_dyref"][i][N:] == 0.0).all()
    # the terminal reference reaches u0: a missing du0_dxe (zeros, or the poison) is an O(1) relative error
    assert np.abs(ref["Jxe"]).max() >= 1e-2 and np.abs(out["du0_dxe"][i]).max() >= 0.5 * np.abs(ref["Jxe"]).max()


@pytest.mark.parametrize("waves,pool", GEOMETRIES, ids=["w%d-p%d" % g for g in GEOMETRIES])
@pytest.mark.parametrize("N", RESET_HORIZONS)
def test_reset_step_sensitivities_against_dense(N, waves, pool):
    cid = f"N{N}-rand-term"
    c = BY_ID[cid]
    out = emulated(c, waves, pool).step(c["xhat"][None], sens=True)
    assert out["status"][0] == 0 and out["qp_iter"][0] == 1
    check_sens(reset_reference(cid), out, 0, ORACLE_VS_DENSE_TERM[cid][0], "emu-w%d-p%d" % (waves, pool), cid)


def test_horizon_of_one_has_a_terminal_sensitivity():
    """With a horizon of 1 the reference rows are all zero, but x_1 is the terminal state: du0_dxe is the dense one, not zero."""
    c = BY_ID["N1-rand-term"]
    out = emulated(c, 1, 19392).step(c["xhat"][None], sens=True)
    ref = reset_reference("N1-rand-term")
    assert (out["du0_dyref"][0] == 0.0).all()
    assert np.abs(ref["Jxe"]).max() > 1.0
    assert np.abs(out["du0_dxe"][0] - ref["Jxe"]).max() <= sc.bound(ref, ORACLE_VS_DENSE_TERM["N1-rand-term"][0])


def stage_varying(case, step):
    """Two carried steps on the off-model plant of terminal_cases.chained, then the step under test: returns (the dense reference
    assembled at the solver's own previous iterate with the new feedback state, that step's output)."""
    cfg = case["cfg"]
    Ap, Bp = dq.lti(0.8 * np.asarray(cfg["wcv"]), cfg["dt"])
    rng = np.random.default_rng(77)
    x = case["xhat"].copy()
    for _ in range(2):
        out = step(x, False)
        assert out["status"][0] == 0
        prev = (out["x_pred"][0].copy(), out["u_pred"][0].copy())
        x = Ap @ x + Bp @ prev[1][0] + rng.uniform(-1e-3, 1e-3, 12)
    assert np.abs(np.diff(prev[0], axis=0)).max() > 1e-4                 # the iterate varies from stage to stage
    ref = dqt.dense_jacobians(dc.chain_of(case), cfg, prev[0], prev[1], x, case["P"], case["x_e"], case["yref"])
    return ref, step(x, True)


def test_stage_varying_iterate_sensitivities_against_dense():
    case = BY_ID[tc.CHAINED_CASE]
    ctl = emulated(case, 4, 19392)
    ref, out = stage_varying(case, lambda x, sens: ctl.step(x[None], sens=sens))
    assert out["status"][0] == 0 and out["qp_iter"][0] == 1
    check_sens(ref, out, 0, max(CHAINED_ORACLE_VS_DENSE_TERM[False]), "emu-w4-p19392", "N20-carried")


def test_no_sensitivities_through_the_interior_point():
    c = BY_ID["N20-rand-term-ipm"]
    out = emulated(c, 4, 19392).step(c["xhat"][None], sens=True)
    assert out["status"][0] == 0 and out["sens_valid"][0] == 0
    assert np.isnan(out["du0_dx"][0]).all() and np.isnan(out["du0_dyref"][0]).all() and np.isnan(out["du0_dxe"][0]).all()


def test_the_step_is_unchanged_by_the_sensitivity_pass():
    c = BY_ID["N20-rand-term"]
    a = emulated(c, 4, 19392).step(c["xhat"][None], sens=False)
    b = emulated(c, 4, 19392).step(c["xhat"][None], sens=True)
    for k in ("u0", "x_pred", "u_pred", "cost", "qp_iter", "residuals"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
