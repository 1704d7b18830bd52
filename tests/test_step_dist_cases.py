"""The input disturbance of the controller step's prediction model (mpcb_step_dist) on the CPU: the cases of tests/step_dist_cases.py,
the oracle's QP routines and the emulated latency engine (tests/emu/emu_dist*) against the dense KKT reference of
tests/dense_qp_dist.py.

ORACLE_VS_DENSE_DIST is the committed record of how far the oracle's solution of every disturbed QP lies from the dense one (and of
the dense solve's LU-vs-refined estimate); the bound of every engine-vs-dense comparison, here and in tests/test_gpu_step_dist.py, is
10 x that distance, floor 1e-12, and stays <= 1e-9 (the rule of tests/test_dense_qp.py).
"""
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
import dense_qp_dist as dd  # noqa: E402
import step_dist_cases as sd  # noqa: E402

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

# case id -> (max |oracle - dense| over dX, dU; max |plain LU - refined| of the dense solve), measured on the CPU
ORACLE_VS_DENSE_DIST = {
    "N1-rand-dist": (1.11e-16, 1.1e-16),
    "N2-rand-dist": (2.78e-16, 2.2e-16),
    "N3-rand-dist": (2.78e-16, 1.1e-16),
    "N7-rand-dist": (1.05e-15, 1.2e-15),
    "N20-rand-dist": (6.44e-15, 6.3e-15),
    "N25-rand-dist": (4.44e-16, 1.0e-15),
    "N26-rand-dist": (5.27e-16, 7.5e-16),
    "N37-rand-dist": (5.27e-15, 4.8e-15),
    "N38-rand-dist": (7.04e-14, 3.7e-14),
    "N42-rand-dist": (2.03e-15, 5.7e-16),
    "N43-rand-dist": (9.44e-16, 1.4e-15),
    "N80-rand-dist": (3.16e-15, 5.2e-15),
    "N125-rand-dist": (1.11e-13, 5.3e-14),
    "N126-rand-dist": (3.50e-15, 1.4e-15),
    "N130-rand-dist": (8.66e-14, 3.8e-14),
    "N135-rand-dist": (4.83e-15, 2.9e-15),
    "N136-rand-dist": (5.64e-14, 4.5e-14),
    "N140-rand-dist": (5.46e-14, 5.4e-14),
    "N141-rand-dist": (1.15e-13, 1.2e-13),
    "N245-rand-dist": (2.16e-12, 1.3e-13),
    "N246-rand-dist": (5.84e-13, 6.5e-14),
    "N20-rand-dist-ipm": (1.13e-14, 6.3e-15),
    "N130-rand-dist-ipm": (6.62e-14, 3.8e-14),
    "N20-tight-dist": (2.89e-11, 6.7e-16),
    "N20-tight-dist-ipm": (2.89e-11, 6.7e-16),
}
N_CASES = 25

CASES = sd.all_cases()
BY_ID = sd.by_id()


def test_case_list_is_complete():
    assert len(CASES) == N_CASES and sorted(ORACLE_VS_DENSE_DIST) == sorted(BY_ID)
    for N in (1, 2, 3, 7, 20, 25, 26, 37, 38, 42, 43, 80, 125, 126, 130, 135, 136, 140, 141, 245, 246):
        assert BY_ID[f"N{N}-rand-dist"]["fast"]
    for N in (20, 130):
        assert not BY_ID[f"N{N}-rand-dist-ipm"]["fast"]
    assert BY_ID["N20-tight-dist"]["fast"] and not BY_ID["N20-tight-dist-ipm"]["fast"]
    for cid in ("N20-tight-dist", "N20-tight-dist-ipm"):
        assert BY_ID[cid]["certify"] and BY_ID[cid]["active"]
    assert max(sd.tolerance(ORACLE_VS_DENSE_DIST, cid) for cid in BY_ID) <= 1e-9
    for c in CASES:
        m = sd.D_TRY.get(c["N"], 0) if not c["certify"] else 0
        assert c["d_seed"] == 900 + c["N"] + 1000 * m
        np.testing.assert_array_equal(c["d"], np.random.default_rng(c["d_seed"]).uniform(-0.1, 0.1, 6))
        assert c["d"].shape == (6,) and (np.abs(c["d"]) <= 0.1).all() and np.abs(c["d"]).max() > 0.01


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if not c["active"]])
def test_inactive_minimisers_clear_every_bound(cid):
    """From the dense solution alone: the bound-free minimiser of every inactive disturbed QP is >= 0.05 inside every bound, at the
    FIRST m of the seed rule (every smaller m leaves less), and the disturbance moves u0 by >= 0.05 (measured 0.064 .. 0.099), fifty
    million times the largest bound of these tests (1e-9) -- a kernel that ignores d cannot pass."""
    c = BY_ID[cid]
    assert sd.clearance(c) >= sd.CLEARANCE
    for m in range(sd.D_TRY.get(c["N"], 0)):
        assert sd.clearance(sd.random_case(c["N"], fast=c["fast"], m=m)) < sd.CLEARANCE
    X, U = dc.guess(c)
    plain = dq.solve_equality(dq.assemble(dc.chain_of(c), c["cfg"], X, U, c["xhat"], c["yref"]))
    assert np.abs(sd.dense_solution(c)["dU"][0] - plain["dU"][0]).max() >= 0.05


def test_dense_reference_is_the_model_with_the_effective_input():
    """dense_qp_dist against first principles, without dense_qp's assembly of b and g: the defect is that of the model stepped with
    u + d, the residual's acceleration rows are the model's (qdot+ - qdot) / dt, the Hessians are dense_qp's untouched, and d = 0
    is dense_qp bit for bit."""
    c = BY_ID["N7-rand-dist"]
    cfg, chain, d = c["cfg"], dc.chain_of(c), c["d"]
    rng = np.random.default_rng(5)
    X, U = dc.guess(c)
    X = X + rng.uniform(-0.05, 0.05, X.shape)
    U = U + rng.uniform(-0.3, 0.3, U.shape)
    A, B = dq.lti(cfg["wcv"], cfg["dt"])
    qp, q0 = dd.assemble(chain, cfg, X, U, c["xhat"], d), dq.assemble(chain, cfg, X, U, c["xhat"])
    np.testing.assert_array_equal(qp.H, q0.H)
    W = dq.weights(cfg)
    for k in range(c["N"]):
        xn = A @ X[k] + B @ (U[k] + d)
        np.testing.assert_allclose(qp.b[k], xn - X[k + 1], rtol=0, atol=1e-15)
        r, Jr = dq.stage_residual(chain, cfg, X[k], U[k])
        r[11:] = (xn[6:] - X[k, 6:]) / cfg["dt"]
        np.testing.assert_allclose(qp.g[k], cfg["dt"] * Jr.T @ (W * r), rtol=0, atol=1e-12 * np.abs(qp.g[k]).max())
    z = dd.assemble(chain, cfg, X, U, c["xhat"], np.zeros(6))
    np.testing.assert_array_equal(z.g, q0.g)
    np.testing.assert_array_equal(z.b, q0.b)
    assert dd.nlp_cost(chain, cfg, X, U, np.zeros(6)) == dq.nlp_cost(chain, cfg, X, U)


@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_oracle_qp_solvers_against_dense(orc, cid):
    """orc.qp_fast / orc.qp_ipm on the oracle's assembly with the two changes of the disturbed model against the dense solve /
    certificate: the measured distance stays within the derived bound of its own committed value."""
    case = BY_ID[cid]
    o = sd.oracle_solution(orc, case)
    assert o["status"] == 0 and o["accepted"] == (case["fast"] and not case["active"])
    dist, sol = sd.distance(case, o["dX"], o["dU"])
    print(f"\n[dist] {cid}: |oracle - dense| = {dist:.2e}, LU vs refined = {sol['lu_vs_refined']:.1e}, iters {o['iters']}")
    assert dist <= sd.tolerance(ORACLE_VS_DENSE_DIST, cid)
    assert sol["lu_vs_refined"] <= 1e-11


# (case, wavefronts, chunk pool in doubles, the sweep family it must take): the triples of tests/test_terminal_cases.py EMULATED at
# the horizons of these cases -- every case once, and the resident, segment, register and streaming sweeps
EMULATED = [
    ("N1-rand-dist", 1, 19392, "resident"), ("N2-rand-dist", 2, 19392, "resident"), ("N3-rand-dist", 8, 19392, "resident"),
    ("N7-rand-dist", 4, 9152, "resident"), ("N20-rand-dist", 4, 19392, "resident"), ("N20-rand-dist-ipm", 8, 19392, "resident"),
    ("N80-rand-dist", 8, 19392, "resident"), ("N126-rand-dist", 8, 19392, "segment"), ("N130-rand-dist", 4, 19392, "segment"),
    ("N245-rand-dist", 8, 19392, "segment"), ("N130-rand-dist-ipm", 4, 19392, "segment"),
    ("N141-rand-dist", 1, 19392, "streaming"), ("N43-rand-dist", 1, 9152, "streaming"), ("N38-rand-dist", 2, 9152, "streaming"),
    ("N130-rand-dist-ipm", 2, 9152, "streaming"),
    ("N25-rand-dist", 4, 9152, "resident"), ("N37-rand-dist", 2, 9152, "resident"), ("N42-rand-dist", 1, 9152, "resident"),
    ("N125-rand-dist", 8, 19392, "resident"), ("N135-rand-dist", 2, 19392, "resident"), ("N136-rand-dist", 2, 19392, "segment"),
    ("N140-rand-dist", 1, 19392, "resident"),
    ("N26-rand-dist", 4, 9152, "register"), ("N130-rand-dist", 8, 9152, "register"), ("N246-rand-dist", 4, 9152, "register"),
    ("N130-rand-dist-ipm", 8, 9152, "register"),
    ("N20-tight-dist", 4, 19392, "resident"), ("N20-tight-dist-ipm", 4, 9152, "resident"),
]


def emulated(case, waves, pool):
    import emu_dist

    ctl = emu_dist.Controller([case["cfg"]], dc.chain_of(case), pool_doubles=pool, waves=waves)
    ctl.set_dist(case["d"][None])
    return ctl


def check_step(case, out, i, tag, rtol_cost=1e-10):
    """One simulation of a reset step's output against the dense disturbed QP of its case and the cost at the returned iterate."""
    N = case["N"]
    X, U = dc.guess(case)
    xp, up = out["x_pred"][i][:N + 1], out["u_pred"][i][:N]
    assert np.isfinite(xp).all() and np.isfinite(up).all() and out["status"][i] == 0, (case["id"], out["status"][i])
    assert (out["qp_iter"][i] == 1) == (case["fast"] and not case["active"]), (case["id"], out["qp_iter"][i])
    dist, _ = sd.distance(case, xp - X, up - U)
    bound = sd.tolerance(ORACLE_VS_DENSE_DIST, case["id"])
    print(f"\n[dist] {tag} {case['id']}: distance from dense = {dist:.2e} (bound {bound:.1e})")
    assert dist <= bound, (tag, case["id"], dist)
    np.testing.assert_array_equal(out["u0"][i], up[0])
    want = dd.nlp_cost(dc.chain_of(case), case["cfg"], xp, up, case["d"], case["yref"])
    np.testing.assert_allclose(out["cost"][i], want, rtol=rtol_cost, atol=0, err_msg=case["id"])
    return dist


def test_emulated_list_covers_every_case_and_sweep():
    assert {e[0] for e in EMULATED} == set(BY_ID)
    assert {e[3] for e in EMULATED} == {"resident", "segment", "register", "streaming"}


@needs_hipcc
@pytest.mark.parametrize("cid,waves,pool,sweep", EMULATED, ids=["%s-w%d-p%d-%s" % e for e in EMULATED])
def test_emulated_latency_engine_against_dense(cid, waves, pool, sweep):
    """Engine<.., 0, DIST>::control_step on the host: one reset step of SQP_RTI with the disturbance in the model, minus the initial
    guess, is the solution of the disturbed QP; u0 is the first predicted input; cost is the NLP cost of the disturbed model at the
    returned iterate; the returned iterate satisfies the disturbed dynamics (the eq residual) to rounding."""
    import emu

    case = BY_ID[cid]
    assert emu.emu_paths(case["N"], pool, waves)["sweep"] == sweep
    out = emulated(case, waves, pool).step(case["xhat"][None])
    check_step(case, out, 0, "emu-w%d-p%d" % (waves, pool))
    assert out["residuals"][0][1] <= 1e-12, out["residuals"][0]


@needs_hipcc
def test_emulated_zero_disturbance_is_the_plain_step_relinearised():
    """d = 0 through the DIST engine equals, bit for bit (the harness is built with -ffp-contract=off), the plain step that is made
    to linearise again every step as a changed disturbance does: reset and carried, fast path and interior point."""
    import emu_dist

    for N, fast in ((20, True), (20, False), (7, True)):
        base = dc.random_case(N, dc.SEEDS[N], fast=fast)
        a = emu_dist.Controller([base["cfg"]], dc.chain_of(base), pool_doubles=19392, waves=4)
        b = emu_dist.Controller([base["cfg"]], dc.chain_of(base), pool_doubles=19392, waves=4)
        x = base["xhat"]
        for _ in range(3):
            oa = a.step(x[None], ref_changed=True)
            ob = b.step(x[None], dist=np.zeros((1, 6)))
            for k in ("u0", "x_pred", "u_pred", "cost", "qp_iter", "residuals", "status"):
                np.testing.assert_array_equal(oa[k], ob[k], err_msg=k)
            x = x + 1e-3


# |oracle - dense| on the QPs of the three chained steps of CHAINED_CASE (carried; shifted from the second step on), measured by
# test_emulated_chained_steps_against_dense; the bound of a step is 10 x its entry, floor 1e-12
CHAINED_ORACLE_VS_DENSE_DIST = {False: (7.44e-15, 3.83e-15, 1.28e-15), True: (7.44e-15, 8.33e-15, 6.66e-16)}


def chained_tolerance(shift, k):
    return max(10.0 * CHAINED_ORACLE_VS_DENSE_DIST[shift][k], 1e-12)


@needs_hipcc
@pytest.mark.parametrize("shift", [False, True], ids=["carry", "shift"])
def test_emulated_chained_steps_against_dense(orc, shift):
    """Three chained steps on the off-model plant with a different disturbance each step: each step is certified against the dense
    disturbed QP assembled at the iterate it started from (the shifted one built with Bd (u_{N-1} + d)); its bound is 10 x the
    oracle's distance on that same QP, which is computed here and must match the committed tuple the device test uses."""
    case = BY_ID[sd.CHAINED_CASE]
    ctl = emulated(case, 4, 19392)

    def step(x, sh, d):
        out = ctl.step(x[None], warm=np.array([2 if sh else 0], np.int32), dist=d[None])
        assert out["status"][0] == 0
        return out["x_pred"][0], out["u_pred"][0]

    d, ora = sd.chained(case, step, orc=orc, shift=shift)
    print(f"\n[dist] chained {'shift' if shift else 'carry'}: |emulated - dense| = {d}, |oracle - dense| = {ora}")
    for k in range(sd.CHAINED_STEPS):
        assert ora[k] <= chained_tolerance(shift, k)          # the committed tuple still bounds the oracle's own distance
        assert d[k] <= max(10.0 * ora[k], 1e-12) and d[k] <= chained_tolerance(shift, k), (k, d[k], ora[k])
