"""The joint-wise terminal cost of the controller step (mpcb_step_term) on the CPU: the cases of tests/terminal_cases.py, the oracle's
QP routines and the emulated latency engine (tests/emu/emu_term*) against the dense KKT reference of tests/dense_qp_terminal.py.

ORACLE_VS_DENSE_TERM is the committed record of how far the oracle's solution of every terminal QP lies from the dense one (and of
the dense solve's LU-vs-refined estimate); the bound of every engine-vs-dense comparison, here and in tests/test_gpu_terminal.py, is
10 x that distance, floor 1e-12, and stays <= 1e-9 (the rule of tests/test_dense_qp.py).  tests/tools/terminal_profile.py writes the
measured distances to profiles/step_terminal_distances.txt (TERMINAL_DUMP=<file> collects them).
"""
import json
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
import terminal_cases as tc  # noqa: E402

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

# case id -> (max |oracle - dense| over dX, dU; max |plain LU - refined| of the dense solve), measured on the CPU
ORACLE_VS_DENSE_TERM = {
    "N1-rand-term": (1.25e-16, 1.0e-15),
    "N2-rand-term": (2.50e-16, 9.0e-16),
    "N3-rand-term": (2.22e-16, 2.0e-15),
    "N7-rand-term": (3.68e-16, 4.3e-16),
    "N20-rand-term": (9.99e-16, 1.9e-15),
    "N25-rand-term": (4.44e-16, 9.6e-16),
    "N26-rand-term": (1.22e-15, 2.8e-15),
    "N37-rand-term": (8.88e-16, 1.3e-15),
    "N38-rand-term": (3.89e-15, 2.4e-15),
    "N42-rand-term": (9.99e-16, 2.2e-15),
    "N43-rand-term": (5.55e-16, 2.0e-15),
    "N80-rand-term": (8.88e-16, 1.3e-15),
    "N125-rand-term": (1.17e-13, 3.2e-14),
    "N126-rand-term": (1.73e-15, 8.3e-15),
    "N130-rand-term": (2.12e-14, 1.2e-14),
    "N135-rand-term": (3.22e-15, 1.2e-14),
    "N136-rand-term": (5.64e-14, 3.0e-14),
    "N140-rand-term": (8.03e-14, 1.2e-14),
    "N141-rand-term": (8.65e-14, 3.0e-14),
    "N246-rand-term": (5.18e-13, 6.5e-14),
    "N300-rand-term": (1.89e-15, 7.9e-15),
    "N20-rand-term-ipm": (4.72e-16, 1.9e-15),
    "N200-rand-term-ipm": (1.46e-14, 9.0e-15),
    "N20-tight-term": (6.11e-16, 6.7e-16),
    "N20-tight-term-ipm": (5.01e-14, 6.7e-16),
    "N20-tight-far-term": (6.66e-16, 5.9e-15),
    "N20-tight-far-term-ipm": (6.66e-16, 5.9e-15),
}
N_CASES = 27

CASES = tc.all_cases()
BY_ID = tc.by_id()

_MEASURED = {}


def record(cid, tag, dist):
    _MEASURED.setdefault(cid, {})
    _MEASURED[cid][tag] = max(dist, _MEASURED[cid].get(tag, 0.0))
    if os.environ.get("TERMINAL_DUMP"):
        with open(os.environ["TERMINAL_DUMP"], "w") as f:
            json.dump(_MEASURED, f, indent=1, sort_keys=True)


def test_case_list_is_complete():
    assert len(CASES) == N_CASES and sorted(ORACLE_VS_DENSE_TERM) == sorted(BY_ID)
    for N in (1, 2, 3, 7, 20, 25, 26, 37, 38, 42, 43, 80, 125, 126, 130, 135, 136, 140, 141, 246, 300):
        assert BY_ID[f"N{N}-rand-term"]["fast"]
    for N in (20, 200):
        assert not BY_ID[f"N{N}-rand-term-ipm"]["fast"]
    for cid in ("N20-tight-term", "N20-tight-term-ipm", "N20-tight-far-term", "N20-tight-far-term-ipm"):
        assert BY_ID[cid]["certify"]
    assert max(tc.tolerance(ORACLE_VS_DENSE_TERM, cid) for cid in BY_ID) <= 1e-9
    for c in CASES:
        assert c["term"].shape == (30,) and np.isfinite(c["term"]).all()
        np.testing.assert_array_equal(dqt.blocks_to_matrix(c["blocks"]), c["P"])
        b = c["blocks"]
        assert (b[:, 0] > 0).all() and (b[:, 2] > 0).all() and (b[:, 0] * b[:, 2] > b[:, 1] ** 2).all()


@pytest.mark.parametrize("cid", [c["id"] for c in CASES if not c["active"]])
def test_inactive_minimisers_clear_every_bound(cid):
    """From the dense solution alone: the bound-free minimiser of every inactive terminal QP is >= 0.05 inside every bound (the x_e
    seed rule of tests/terminal_cases.py), and the terminal cost moves u0 by >= 1e-3, a million times the largest bound of these tests
    (1e-9; the short horizons move it by 0.08 .. 0.45, N = 136 and 140 by 0.02 .. 0.03) -- a missing terminal term cannot hide."""
    c = BY_ID[cid]
    assert tc.clearance(c) >= tc.CLEARANCE
    X, U = dc.guess(c)
    plain = dq.solve_equality(dq.assemble(dc.chain_of(c), c["cfg"], X, U, c["xhat"], c["yref"]))
    assert np.abs(tc.dense_solution(c)["dU"][0] - plain["dU"][0]).max() >= 1e-3


@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_oracle_qp_solvers_against_dense(orc, cid):
    """orc.qp_fast / orc.qp_ipm on the oracle's assembly plus the terminal block against the dense solve / certificate: the
    measured distance stays within the derived bound of its own committed value."""
    case = BY_ID[cid]
    o = tc.oracle_solution(orc, case)
    assert o["status"] == 0 and o["accepted"] == (case["fast"] and not case["active"])
    dist, sol = tc.distance(case, o["dX"], o["dU"])
    print(f"\n[terminal] {cid}: |oracle - dense| = {dist:.2e}, LU vs refined = {sol['lu_vs_refined']:.1e}, iters {o['iters']}")
    record(cid, "oracle", dist)
    assert dist <= tc.tolerance(ORACLE_VS_DENSE_TERM, cid)
    assert sol["lu_vs_refined"] <= 1e-11


# (case, wavefronts, chunk pool in doubles, the sweep family it must take): the triples of tests/test_dense_qp.py EMULATED at the
# horizons of the terminal cases -- every case once, and the resident, segment, register and streaming sweeps
EMULATED = [
    ("N1-rand-term", 1, 19392, "resident"), ("N2-rand-term", 2, 19392, "resident"), ("N3-rand-term", 8, 19392, "resident"),
    ("N7-rand-term", 4, 9152, "resident"), ("N20-rand-term", 4, 19392, "resident"), ("N20-rand-term-ipm", 8, 19392, "resident"),
    ("N80-rand-term", 8, 19392, "resident"), ("N126-rand-term", 8, 19392, "segment"), ("N130-rand-term", 4, 19392, "segment"),
    ("N300-rand-term", 8, 19392, "segment"), ("N200-rand-term-ipm", 4, 19392, "segment"),
    ("N141-rand-term", 1, 19392, "streaming"), ("N43-rand-term", 1, 9152, "streaming"), ("N38-rand-term", 2, 9152, "streaming"),
    ("N200-rand-term-ipm", 2, 9152, "streaming"),
    ("N25-rand-term", 4, 9152, "resident"), ("N37-rand-term", 2, 9152, "resident"), ("N42-rand-term", 1, 9152, "resident"),
    ("N125-rand-term", 8, 19392, "resident"), ("N135-rand-term", 2, 19392, "resident"), ("N136-rand-term", 2, 19392, "segment"),
    ("N140-rand-term", 1, 19392, "resident"),
    ("N26-rand-term", 4, 9152, "register"), ("N130-rand-term", 8, 9152, "register"), ("N246-rand-term", 4, 9152, "register"),
    ("N200-rand-term-ipm", 8, 9152, "register"),
    ("N20-tight-term", 4, 19392, "resident"), ("N20-tight-term-ipm", 4, 9152, "resident"),
    ("N20-tight-far-term", 4, 19392, "resident"), ("N20-tight-far-term-ipm", 2, 9152, "resident"),
]


def emulated(case, waves, pool):
    import emu_term

    ctl = emu_term.Controller([case["cfg"]], dc.chain_of(case), pool_doubles=pool, waves=waves)
    ctl.set_terminal(case["term"][None])
    return ctl


def check_step(case, out, i, tag, rtol_cost=1e-10):
    """One simulation of a reset step's output against the dense terminal QP of its case and the cost at the returned iterate."""
    N = case["N"]
    X, U = dc.guess(case)
    xp, up = out["x_pred"][i][:N + 1], out["u_pred"][i][:N]
    assert np.isfinite(xp).all() and np.isfinite(up).all() and out["status"][i] == 0, (case["id"], out["status"][i])
    assert (out["qp_iter"][i] == 1) == (case["fast"] and not case["active"]), (case["id"], out["qp_iter"][i])
    dist, _ = tc.distance(case, xp - X, up - U)
    bound = tc.tolerance(ORACLE_VS_DENSE_TERM, case["id"])
    print(f"\n[terminal] {tag} {case['id']}: distance from dense = {dist:.2e} (bound {bound:.1e})")
    record(case["id"], tag, dist)
    assert dist <= bound, (tag, case["id"], dist)
    np.testing.assert_array_equal(out["u0"][i], up[0])
    want = dqt.nlp_cost(dc.chain_of(case), case["cfg"], xp, up, case["P"], case["x_e"], case["yref"])
    np.testing.assert_allclose(out["cost"][i], want, rtol=rtol_cost, atol=0, err_msg=case["id"])
    return dist


def test_emulated_list_covers_every_case_and_sweep():
    assert {e[0] for e in EMULATED} == set(BY_ID)
    assert {e[3] for e in EMULATED} == {"resident", "segment", "register", "streaming"}


@needs_hipcc
@pytest.mark.parametrize("cid,waves,pool,sweep", EMULATED, ids=["%s-w%d-p%d-%s" % e for e in EMULATED])
def test_emulated_latency_engine_against_dense(cid, waves, pool, sweep):
    """Engine<.., TERM>::control_step on the host: one reset step of SQP_RTI with the terminal cost, minus the initial guess, is the
    solution of the terminal QP; u0 is the first predicted input; cost is the NLP cost plus l_N at the returned iterate."""
    import emu

    case = BY_ID[cid]
    assert emu.emu_paths(case["N"], pool, waves)["sweep"] == sweep
    out = emulated(case, waves, pool).step(case["xhat"][None])
    check_step(case, out, 0, "emu-w%d-p%d" % (waves, pool))


@needs_hipcc
def test_emulated_zero_terminal_is_no_terminal():
    """All-zero blocks with an arbitrary reference: bit for bit the step without a terminal cost, reset and carried."""
    import emu_term

    base = dc.random_case(20, dc.SEEDS[20])
    a = emu_term.Controller([base["cfg"]], dc.chain_of(base), pool_doubles=19392, waves=4)
    b = emu_term.Controller([base["cfg"]], dc.chain_of(base), pool_doubles=19392, waves=4)
    b.set_terminal(np.concatenate([np.zeros(18), np.linspace(-3.0, 4.0, 12)])[None])
    x = base["xhat"]
    for _ in range(3):
        oa, ob = a.step(x[None]), b.step(x[None])
        for k in ("u0", "x_pred", "u_pred", "cost", "qp_iter", "residuals"):
            np.testing.assert_array_equal(oa[k], ob[k], err_msg=k)
        x = x + 1e-3


# |oracle - dense| on the QPs of the three chained steps of CHAINED_CASE (carried; shifted from the second step on), measured by
# test_emulated_chained_steps_against_dense; the bound of a step is 10 x its entry, floor 1e-12
CHAINED_ORACLE_VS_DENSE_TERM = {False: (9.99e-16, 3.19e-16, 1.94e-16), True: (9.99e-16, 1.67e-16, 1.39e-16)}


def chained_tolerance(shift, k):
    return max(10.0 * CHAINED_ORACLE_VS_DENSE_TERM[shift][k], 1e-12)


@needs_hipcc
@pytest.mark.parametrize("shift", [False, True], ids=["carry", "shift"])
def test_emulated_chained_steps_against_dense(orc, shift):
    """Three chained steps on the off-model plant with the terminal cost in force: each step is certified against the dense
    terminal QP assembled at the iterate it started from; its bound is 10 x the oracle's distance on that same QP, which is
    computed here and must match the committed tuple the device test uses."""
    case = BY_ID[tc.CHAINED_CASE]
    ctl = emulated(case, 4, 19392)

    def step(x, sh):
        out = ctl.step(x[None], warm=np.array([2 if sh else 0], np.int32))
        assert out["status"][0] == 0
        return out["x_pred"][0], out["u_pred"][0]

    d, ora = tc.chained(case, step, orc=orc, shift=shift)
    print(f"\n[terminal] chained {'shift' if shift else 'carry'}: |emulated - dense| = {d}, |oracle - dense| = {ora}")
    for k in range(tc.CHAINED_STEPS):
        record("chained-%s-step%d" % ("shift" if shift else "carry", k), "emu", d[k])
        record("chained-%s-step%d" % ("shift" if shift else "carry", k), "oracle", ora[k])
        assert ora[k] <= chained_tolerance(shift, k)          # the committed tuple still bounds the oracle's own distance
        assert d[k] <= max(10.0 * ora[k], 1e-12) and d[k] <= chained_tolerance(shift, k), (k, d[k], ora[k])
