"""Host emulation of the combined controller step (Engine<.., 1, 1, 1>::control_step<true>, the device code behind mpcb_step_combined
on the latency engine): terminal cost, input disturbance and surface window in one step, against the dense reference that composes
the three assemblies (tests/dense_qp_combined.py), in all four sweep families; three chained steps, carried and shifted, each with a
new d, a new window and a new x_e; and NEUTRALITY -- the combined step with exactly one feature live against the existing
single-feature emulated step, by the rule of test_constant_window_is_the_plain_step_relinearised: rtol 1e-12 and qp_iter equal."""
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
import dense_qp_combined as dcomb  # noqa: E402
import dense_qp_dist as dd  # noqa: E402
import dense_qp_surf as ds  # noqa: E402
import dense_qp_terminal as dterm  # noqa: E402
import step_combined_cases as sc  # noqa: E402
import step_dist_cases as sd  # noqa: E402
import step_surf_cases as ss  # noqa: E402

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

BY_ID = sc.by_id()
# (case, wavefronts, chunk pool in doubles, the sweep family it must take): test_emulation_step_surf.py's list
EMULATED = [
    ("N1-rand-comb", 1, 19392, "resident"), ("N2-rand-comb", 2, 19392, "resident"), ("N7-rand-comb", 4, 9152, "resident"),
    ("N20-rand-comb", 4, 19392, "resident"), ("N20-rand-comb-ipm", 8, 19392, "resident"), ("N20-tight-comb", 4, 19392, "resident"),
    ("N20-tight-comb-ipm", 2, 19392, "resident"), ("N26-rand-comb", 4, 9152, "register"), ("N126-rand-comb", 8, 19392, "segment"),
    ("N43-rand-comb", 1, 9152, "streaming"),
]
# the chained steps: max |oracle QP routines - dense certificate| on the three QPs of each chain, measured on the CPU with the
# emulated step's iterates (test_emulated_chained_steps_against_dense re-measures them); the bound of step k is 10 x that, floor 1e-12
CHAINED_ORACLE_VS_DENSE = {False: (8.60e-16, 5.27e-16, 6.66e-16), True: (8.60e-16, 5.00e-16, 5.27e-16)}


def chained_tolerance(shift, k):
    return max(10.0 * CHAINED_ORACLE_VS_DENSE[shift][k], 1e-12)


def emulated(case, waves, pool):
    import emu_combined

    return emu_combined.Controller([case["cfg"]], dc.chain_of(case), pool_doubles=pool, waves=waves)


def _step(ctl, case, **kw):
    return ctl.step(case["xhat"][None], term=sc.term_record(case)[None], dist=case["d"][None], surface=case["surf"][None], **kw)


# ------------------------------------------------------------------------------------------------------------ the dense reference
def test_dense_composition_reduces_to_each_single_assembly():
    """With two of the three neutral the composed assembly IS the third one's, entry for entry; with all three it differs from each."""
    case = BY_ID["N7-rand-comb"]
    X, U = dc.guess(case)
    rng = np.random.default_rng(3)
    X, U = X + rng.normal(size=X.shape) * 1e-2, U + rng.normal(size=U.shape) * 1e-2
    chain, cfg, x = dc.chain_of(case), case["cfg"], case["xhat"]
    flat, z6, P0 = np.tile(cfg["coeffs"], (7, 1)), np.zeros(6), np.zeros((12, 12))
    pairs = [(dcomb.assemble(chain, cfg, X, U, x, case["surf"], z6, P0, case["x_e"]), ds.assemble(chain, cfg, X, U, x, case["surf"])),
             (dcomb.assemble(chain, cfg, X, U, x, flat, case["d"], P0, case["x_e"]), dd.assemble(chain, cfg, X, U, x, case["d"])),
             (dcomb.assemble(chain, cfg, X, U, x, flat, z6, case["P"], case["x_e"]), dterm.assemble(chain, cfg, X, U, x, case["P"], case["x_e"])),
             (dcomb.assemble(chain, cfg, X, U, x, flat, z6, P0, case["x_e"]), dq.assemble(chain, cfg, X, U, x))]
    for a, b in pairs:
        for k in ("H", "g", "b"):
            np.testing.assert_allclose(getattr(a, k), getattr(b, k), rtol=0, atol=1e-15 * np.abs(getattr(b, k)).max(), err_msg=k)
    full = dcomb.assemble(chain, cfg, X, U, x, case["surf"], case["d"], case["P"], case["x_e"])
    for _, single in pairs:
        assert max(np.abs(full.H - single.H).max(), np.abs(full.g - single.g).max(), np.abs(full.b - single.b).max()) > 1e-5
    want = ds.nlp_cost(chain, cfg, X, U, flat) + dterm.terminal_cost(X, case["P"], case["x_e"])
    assert dcomb.nlp_cost(chain, cfg, X, U, flat, z6, case["P"], case["x_e"]) == pytest.approx(want, rel=1e-14)


def test_case_table_is_complete_and_bounds_the_oracle(orc):
    assert sorted(sc.ORACLE_VS_DENSE_COMBINED) == sorted(BY_ID)
    assert max(sc.ORACLE_VS_DENSE_COMBINED.values()) <= 1e-10
    assert max(sc.tolerance(sc.ORACLE_VS_DENSE_COMBINED, cid) for cid in BY_ID) <= 1e-9
    assert sorted({c["N"] for c in sc.all_cases()}) == sorted(sd.FAST_HORIZONS)
    for cid in ("N1-rand-comb", "N7-rand-comb", "N20-rand-comb", "N20-rand-comb-ipm", "N20-tight-comb", "N26-rand-comb", "N43-rand-comb"):
        o = sc.oracle_solution(orc, BY_ID[cid])
        assert o["status"] == 0 and o["accepted"] == (BY_ID[cid]["fast"] and not BY_ID[cid]["active"])
        d, _ = sc.distance(BY_ID[cid], o["dX"], o["dU"])
        print(f"\n[combined] oracle {cid}: {d:.2e}")
        assert d <= sc.tolerance(sc.ORACLE_VS_DENSE_COMBINED, cid), (cid, d)


def test_every_feature_moves_the_dense_solution():
    """No feature of a case is a passenger: the dense solution without it lies more than 1e-5 away (N >= 2; with N = 1 only the
    terminal cost and the disturbance can reach the one input)."""
    for cid in ("N1-rand-comb", "N7-rand-comb", "N20-rand-comb"):
        c = BY_ID[cid]
        X, U = dc.guess(c)
        chain, cfg, N = dc.chain_of(c), c["cfg"], c["N"]
        full = sc.dense_solution(c)["dU"]
        flat, z6, P0 = np.tile(cfg["coeffs"], (N, 1)), np.zeros(6), np.zeros((12, 12))
        for name, args in (("surf", (flat, c["d"], c["P"])), ("dist", (c["surf"], z6, c["P"])), ("term", (c["surf"], c["d"], P0))):
            other = dq.solve_equality(dcomb.assemble(chain, cfg, X, U, c["xhat"], *args, c["x_e"], c["yref"]))["dU"]
            if N == 1 and name == "surf":
                continue
            assert np.abs(other - full).max() > 1e-5, (cid, name)


# --------------------------------------------------------------------------------------------------------- the emulated reset step
@needs_hipcc
@pytest.mark.parametrize("cid,waves,pool,sweep", EMULATED, ids=["%s-w%d-p%d-%s" % e for e in EMULATED])
def test_emulated_combined_step_against_dense(cid, waves, pool, sweep):
    import emu

    case = BY_ID[cid]
    assert emu.emu_paths(case["N"], pool, waves)["sweep"] == sweep
    out = _step(emulated(case, waves, pool), case)
    sc.check_step(case, out, 0, "emu-w%d-p%d" % (waves, pool))


@needs_hipcc
def test_n1_the_terminal_cost_alone_couples_u0_to_x_e():
    """N = 1: the terminal cost sits on stage 1 and is the only thing that couples u0 to x_e -- moving x_e moves u0, and without the
    terminal cost x_e does nothing."""
    case = BY_ID["N1-rand-comb"]
    rec = sc.term_record(case)
    far = rec.copy()
    far[18:24] += 0.05
    a = emulated(case, 1, 19392).step(case["xhat"][None], term=rec[None], dist=case["d"][None], surface=case["surf"][None])
    b = emulated(case, 1, 19392).step(case["xhat"][None], term=far[None], dist=case["d"][None], surface=case["surf"][None])
    assert a["status"][0] == 0 and b["status"][0] == 0 and np.abs(a["u0"] - b["u0"]).max() > 1e-4
    zero, zfar = rec.copy(), far.copy()
    zero[:18] = zfar[:18] = 0.0
    c = emulated(case, 1, 19392).step(case["xhat"][None], term=zero[None], dist=case["d"][None], surface=case["surf"][None])
    d = emulated(case, 1, 19392).step(case["xhat"][None], term=zfar[None], dist=case["d"][None], surface=case["surf"][None])
    np.testing.assert_array_equal(c["u0"], d["u0"])


# ------------------------------------------------------------------------------------------------------------------ chained steps
def _chain(shift, orc=None):
    case = BY_ID[sc.CHAINED_CASE]
    ctl = emulated(case, 4, 19392)

    def step(x, sh, w, d, xe):
        rec = np.concatenate([sc.term_record(case)[:18], xe])
        out = ctl.step(x[None], warm=np.array([2 if sh else 0], np.int32), term=rec[None], dist=d[None], surface=w[None])
        assert out["status"][0] == 0
        return out["x_pred"][0], out["u_pred"][0]

    return sc.chained(case, step, shift=shift, orc=orc)


@needs_hipcc
@pytest.mark.parametrize("shift", [False, True], ids=["carry", "shift"])
def test_emulated_chained_steps_against_dense(orc, shift):
    """Each step is certified against the dense QP assembled at the iterate it started from; the shifted iterate is built with
    Bd (u_{N-1} + d_t), THIS step's disturbance.  The bound of step k is 10 x the oracle's distance on that same QP, which is
    computed here and must be covered by the committed tuple the device test uses."""
    d, ora = _chain(shift, orc)
    print(f"\n[combined] chained {'shift' if shift else 'carry'}: |emulated - dense| = {d}, |oracle - dense| = {ora}")
    for k in range(sc.CHAINED_STEPS):
        assert ora[k] <= 2.0 * CHAINED_ORACLE_VS_DENSE[shift][k] + 1e-16, (k, ora[k])     # (the committed figure is the oracle's)
        assert d[k] <= chained_tolerance(shift, k), (k, d[k])


# --------------------------------------------------------------------------------------------------------------------- neutrality
def _close(g, w):
    np.testing.assert_array_equal(g["qp_iter"], w["qp_iter"])
    np.testing.assert_array_equal(g["status"], w["status"])
    for k in ("u0", "x_pred", "u_pred", "cost"):
        np.testing.assert_allclose(g[k], w[k], rtol=1e-12, atol=1e-12 * np.abs(w[k]).max(), err_msg=k)


@needs_hipcc
@pytest.mark.parametrize("feature", ["term", "dist", "surf", "shift", "none"])
@pytest.mark.parametrize("cid,waves", [("N20-rand-comb", 4), ("N130-rand-comb", 8)])
def test_one_live_feature_is_the_single_feature_step(cid, waves, feature):
    """The combined step with the other features neutral (zero blocks, d = 0, the packed a..f on every row, carry) against the
    existing emulated step of that one feature: a reset step and two more (shifted where the feature is the shift) from states that
    move, everything set again every step so that both sides linearise again."""
    import emu_dist
    import emu_surf
    import emu_term
    import emu_warm

    c = BY_ID[cid]
    cfg, chain, N = c["cfg"], dc.chain_of(c), c["N"]
    comb = emulated(c, waves, 19392)
    xs = [c["xhat"] + 1e-3 * k for k in range(3)]
    yref = np.tile(dq.packed_reference(cfg), (1, N, 1))
    rec = sc.term_record(c)
    if feature == "term":
        one = emu_term.Controller([cfg], chain, pool_doubles=19392, waves=waves)
    elif feature == "dist":
        one = emu_dist.Controller([cfg], chain, pool_doubles=19392, waves=waves)
    elif feature == "surf":
        one = emu_surf.Controller([cfg], chain, pool_doubles=19392, waves=waves)
    else:
        one = emu_warm.Controller([cfg], chain, pool_doubles=19392, waves=waves)
    for k, x in enumerate(xs):
        warm = np.array([2 if (feature == "shift" and k > 0) else 0], np.int32)
        g = comb.step(x[None], yref=yref, ref_changed=True, warm=warm, term=rec[None] if feature == "term" else None,
                      dist=c["d"][None] if feature == "dist" else None, surface=c["surf"][None] if feature == "surf" else None)
        if feature == "term":
            one.set_terminal(rec[None])
            w = one.step(x[None], yref=yref, ref_changed=True, warm=warm)
        elif feature == "dist":
            w = one.step(x[None], yref=yref, ref_changed=True, warm=warm, dist=c["d"][None])
        elif feature == "surf":
            w = one.step(x[None], yref=yref, ref_changed=True, warm=warm, surface=c["surf"][None])
        else:
            w = one.step(x[None], yref=yref, ref_changed=True, warm=warm)
        assert w["status"][0] == 0
        _close(g, w)
