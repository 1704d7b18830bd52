"""Host emulation of the controller step over a scheduled, stage-varying surface (Engine<.., 0, 0, 1>::control_step, the device code
behind mpcb_step_surf on the latency engine) against the dense reference with per-stage coefficients (tests/dense_qp_surf.py), in
all four sweep families; the constant window against the plain step relinearised; the f-shift equivalence -- f enters g1 alone, so a
window that varies only in f is the packed surface with yref[..., 0] lowered by the same amounts, the one stage-varying case that
has an exact equivalent in code that already existed; chained steps with a window that slides."""
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
import dense_qp_surf as ds  # noqa: E402
import step_surf_cases as ss  # noqa: E402
import test_step_dist_cases as tsd  # noqa: E402  (the chained steps' bounds: the committed tuples of the disturbed chain, same case)

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

BY_ID = ss.by_id()
# (case, wavefronts, chunk pool in doubles, the sweep family it must take)
EMULATED = [
    ("N1-rand-dist", 1, 19392, "resident"), ("N7-rand-dist", 4, 9152, "resident"), ("N20-rand-dist", 4, 19392, "resident"),
    ("N20-rand-dist-ipm", 8, 19392, "resident"), ("N20-tight-dist", 4, 19392, "resident"), ("N20-tight-dist-ipm", 2, 19392, "resident"),
    ("N26-rand-dist", 4, 9152, "register"), ("N126-rand-dist", 8, 19392, "segment"), ("N43-rand-dist", 1, 9152, "streaming"),
]


def emulated(case, waves, pool):
    import emu_surf

    return emu_surf.Controller([case["cfg"]], dc.chain_of(case), pool_doubles=pool, waves=waves)


def test_dense_reference_with_a_constant_window_is_the_dense_reference():
    case = BY_ID["N7-rand-dist"]
    X, U = dc.guess(case)
    rng = np.random.default_rng(3)
    X, U = X + rng.normal(size=X.shape) * 1e-2, U + rng.normal(size=U.shape) * 1e-2
    chain, cfg = dc.chain_of(case), case["cfg"]
    a = dq.assemble(chain, cfg, X, U, case["xhat"])
    b = ds.assemble(chain, cfg, X, U, case["xhat"], np.tile(cfg["coeffs"], (7, 1)))
    for k in ("H", "g", "b"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    assert ds.nlp_cost(chain, cfg, X, U, np.tile(cfg["coeffs"], (7, 1))) == pytest.approx(dq.nlp_cost(chain, cfg, X, U), rel=1e-14)
    # and the window changes H_k, g_k and the cost
    c = ds.assemble(chain, cfg, X, U, case["xhat"], case["surf"])
    assert np.abs(c.H - a.H).max() > 1e-4 and np.abs(c.g - a.g).max() > 1e-5
    assert abs(ds.nlp_cost(chain, cfg, X, U, case["surf"]) - dq.nlp_cost(chain, cfg, X, U)) > 1e-6
    np.testing.assert_array_equal(c.b, a.b)


def test_case_table_is_complete_and_bounds_the_oracle(orc):
    assert sorted(ss.ORACLE_VS_DENSE_SURF) == sorted(BY_ID)
    assert max(ss.tolerance(ss.ORACLE_VS_DENSE_SURF, cid) for cid in BY_ID) <= 1e-9
    for cid in ("N7-rand-dist", "N20-rand-dist", "N20-rand-dist-ipm", "N20-tight-dist", "N26-rand-dist", "N43-rand-dist"):
        o = ss.oracle_solution(orc, BY_ID[cid])
        assert o["status"] == 0 and o["accepted"] == (BY_ID[cid]["fast"] and not BY_ID[cid]["active"])
        d, _ = ss.distance(BY_ID[cid], o["dX"], o["dU"])
        assert d <= ss.tolerance(ss.ORACLE_VS_DENSE_SURF, cid), (cid, d)


def test_windows_vary_curvature_and_slope():
    for c in ss.all_cases():
        if c["N"] < 7:
            continue
        v = c["surf"] - c["cfg"]["coeffs"]
        assert (np.ptp(v[:, :3], axis=0) > 1e-3).all() and (np.ptp(v[:, 3:5], axis=0) > 1e-3).all(), c["id"]
        assert (np.abs(v) <= ss.AMP).all()


@pytest.mark.parametrize("cid,waves,pool,sweep", EMULATED, ids=["%s-w%d-p%d-%s" % e for e in EMULATED])
def test_emulated_step_with_a_window_against_dense(cid, waves, pool, sweep):
    import emu

    case = BY_ID[cid]
    assert emu.emu_paths(case["N"], pool, waves)["sweep"] == sweep
    ctl = emulated(case, waves, pool)
    out = ctl.step(case["xhat"][None], surface=case["surf"][None])
    ss.check_step(case, out, 0, "emu-w%d-p%d" % (waves, pool))
    # the window matters: the step on the packed surface lies elsewhere
    plain = emulated(case, waves, pool).step(case["xhat"][None])
    assert np.abs(plain["u_pred"] - out["u_pred"]).max() > 1e-5 or case["N"] == 1


@pytest.mark.parametrize("N", [20, 130])
def test_constant_window_is_the_plain_step_relinearised(N):
    """The packed coefficients on every row, set again every step, against the plain step given yref = the packed row every step,
    so that both linearise again: one reset step and two carried ones at rtol 1e-12, qp_iter equal."""
    c = BY_ID["N%d-rand-dist" % N]
    cfg = c["cfg"]
    xs = [c["xhat"] + 1e-3 * k for k in range(3)]
    yref = np.tile(dq.packed_reference(cfg), (1, N, 1))
    plain, const = emulated(c, 4, 19392), emulated(c, 4, 19392)
    for x in xs:
        w = plain.step(x[None], yref=yref, ref_changed=True)
        g = const.step(x[None], surface=np.tile(cfg["coeffs"], (1, N, 1)))
        np.testing.assert_array_equal(g["qp_iter"], w["qp_iter"])
        for k in ("u0", "x_pred", "u_pred", "cost"):
            np.testing.assert_allclose(g[k], w[k], rtol=1e-12, atol=1e-12 * np.abs(w[k]).max(), err_msg=k)


@pytest.mark.parametrize("N,waves", [(20, 4), (130, 8)])
def test_f_shift_equivalence(N, waves):
    """A window that varies only in f against the packed surface with yref[..., 0] lowered... g1 = S - Z carries f additively, so
    g1(f_k) - y0 = g1(f) - (y0 - (f_k - f)): the same residuals, Jacobians, QP and cost.  rtol 1e-12; a different shift per step."""
    c = BY_ID["N%d-rand-dist" % N]
    cfg = c["cfg"]
    a, b = emulated(c, waves, 19392), emulated(c, waves, 19392)
    for k in range(3):
        x = (c["xhat"] + 1e-3 * k)[None]
        df = 0.01 * np.sin(0.3 * (np.arange(N) + k) + 0.5)
        surf = np.tile(cfg["coeffs"], (N, 1))
        surf[:, 5] += df
        yref = np.tile(dq.packed_reference(cfg), (N, 1))
        yref[:, 0] -= df
        ga = a.step(x, surface=surf[None])
        gb = b.step(x, yref=yref[None], ref_changed=True)
        assert ga["status"][0] == 0
        np.testing.assert_array_equal(ga["qp_iter"], gb["qp_iter"])
        for key in ("u0", "x_pred", "u_pred", "cost"):
            np.testing.assert_allclose(ga[key], gb[key], rtol=1e-12, atol=1e-12 * np.abs(gb[key]).max(), err_msg=key)
    # (and the shift is not nothing)
    plain = emulated(c, waves, 19392).step(c["xhat"][None])
    first = emulated(c, waves, 19392).step(c["xhat"][None], surface=(np.tile(cfg["coeffs"], (N, 1)) + np.outer(0.01 * np.sin(0.3 * np.arange(N) + 0.5), np.eye(6)[5]))[None])
    assert np.abs(plain["u_pred"] - first["u_pred"]).max() > 1e-5


@pytest.mark.parametrize("shift", [False, True], ids=["carry", "shift"])
def test_emulated_chained_steps_against_dense(shift):
    """Three chained steps on the off-model plant with a window that slides one row per step, carried and shifted: each step is
    certified against the dense QP assembled at the iterate it started from on that step's window."""
    case = BY_ID[ss.CHAINED_CASE]
    ctl = emulated(case, 4, 19392)

    def step(x, sh, w):
        out = ctl.step(x[None], warm=np.array([2 if sh else 0], np.int32), surface=w[None])
        assert out["status"][0] == 0
        return out["x_pred"][0], out["u_pred"][0]

    d = ss.chained(case, step, shift=shift)
    print(f"\n[surf] chained {'shift' if shift else 'carry'}: |emulated - dense| = {d}")
    for k in range(ss.CHAINED_STEPS):
        assert d[k] <= tsd.chained_tolerance(shift, k), (k, d[k])


def test_switching_the_window_off_linearises_again():
    """surface=None after a window: the step is the plain one from a fresh linearisation (the emulated surf_changed)."""
    c = BY_ID["N20-rand-dist"]
    N = 20
    a, b = emulated(c, 4, 19392), emulated(c, 4, 19392)
    yref = np.tile(dq.packed_reference(c["cfg"]), (1, N, 1))
    x0, x1 = c["xhat"][None], (c["xhat"] + 1e-3)[None]
    ga = a.step(x0, surface=c["surf"][None])
    gb = b.step(x0, surface=c["surf"][None])
    np.testing.assert_array_equal(ga["u_pred"], gb["u_pred"])
    ga = a.step(x1, surface=None)
    gb = b.step(x1, surface=np.tile(c["cfg"]["coeffs"], (1, N, 1)))
    for key in ("u0", "x_pred", "u_pred", "cost"):
        np.testing.assert_allclose(ga[key], gb[key], rtol=1e-12, atol=1e-12 * np.abs(gb[key]).max(), err_msg=key)
    del yref
