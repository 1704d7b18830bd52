"""The cases of the combined-step tests (tests/test_emulation_step_combined.py on the CPU, tests/test_gpu_step_combined.py on the
device): the reset step of a step_dist_cases case -- the same horizons, feedback states, fast-path settings and bounds -- WITH its
input disturbance d AND the surface window of step_surf_cases.window AND an LQR terminal block set (terminal.lqr_terminal: q 10,
qdot 1, r 1) around a terminal reference x_e off the iterate, against the dense reference of tests/dense_qp_combined.py.

x_e = X_N of the initial guess + a seeded offset, uniform +-XE_AMP_Q on q and +-XE_AMP_V on qdot, seed 1300 + N.  With that first
draw the dense minimiser of every case but N = 135 clears every bound by CLEARANCE; N = 135 is an active case (TERM_ACTIVE).

ORACLE_VS_DENSE_COMBINED is the committed record of how far the oracle's QP routines, given the matrices of the dense assembly (its
QP solvers take any OCP-QP), land from the dense solution of every case: the reference solver's own error on that QP.  The bound of
every engine-vs-dense comparison is 10 x that distance, floor 1e-12, and stays <= 1e-9 (the rule of tests/test_dense_qp.py).
"""
import numpy as np

import dense_qp as dq
import dense_qp_cases as dc
import dense_qp_combined as dcomb
import step_dist_cases as sd
import step_surf_cases as ss

# case id -> max |oracle - dense| over dX, dU, measured on the CPU (tests/test_emulation_step_combined.py re-measures a sample)
ORACLE_VS_DENSE_COMBINED = {
    "N1-rand-comb": 1.11e-16, "N2-rand-comb": 1.11e-16, "N3-rand-comb": 1.67e-16, "N7-rand-comb": 3.33e-16,
    "N20-rand-comb": 9.99e-16, "N25-rand-comb": 7.22e-16, "N26-rand-comb": 1.11e-15, "N37-rand-comb": 7.77e-16,
    "N38-rand-comb": 9.99e-16, "N42-rand-comb": 1.22e-15, "N43-rand-comb": 5.55e-16, "N80-rand-comb": 8.05e-16,
    "N125-rand-comb": 1.40e-14, "N126-rand-comb": 5.90e-15, "N130-rand-comb": 2.69e-14, "N135-rand-comb": 7.99e-15,
    "N136-rand-comb": 2.84e-14, "N140-rand-comb": 2.66e-14, "N141-rand-comb": 3.47e-14, "N245-rand-comb": 2.82e-13,
    "N246-rand-comb": 6.69e-14, "N20-rand-comb-ipm": 1.72e-14, "N130-rand-comb-ipm": 1.48e-11, "N20-tight-comb": 3.92e-11,
    "N20-tight-comb-ipm": 3.92e-11,
}
CLEARANCE = sd.CLEARANCE
XE_AMP_Q, XE_AMP_V = 0.05, 0.1
TIGHT_XE_SCALE = 10.0
# horizons at which the terminal cost drives an input bound active whatever the draw (the pull towards an x_e near the initial guess
# grows with the horizon's reach): those cases are ACTIVE ones, held to the exact active-set certificate like the tight-bounds cases
# (N = 135: the dense minimiser violates an input bound with every x_e tried -- seeds 1435 + 1000 m, m = 0 .. 7, clearance -0.26,
# -0.20, -0.78, -0.85, -0.90, -0.35, -0.30, -0.32 rad/s -- so the case keeps the first draw and is certified as an active one)
TERM_ACTIVE = (135,)
tolerance = ss.tolerance


def lqr_P(cfg):
    from robotic_mpc_amd import terminal

    return terminal._lqr(np.asarray(cfg["wcv"], float), float(cfg["dt"]), 10.0, 1.0, 1.0)


def x_e_of(base, seed, scale=1.0):
    X, _ = dc.guess(base)
    rng = np.random.default_rng(seed)
    return X[-1] + scale * np.concatenate([rng.uniform(-XE_AMP_Q, XE_AMP_Q, 6), rng.uniform(-XE_AMP_V, XE_AMP_V, 6)])


def _with_all(base):
    N = base["N"]
    lq = lqr_P(base["cfg"])
    seed = 1300 + N
    # (the tight-bounds cases start from rest: an x_e as close as the others' holds the arm still and no bound is active, so theirs
    # lies TIGHT_XE_SCALE times as far -- the terminal pull then asks for more than the 0.8 rad/s the bounds allow)
    scale = TIGHT_XE_SCALE if "tight" in base["id"] else 1.0
    out = dict(base, id=base["id"].replace("-dist", "-comb"), P=lq["P"], blocks=lq["blocks"], x_e=x_e_of(base, seed, scale), xe_seed=seed)
    if N in TERM_ACTIVE and not base["id"].endswith("-ipm"):
        out.update(active=True, certify=True)
    return out


_ALL = None


def all_cases():
    """step_surf_cases' cases (each a step_dist_cases case with its d and a window) with the terminal cost added."""
    global _ALL
    if _ALL is None:
        _ALL = [_with_all(c) for c in ss.all_cases()]
    return _ALL


def by_id():
    return {c["id"]: c for c in all_cases()}


def term_record(case):
    """[30] = pqq 6 | pqv 6 | pvv 6 | x_e 12, as mpcb_step_combined takes it."""
    b = case["blocks"]
    return np.concatenate([b[:, 0], b[:, 1], b[:, 2], case["x_e"]])


_QPS, _SOLS = {}, {}


def dense_qp(case):
    key = case["id"].replace("-ipm", "")
    if key not in _QPS:
        X, U = dc.guess(case)
        _QPS[key] = dcomb.assemble(dc.chain_of(case), case["cfg"], X, U, case["xhat"], case["surf"], case["d"], case["P"], case["x_e"],
                                   case["yref"])
    return _QPS[key]


def dense_solution(case):
    key = case["id"].replace("-ipm", "")
    if key not in _SOLS:
        _SOLS[key] = dq.solve_equality(dense_qp(case))
    return _SOLS[key]


def clearance(case):
    qp, sol = dense_qp(case), dense_solution(case)
    idx, lo, hi = qp.bounded()
    return float(np.minimum(sol["w"][idx] - lo, hi - sol["w"][idx]).min())


def distance(case, dX, dU):
    """(distance of a candidate QP step from the dense solution, the solve / certificate); an active case is held to its exact
    active-set certificate, an inactive one to the clearance of every bound."""
    qp = dense_qp(case)
    if case["certify"]:
        cert = dq.certify(qp, dX, dU)
        assert cert["n_active"] > 0 and cert["min_multiplier"] > 0 and cert["min_slack"] >= 1e-5, \
            (case["id"], {k: cert[k] for k in ("n_active", "min_multiplier", "min_slack")})
        assert cert["candidate_min_slack"] >= 1e-5, (case["id"], cert["candidate_min_slack"])
        return cert["distance"], cert
    assert not case["active"]
    sol = dense_solution(case)
    assert clearance(case) >= CLEARANCE, case["id"]
    return float(max(np.abs(sol["dX"] - dX).max(), np.abs(sol["dU"] - dU).max())), sol


def oracle_solution(orc, case):
    """The oracle's QP routines (orc.qp_fast where the case has the fast path on and it accepts, orc.qp_ipm at the case's qp_tol /
    iteration limit otherwise) on the matrices of the DENSE assembly."""
    cfg, N = case["cfg"], case["N"]
    qp = dense_qp(case)
    args = (qp.H, qp.g, qp.b, qp.A, qp.B, qp.lb, qp.ub, qp.dx0)
    q = orc.qp_fast(*args) if case["fast"] else dict(accepted=0)
    status = 0
    if not q["accepted"]:
        q = orc.qp_ipm(*args, tol=cfg["qp_tol"], iter_max=cfg["qp_iter_max"])
        status = q["status"]
    return dict(dX=q["w"][:, 6:], dU=q["w"][:N, :6], accepted=bool(q.get("accepted", 0)), status=status)


def oracle_distance(orc, case):
    o = oracle_solution(orc, case)
    assert o["status"] == 0, case["id"]
    return distance(case, o["dX"], o["dU"])[0]


def check_step(case, out, i, tag, rtol_cost=1e-10):
    """One simulation of a reset step's output against the dense QP of its case, and the cost at the returned iterate."""
    N = case["N"]
    X, U = dc.guess(case)
    xp, up = out["x_pred"][i][:N + 1], out["u_pred"][i][:N]
    assert np.isfinite(xp).all() and np.isfinite(up).all() and out["status"][i] == 0, (case["id"], out["status"][i])
    assert (out["qp_iter"][i] == 1) == (case["fast"] and not case["active"]), (case["id"], out["qp_iter"][i])
    dist, _ = distance(case, xp - X, up - U)
    bound = tolerance(ORACLE_VS_DENSE_COMBINED, case["id"])
    print(f"\n[combined] {tag} {case['id']}: distance from dense = {dist:.2e} (bound {bound:.1e})")
    assert dist <= bound, (tag, case["id"], dist)
    np.testing.assert_array_equal(out["u0"][i], up[0])
    want = dcomb.nlp_cost(dc.chain_of(case), case["cfg"], xp, up, case["surf"], case["d"], case["P"], case["x_e"], case["yref"])
    np.testing.assert_allclose(out["cost"][i], want, rtol=rtol_cost, atol=0, err_msg=case["id"])
    return dist


CHAINED_CASE, CHAINED_STEPS = "N20-rand-comb", 3
CHAINED_XE_SEED = 1350


def chained_x_e(case, k):
    return x_e_of(case, CHAINED_XE_SEED + k)


def chained(case, step, shift=False, orc=None):
    """Three chained steps without a reset on the off-model plant, carried or shifted, each with a NEW disturbance
    (step_dist_cases.chained_dist), a NEW window (step_surf_cases.chained_window: it slides) and a NEW x_e.
    `step(x, shift, surf, d, x_e)` -> (x_pred, u_pred) is the solver under test.  Step k minus the iterate it started from (the
    previous result, moved one stage when shifting, x_N propagated by the model with THIS step's disturbance: Ad x_N + Bd (u_{N-1} +
    d_k)) is certified against the dense QP assembled there.  Returns (the distances, the oracle's on the same QPs or None)."""
    cfg, chain = case["cfg"], dc.chain_of(case)
    A, B = dq.lti(cfg["wcv"], cfg["dt"])
    Ap, Bp = dq.lti(0.8 * np.asarray(cfg["wcv"]), cfg["dt"])
    rng = np.random.default_rng(77)
    x, prev, out, ora = case["xhat"].copy(), dc.guess(case), [], []
    for k in range(CHAINED_STEPS):
        d, w, xe = sd.chained_dist(k), ss.chained_window(case, k), chained_x_e(case, k)
        if shift and k > 0:
            Xs = np.vstack([prev[0][1:], (A @ prev[0][-1] + B @ (prev[1][-1] + d))[None]])
            Us = np.vstack([prev[1][1:], prev[1][-1:]])
            prev = (Xs, Us)
        xp, up = step(x, shift and k > 0, w, d, xe)
        qp = dcomb.assemble(chain, cfg, prev[0], prev[1], x, w, d, case["P"], xe, case["yref"])
        cert = dq.certify(qp, xp - prev[0], up - prev[1])
        assert cert["min_multiplier"] >= 0 and cert["min_slack"] >= 1e-5, cert
        out.append(cert["distance"])
        if orc is not None:
            q = orc.qp_fast(qp.H, qp.g, qp.b, qp.A, qp.B, qp.lb, qp.ub, qp.dx0)
            assert q["accepted"]
            ora.append(float(max(np.abs(cert["dX"] - q["w"][:, 6:]).max(), np.abs(cert["dU"] - q["w"][:case["N"], :6]).max())))
        prev = (xp.copy(), up.copy())
        x = Ap @ x + Bp @ (up[0] + d) + rng.uniform(-1e-3, 1e-3, 12)
    return out, (ora if orc is not None else None)
