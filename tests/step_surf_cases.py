"""The cases of the scheduled-surface tests (tests/test_emulation_step_surf.py on the CPU, tests/test_gpu_step_surf.py on the device):
the reset step of a step_dist_cases case -- the same horizons, feedback states, fast-path settings and bounds -- WITHOUT its input
disturbance and WITH a surface window surf [N, 6] (mpcb_step_surf), against the dense reference of tests/dense_qp_surf.py.

window(cfg, N, seed): the configuration's own a..f plus, per row k, a smooth variation of EVERY coefficient -- curvature (a, b, c),
slope (d, e) and height (f) -- of seeded amplitude and phase: +-0.03 on a, b, +-0.01 on c, +-0.02 on d, e, +-0.005 on f, one to
three periods over 40 rows.

ORACLE_VS_DENSE_SURF is the committed record of how far the oracle's QP routines, given the matrices of the dense assembly (the
oracle cannot express a stage-varying surface; its QP solvers take any OCP-QP), land from the dense solution of every case: the
reference solver's own error on that QP -- rounding where the fast path solves it, the interior point's termination at qp_tol where
it does not.  The bound of every engine-vs-dense comparison, here and in tests/test_gpu_step_surf.py, is 10 x that distance, floor
1e-12, and stays <= 1e-9 (the rule of tests/test_dense_qp.py).
"""
import numpy as np

import dense_qp as dq
import dense_qp_cases as dc
import dense_qp_surf as ds
import step_dist_cases as sd

# case id -> max |oracle - dense| over dX, dU, measured on the CPU (tests/test_emulation_step_surf.py re-measures a sample)
ORACLE_VS_DENSE_SURF = {
    "N1-rand-dist": 1.11e-16, "N2-rand-dist": 2.29e-16, "N3-rand-dist": 1.53e-16, "N7-rand-dist": 7.49e-16,
    "N20-rand-dist": 4.44e-15, "N25-rand-dist": 2.78e-16, "N26-rand-dist": 3.89e-16, "N37-rand-dist": 6.66e-16,
    "N38-rand-dist": 2.71e-14, "N42-rand-dist": 3.04e-16, "N43-rand-dist": 7.77e-16, "N80-rand-dist": 3.16e-15,
    "N125-rand-dist": 2.12e-14, "N126-rand-dist": 9.44e-16, "N130-rand-dist": 1.98e-14, "N135-rand-dist": 7.22e-16,
    "N136-rand-dist": 2.59e-14, "N140-rand-dist": 6.99e-14, "N141-rand-dist": 2.62e-13, "N245-rand-dist": 3.98e-13,
    "N246-rand-dist": 6.92e-14, "N20-rand-dist-ipm": 6.25e-12, "N130-rand-dist-ipm": 5.03e-13, "N20-tight-dist": 5.46e-12,
    "N20-tight-dist-ipm": 5.46e-12,
}
AMP = np.array([0.03, 0.03, 0.01, 0.02, 0.02, 0.005])
CLEARANCE = sd.CLEARANCE


def variation(rows, seed, r0=0):
    """[rows, 6]: what rows r0 .. r0 + rows - 1 of a table add to the base coefficients."""
    rng = np.random.default_rng(seed)
    amp = AMP * rng.uniform(0.5, 1.0, 6)
    freq = rng.uniform(1.0, 3.0, 6) * 2.0 * np.pi / 40.0
    phase = rng.uniform(0.0, 2.0 * np.pi, 6)
    r = (r0 + np.arange(rows))[:, None]
    return amp * np.sin(freq * r + phase)


def window(cfg, rows, seed, r0=0):
    return np.asarray(cfg["coeffs"], float)[None] + variation(rows, seed, r0)


def _with_surf(base):
    seed = 1100 + base["N"]
    return dict(base, surf=window(base["cfg"], base["N"], seed), surf_seed=seed)


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = [_with_surf(c) for c in sd.all_cases()]
    return _ALL


def by_id():
    return {c["id"]: c for c in all_cases()}


_QPS, _SOLS = {}, {}


def dense_qp(case):
    key = case["id"].replace("-ipm", "")
    if key not in _QPS:
        X, U = dc.guess(case)
        _QPS[key] = ds.assemble(dc.chain_of(case), case["cfg"], X, U, case["xhat"], case["surf"], case["yref"])
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
    iteration limit otherwise) on the matrices of the DENSE assembly: the oracle cannot express a stage-varying surface, its QP
    solvers take any OCP-QP.  What its distance from solve_equality / certify measures is the reference solver's own error on this QP."""
    cfg, N = case["cfg"], case["N"]
    qp = dense_qp(case)
    args = (qp.H, qp.g, qp.b, qp.A, qp.B, qp.lb, qp.ub, qp.dx0)
    q = orc.qp_fast(*args) if case["fast"] else dict(accepted=0)
    status = 0
    if not q["accepted"]:
        q = orc.qp_ipm(*args, tol=cfg["qp_tol"], iter_max=cfg["qp_iter_max"])
        status = q["status"]
    return dict(dX=q["w"][:, 6:], dU=q["w"][:N, :6], accepted=bool(q.get("accepted", 0)), status=status)


def tolerance(table, cid):
    """10 x the committed oracle-vs-dense distance of the case, floor 1e-12."""
    return max(10.0 * table[cid], 1e-12)


def check_step(case, out, i, tag, table=None, rtol_cost=1e-10):
    """One simulation of a reset step's output against the dense QP of its case on its window, and the cost at the returned iterate."""
    N = case["N"]
    X, U = dc.guess(case)
    xp, up = out["x_pred"][i][:N + 1], out["u_pred"][i][:N]
    assert np.isfinite(xp).all() and np.isfinite(up).all() and out["status"][i] == 0, (case["id"], out["status"][i])
    assert (out["qp_iter"][i] == 1) == (case["fast"] and not case["active"]), (case["id"], out["qp_iter"][i])
    dist, _ = distance(case, xp - X, up - U)
    bound = tolerance(ORACLE_VS_DENSE_SURF if table is None else table, case["id"])
    print(f"\n[surf] {tag} {case['id']}: distance from dense = {dist:.2e} (bound {bound:.1e})")
    assert dist <= bound, (tag, case["id"], dist)
    np.testing.assert_array_equal(out["u0"][i], up[0])
    want = ds.nlp_cost(dc.chain_of(case), case["cfg"], xp, up, case["surf"], case["yref"])
    np.testing.assert_allclose(out["cost"][i], want, rtol=rtol_cost, atol=0, err_msg=case["id"])
    return dist


CHAINED_CASE, CHAINED_STEPS = sd.CHAINED_CASE, 3
CHAINED_SEED = 1150


def chained_window(case, k):
    """The window of chained step k: rows [k, k + N) of one table -- a window that slides, as a rollout's does."""
    return window(case["cfg"], case["N"], CHAINED_SEED, r0=k)


def chained(case, step, shift=False):
    """step_dist_cases.chained with a surface window that slides one row per step instead of a disturbance: three steps without a
    reset on the off-model plant, carried or shifted.  `step(x, shift, surf)` -> (x_pred, u_pred) is the solver under test.  Step k
    minus the iterate it started from (the previous result, moved one stage when shifting, x_N propagated by the model) is
    certified against the dense QP assembled there on window k.  Returns the distances."""
    cfg, chain = case["cfg"], dc.chain_of(case)
    A, B = dq.lti(cfg["wcv"], cfg["dt"])
    Ap, Bp = dq.lti(0.8 * np.asarray(cfg["wcv"]), cfg["dt"])
    rng = np.random.default_rng(77)
    x, prev, out = case["xhat"].copy(), dc.guess(case), []
    for k in range(CHAINED_STEPS):
        w = chained_window(case, k)
        if shift and k > 0:
            Xs = np.vstack([prev[0][1:], (A @ prev[0][-1] + B @ prev[1][-1])[None]])
            Us = np.vstack([prev[1][1:], prev[1][-1:]])
            prev = (Xs, Us)
        xp, up = step(x, shift and k > 0, w)
        qp = ds.assemble(chain, cfg, prev[0], prev[1], x, w, case["yref"])
        cert = dq.certify(qp, xp - prev[0], up - prev[1])
        assert cert["min_multiplier"] >= 0 and cert["min_slack"] >= 1e-5, cert
        out.append(cert["distance"])
        prev = (xp.copy(), up.copy())
        x = Ap @ x + Bp @ up[0] + rng.uniform(-1e-3, 1e-3, 12)
    return out
