"""The cases of the input-disturbance tests (tests/test_step_dist_cases.py on the CPU, tests/test_gpu_step_dist.py on the device): the
reset step of a dense_qp_cases case with a constant input disturbance d in the prediction model (mpcb_step_dist).

A case is the dense_qp_cases dict plus  d [6], rad/s: uniform +-0.1, seed 900 + N, or the first of 900 + N + 1000 m whose dense
minimiser clears every bound by CLEARANCE (tests/test_step_dist_cases.py asserts it from the dense reference alone).
"""
import numpy as np

import dense_qp as dq
import dense_qp_cases as dc
import dense_qp_dist as dd

CLEARANCE = 0.05
D_AMP = 0.1
# fast path on: short horizons, both sides of the first sweep switch of every launch geometry of tests/test_boundaries.py (25 | 26,
# 37 | 38, 42 | 43, 125 | 126, 135 | 136, 140 | 141), 80 (eight wavefronts by default), 130, both sides of the throughput engine's
# residual-items switch (245 | 246); fast path off: one resident and one long horizon.  No N = 300: its dense solve takes seconds.
FAST_HORIZONS = (1, 2, 3, 7, 20, 25, 26, 37, 38, 42, 43, 80, 125, 126, 130, 135, 136, 140, 141, 245, 246)
IPM_HORIZONS = (20, 130)
# m of the seed 900 + N + 1000 m per horizon (0 wherever the first draw clears the bounds)
D_TRY = {}
# N20-tight-dist: dense_qp_cases' N20-tight (xhat seed 120) with d of seed 920: bounds active, held to the exact active-set certificate
TIGHT_SEED = 100 + 20


def draw(seed):
    return np.random.default_rng(seed).uniform(-D_AMP, D_AMP, 6)


def _with_dist(base, cid, seed, certify=False):
    return dict(base, id=cid, base_id=base["id"], d=draw(seed), d_seed=seed, certify=certify)


def random_case(N, fast=True, m=None):
    base = dc.random_case(N, dc.SEEDS[N], fast=fast)
    m = D_TRY.get(N, 0) if m is None else m
    return _with_dist(base, f"N{N}-rand-dist" + ("" if fast else "-ipm"), 900 + N + 1000 * m)


def tight_case(fast=True):
    base = dc._case("N20-tight" + ("" if fast else "-ipm"), dc._base(20, fast, **dc.TIGHT), True, TIGHT_SEED)
    return _with_dist(base, "N20-tight-dist" + ("" if fast else "-ipm"), 900 + 20, certify=True)


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        out = [random_case(N) for N in FAST_HORIZONS] + [random_case(N, fast=False) for N in IPM_HORIZONS]
        out += [tight_case(True), tight_case(False)]
        ids = [c["id"] for c in out]
        assert len(set(ids)) == len(ids)
        _ALL = out
    return _ALL


def by_id():
    return {c["id"]: c for c in all_cases()}


_QPS, _SOLS = {}, {}


def dense_qp(case):
    key = (case["id"].replace("-ipm", ""), case["d_seed"])
    if key not in _QPS:
        X, U = dc.guess(case)
        _QPS[key] = dd.assemble(dc.chain_of(case), case["cfg"], X, U, case["xhat"], case["d"], case["yref"])
    return _QPS[key]


def dense_solution(case):
    key = (case["id"].replace("-ipm", ""), case["d_seed"])
    if key not in _SOLS:
        _SOLS[key] = dq.solve_equality(dense_qp(case))
    return _SOLS[key]


def clearance(case):
    """The smallest distance of the dense equality-constrained minimiser from any bound."""
    qp, sol = dense_qp(case), dense_solution(case)
    idx, lo, hi = qp.bounded()
    return float(np.minimum(sol["w"][idx] - lo, hi - sol["w"][idx]).min())


def oracle_qp(orc, case, X, U, xhat, d=None):
    """reference_checks.oracle_qp with the two changes of the disturbed model applied to its matrices: b_k += B d, and g_k gains
    dt Jr'W [0 (11); Du d] = dt w_qddot [Du; 0; Dx]' Du d (the acceleration rows of Jr are linear: no task Jacobian is needed).
    (H, g, b, A, B, lb, ub, dx0) as orc.qp_fast / orc.qp_ipm take them."""
    import reference_checks as rc

    cfg, N = case["cfg"], case["N"]
    d = case["d"] if d is None else np.asarray(d, float)
    rb = orc.make_robot(dc.chain_of(case), cfg["t_ee"])
    yref = np.tile(rc.g_ref(cfg), (N, 1)) if case["yref"] is None else case["yref"]
    H, g, b, A, B, lb, ub, dx0 = rc.oracle_qp(orc, rb, cfg, X, U, xhat, yref)
    Ad, Bd = dq.lti(cfg["wcv"], cfg["dt"])
    dt = float(cfg["dt"])
    Du = Bd[6:] / dt
    Dx = np.hstack([np.zeros((6, 6)), (Ad[6:, 6:] - np.eye(6)) / dt])
    Ja = np.hstack([Du, Dx])                       # rows 11.. of Jr over [u; q; qdot]
    add = dt * float(cfg["w_qddot"]) * Ja.T @ (Du @ d)
    b = np.array(b, float)
    g = np.array(g, float)
    for k in range(N):
        b[k] += Bd @ d
        g[k] += add
    return H, g, b, A, B, lb, ub, dx0


def oracle_solve(orc, case, X, U, xhat, d=None):
    """The oracle's QP routines on the disturbed QP at (X, U): dict(dX, dU, accepted, status, iters)."""
    cfg, N = case["cfg"], case["N"]
    qp = oracle_qp(orc, case, X, U, xhat, d)
    q = orc.qp_fast(*qp) if case["fast"] else dict(accepted=0)
    status, iters = 0, 1
    if not q["accepted"]:
        q = orc.qp_ipm(*qp, tol=cfg["qp_tol"], iter_max=cfg["qp_iter_max"])
        status, iters = q["status"], q["iters"]
    return dict(dX=q["w"][:, 6:], dU=q["w"][:N, :6], accepted=bool(q.get("accepted", 0)), status=status, iters=iters)


def oracle_solution(orc, case):
    X, U = dc.guess(case)
    return oracle_solve(orc, case, X, U, case["xhat"])


def tolerance(table, cid):
    """10 x the committed oracle-vs-dense distance of the case, floor 1e-12."""
    return max(10.0 * table[cid][0], 1e-12)


def distance(case, dX, dU):
    """(distance of a candidate QP step from the dense solution, the solve / certificate); an active case is held to its exact
    active-set certificate (active bounds, min_multiplier > 0, free slack >= 1e-5), an inactive one to the clearance of every bound."""
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


CHAINED_CASE, CHAINED_STEPS = "N20-rand-dist", 3
CHAINED_D_SEED = 950           # the disturbance of step k: draw(CHAINED_D_SEED + k), a different one each step


def chained_dist(k):
    return draw(CHAINED_D_SEED + k)


def chained(case, step, orc=None, shift=False):
    """dense_qp_cases.chained_distances with a disturbance that changes every step: three steps without a reset on the off-model
    plant (the exact discretisation at 80 % of the bandwidths plus a seeded +-1e-3 perturbation), carried or shifted.
    `step(x, shift, d)` -> (x_pred, u_pred) is the solver under test, d = chained_dist(k).  Step k minus the iterate it started from
    (the previous result, moved one stage when shifting: u_k <- u_{k+1} with the last input held, x_k <- x_{k+1} with x_N propagated
    by the model with THIS step's disturbance, Ad x_N + Bd (u_{N-1} + d)) is certified against the dense QP assembled there.
    Returns (the distances, the oracle's distances on the same QPs or None)."""
    cfg, chain = case["cfg"], dc.chain_of(case)
    A, B = dq.lti(cfg["wcv"], cfg["dt"])
    Ap, Bp = dq.lti(0.8 * np.asarray(cfg["wcv"]), cfg["dt"])
    rng = np.random.default_rng(77)
    x, prev, out, ora = case["xhat"].copy(), dc.guess(case), [], []
    for k in range(CHAINED_STEPS):
        d = chained_dist(k)
        if shift and k > 0:
            Xs = np.vstack([prev[0][1:], (A @ prev[0][-1] + B @ (prev[1][-1] + d))[None]])
            Us = np.vstack([prev[1][1:], prev[1][-1:]])
            prev = (Xs, Us)
        xp, up = step(x, shift and k > 0, d)
        qp = dd.assemble(chain, cfg, prev[0], prev[1], x, d, case["yref"])
        cert = dq.certify(qp, xp - prev[0], up - prev[1])
        assert cert["min_multiplier"] >= 0 and cert["min_slack"] >= 1e-5, cert
        out.append(cert["distance"])
        if orc is not None:
            o = oracle_solve(orc, case, prev[0], prev[1], x, d)
            assert o["status"] == 0
            ora.append(float(max(np.abs(cert["dX"] - o["dX"]).max(), np.abs(cert["dU"] - o["dU"]).max())))
        prev = (xp.copy(), up.copy())
        x = Ap @ x + Bp @ (up[0] + d) + rng.uniform(-1e-3, 1e-3, 12)
    return out, (ora if orc is not None else None)
