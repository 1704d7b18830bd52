"""The cases of the terminal-cost tests (tests/test_terminal_*.py on the CPU, tests/test_gpu_terminal*.py on the device): the reset
step of a dense_qp_cases case with a joint-wise LQR terminal cost.

A case is the dense_qp_cases dict plus  P [12, 12], blocks [6, 3] (pqq, pqv, pvv), x_e [12], term [30] (the record mpcb_step_term
takes: pqq 6 | pqv 6 | pvv 6 | x_e 12):
  P    scipy.linalg.solve_discrete_are on dense_qp.lti(wcv, dt) with Q = diag(10 x 6, 1 x 6), R = I -- deliberately not the product's
       own robotic_mpc_amd.terminal.lqr_terminal.  Its entries outside the six joint blocks are exactly 0 (asserted).
  x_e  the guess's terminal state plus a seeded offset, uniform +-0.02 on q and +-0.05 on qdot: seed 500 + N, or the first of
       500 + N + 1000 m whose dense minimiser clears every bound by CLEARANCE (tests/test_terminal_cases.py asserts it).
"""
import numpy as np

import dense_qp as dq
import dense_qp_cases as dc
import dense_qp_terminal as dt_

CLEARANCE = 0.05
# fast path on: short horizons, both sides of the first sweep switch of every launch geometry of tests/test_boundaries.py (25 | 26,
# 37 | 38, 42 | 43, 125 | 126, 135 | 136, 140 | 141), 80 (eight wavefronts by default), 130, the throughput engine's residual-items
# switch (246), 300; fast path off: one resident and one long horizon
FAST_HORIZONS = (1, 2, 3, 7, 20, 25, 26, 37, 38, 42, 43, 80, 125, 126, 130, 135, 136, 140, 141, 246, 300)
IPM_HORIZONS = (20, 200)
# m of the x_e seed 500 + N + 1000 m per horizon (0 wherever the first draw clears the bounds)
XE_TRY = {135: 28}     # (N = 135: the draws of m = 0 .. 27 leave 0.02 or less, most of them active bounds)
# N20-tight-term: dense_qp_cases.TIGHT with the xhat seed 120.  Its certificate separates as asked (min_multiplier > 0, free slack
# >= 1e-5) -- but with NO active bound: this terminal cost holds the terminal velocities at x_e, next to the start's, and keeps every
# input 0.26 inside its bound.  Moving the xhat seed does not change that: at every seed 120 .. 519 the bound-free minimiser clears
# every bound by >= 0.068.  The case stays as specified (tight bounds in the QP, none active: the fast path accepts, the interior
# point runs against near bounds) and is held to its certificate with n_active == 0.  Active bounds come with N20-tight-far-term:
# the same case with the q offsets of x_e ten times as large (+-0.2 rad), a terminal reference the inputs cannot reach inside
# their bounds -- five bounds active, multipliers >= 3.9e-2, free slack 1.1e-2.
TIGHT_SEED = 120
FAR_SCALE = 10.0


def lqr_weight(cfg):
    from scipy.linalg import solve_discrete_are

    A, B = dq.lti(cfg["wcv"], cfg["dt"])
    P = solve_discrete_are(A, B, np.diag(np.concatenate([np.full(6, 10.0), np.full(6, 1.0)])), np.eye(6))
    blocks = np.stack([np.diag(P)[:6], P[np.arange(6), 6 + np.arange(6)], np.diag(P)[6:]], axis=1)
    Pb = dt_.blocks_to_matrix(blocks)
    off = P.copy()
    off[Pb != 0] = 0.0
    assert (off == 0.0).all() and np.abs(P - Pb).max() <= 1e-12 * np.abs(P).max(), "the DARE solution is not joint-block diagonal"
    return Pb, blocks


def _with_terminal(base, cid, xe_seed, q_scale=1.0, certify=False):
    P, blocks = lqr_weight(base["cfg"])
    X, _ = dc.guess(base)
    rng = np.random.default_rng(xe_seed)
    x_e = X[-1] + np.concatenate([q_scale * rng.uniform(-0.02, 0.02, 6), rng.uniform(-0.05, 0.05, 6)])
    term = np.concatenate([blocks[:, 0], blocks[:, 1], blocks[:, 2], x_e])
    return dict(base, id=cid, base_id=base["id"], P=P, blocks=blocks, x_e=x_e, term=term, certify=certify)


def random_case(N, fast=True):
    base = dc.random_case(N, dc.SEEDS[N], fast=fast)
    return _with_terminal(base, f"N{N}-rand-term" + ("" if fast else "-ipm"), 500 + N + 1000 * XE_TRY.get(N, 0))


def tight_case(fast=True, far=False):
    """`far`: active bounds (N20-tight-far-term); otherwise the case as specified, whose bounds are tight but inactive."""
    base = dc._case("N20-tight" + ("" if fast else "-ipm"), dc._base(20, fast, **dc.TIGHT), far, TIGHT_SEED)
    return _with_terminal(base, "N20-tight%s-term" % ("-far" if far else "") + ("" if fast else "-ipm"), 500 + 20,
                          q_scale=FAR_SCALE if far else 1.0, certify=True)


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        out = [random_case(N) for N in FAST_HORIZONS] + [random_case(N, fast=False) for N in IPM_HORIZONS]
        out += [tight_case(True), tight_case(False), tight_case(True, far=True), tight_case(False, far=True)]
        ids = [c["id"] for c in out]
        assert len(set(ids)) == len(ids)
        _ALL = out
    return _ALL


def by_id():
    return {c["id"]: c for c in all_cases()}


_QPS, _SOLS = {}, {}


def dense_qp(case):
    key = case["id"].replace("-ipm", "")
    if key not in _QPS:
        X, U = dc.guess(case)
        _QPS[key] = dt_.assemble(dc.chain_of(case), case["cfg"], X, U, case["xhat"], case["P"], case["x_e"], case["yref"])
    return _QPS[key]


def dense_solution(case):
    key = case["id"].replace("-ipm", "")
    if key not in _SOLS:
        _SOLS[key] = dq.solve_equality(dense_qp(case))
    return _SOLS[key]


def clearance(case):
    """The smallest distance of the dense equality-constrained minimiser from any bound."""
    qp, sol = dense_qp(case), dense_solution(case)
    idx, lo, hi = qp.bounded()
    return float(np.minimum(sol["w"][idx] - lo, hi - sol["w"][idx]).min())


def oracle_qp(orc, case, X, U, xhat):
    """reference_checks.oracle_qp with the terminal block added: (H, g, b, A, B, lb, ub, dx0) as orc.qp_fast / orc.qp_ipm take them."""
    import reference_checks as rc

    cfg, N = case["cfg"], case["N"]
    rb = orc.make_robot(dc.chain_of(case), cfg["t_ee"])
    yref = np.tile(rc.g_ref(cfg), (N, 1)) if case["yref"] is None else case["yref"]
    H, g, b, A, B, lb, ub, dx0 = rc.oracle_qp(orc, rb, cfg, X, U, xhat, yref)
    H[N, 6:, 6:] += case["P"]
    g[N, 6:] += case["P"] @ (np.asarray(X, float)[N] - case["x_e"])
    return H, g, b, A, B, lb, ub, dx0


def oracle_solve(orc, case, X, U, xhat):
    """The oracle's QP routines on the terminal QP at (X, U): dict(dX, dU, accepted, status, iters)."""
    cfg, N = case["cfg"], case["N"]
    qp = oracle_qp(orc, case, X, U, xhat)
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
    active-set certificate (min_multiplier > 0, free slack >= 1e-5), an inactive one to the clearance of every bound."""
    qp = dense_qp(case)
    if case["certify"]:
        cert = dq.certify(qp, dX, dU)
        assert (cert["n_active"] > 0) == case["active"] and cert["min_multiplier"] > 0 and cert["min_slack"] >= 1e-5, \
            (case["id"], {k: cert[k] for k in ("n_active", "min_multiplier", "min_slack")})
        assert cert["candidate_min_slack"] >= 1e-5, (case["id"], cert["candidate_min_slack"])
        return cert["distance"], cert
    assert not case["active"]
    sol = dense_solution(case)
    assert clearance(case) >= CLEARANCE, case["id"]
    return float(max(np.abs(sol["dX"] - dX).max(), np.abs(sol["dU"] - dU).max())), sol


CHAINED_CASE, CHAINED_STEPS = "N20-rand-term", 3


def chained(case, step, orc=None, shift=False):
    """dense_qp_cases.chained_distances with the terminal cost: three steps without a reset on the off-model plant (the exact
    discretisation at 80 % of the bandwidths plus a seeded +-1e-3 perturbation), carried or shifted.  `step(x, shift)` ->
    (x_pred, u_pred) is the solver under test.  Step k minus the iterate it started from (the previous result, moved one stage
    when shifting: u_k <- u_{k+1} with the last input held, x_k <- x_{k+1} with x_N propagated by the model) is certified against
    the dense terminal QP assembled there.  Returns (the distances, the oracle's distances on the same QPs or None)."""
    cfg, chain = case["cfg"], dc.chain_of(case)
    A, B = dq.lti(cfg["wcv"], cfg["dt"])
    Ap, Bp = dq.lti(0.8 * np.asarray(cfg["wcv"]), cfg["dt"])
    rng = np.random.default_rng(77)
    x, prev, out, ora = case["xhat"].copy(), dc.guess(case), [], []
    for k in range(CHAINED_STEPS):
        if shift and k > 0:
            Xs = np.vstack([prev[0][1:], (A @ prev[0][-1] + B @ prev[1][-1])[None]])
            Us = np.vstack([prev[1][1:], prev[1][-1:]])
            prev = (Xs, Us)
        xp, up = step(x, shift and k > 0)
        qp = dt_.assemble(chain, cfg, prev[0], prev[1], x, case["P"], case["x_e"], case["yref"])
        cert = dq.certify(qp, xp - prev[0], up - prev[1])
        assert cert["min_multiplier"] >= 0 and cert["min_slack"] >= 1e-5, cert
        out.append(cert["distance"])
        if orc is not None:
            o = oracle_solve(orc, case, prev[0], prev[1], x)
            assert o["status"] == 0
            ora.append(float(max(np.abs(cert["dX"] - o["dX"]).max(), np.abs(cert["dU"] - o["dU"]).max())))
        prev = (xp.copy(), up.copy())
        x = Ap @ x + Bp @ up[0] + rng.uniform(-1e-3, 1e-3, 12)
    return out, (ora if orc is not None else None)
