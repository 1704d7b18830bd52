"""The reference of the weight-sensitivity tests (mpcb_step_sens_w): d u0 / d weight of one Gauss-Newton QP from the dense KKT
system of tests/dense_qp.py, shared by the emulation and the device tests.  Oracle-free: plain numpy / scipy.

The KKT matrix K and right-hand side of dense_qp._kkt are affine in the seven weights theta = (w_u, w_qddot, w_task[0..4]), so with
K z = rhs solved once by a pivoted sparse LU,  d z / d theta_p = K^-1 (D rhs_p - D K_p z) / (s h_p)  where D K_p, D rhs_p are the
differences of the KKT matrix and right-hand side RE-ASSEMBLED (dense_qp.assemble, dense_qp._kkt) with weight p raised by s h_p
(h_p = theta_p, or 1 for a weight of 0) from the ones at theta.  That is exact up to rounding for any s: s = 1 and s = 0.5 are
both taken and their disagreement, per weight row, is the reference's own noise d_ref_p -- the rounding of the two assemblies
that the subtraction leaves behind.  (s = 1 and s = 0.5 scale a weight by 2 and by 1.5, and on a few rows -- row 0 of N1-rand and
of N20-ramp -- the two re-assembled values agree bit for bit although both carry the same rounding, 3.5e-14 of the row on
N1-rand: d_ref_p is 0 there and does not see it.)  The VALUE the engines are compared with is therefore the same expression
evaluated without that subtraction: D K_p and D rhs_p formed stage by stage from the weight difference itself, by the two
lines of dense_qp.assemble (H_k = dt Jr' W Jr, g_k = dt Jr' W r with dense_qp.weights and dense_qp.stage_residual); it is
asserted to be the re-assembled one within 1e-9 of the row.  The bound stays the one built from the re-assembled d_ref_p.  z
and the rows of K^-1 are refined with an extended-precision residual, as dense_qp.solve_equality refines its solution.  K is
symmetric, so the six rows of K^-1 that give du_0 come from one block solve, and with them every stage's addend to every entry:
A_p = max_c sum_k |addend of stage k| is the rounding scale of the sum the engines form.
central_differences() is the same derivative from full dense solves (assemble + solve_equality) at weights moved both ways: it
guards against a sign error here, not precision.
"""
import numpy as np
import scipy.sparse.linalg as spla

import dense_qp as dq

NWEIGHT = 7
SCALES = (1.0, 0.5)
MARGIN = 10.0            # the project's margin of dense-QP comparisons (dense_qp_cases.tolerance)
CONDITION = 1e-6         # no asserted bound may exceed this fraction of the row's max |J|: a wrong term is an O(1) relative error
CD_REL_STEP = 1e-4
CD_AGREE = 1e-6          # central differences agree with the reference to this fraction of the row's max


def theta(cfg):
    return np.concatenate([[float(cfg["w_u"]), float(cfg["w_qddot"])], np.asarray(cfg["w_task"], float)])


def with_weights(cfg, th):
    c = dict(cfg)
    c["w_u"], c["w_qddot"], c["w_task"] = float(th[0]), float(th[1]), [float(v) for v in th[2:]]
    return c


def _steps(th):
    return np.where(th > 0.0, th, 1.0)


def dense_weight_jacobian(chain, cfg, X, U, xhat, yref=None, refine=True):
    """dict(J [7, 6] = d u0 / d theta, d_ref [7], scale [7] = max_c |J[p][c]|, A [7], u0) of the QP at the iterate (X, U)."""
    X, U = np.asarray(X, float), np.asarray(U, float)
    N, dt = U.shape[0], float(cfg["dt"])
    qp = dq.assemble(chain, cfg, X, U, xhat, yref)
    K, rhs, n = dq._kkt(qp, np.zeros(0, dtype=int), np.zeros(0))
    lu = spla.splu(K.tocsc())
    z = lu.solve(rhs)
    ref = dq.solve_equality(qp)
    assert np.abs(z[:n] - ref["w"]).max() <= 1e-9 * max(1.0, np.abs(ref["w"]).max())
    E = np.zeros((rhs.size, 6))
    E[np.arange(6), np.arange(6)] = 1.0
    Y = lu.solve(E)                                   # K symmetric: column c is row c of K^-1
    if refine:
        # the primal part of z from solve_equality's refined solution (D K_p only touches the Hessian blocks), and the rows of
        # K^-1 refined the same way: residual in np.longdouble, correction through the same LU
        z = np.concatenate([ref["w"], z[n:]])
        Kc = K.tocoo()
        r_, c_, v_ = Kc.row, Kc.col, Kc.data.astype(np.longdouble)
        Yl = Y.astype(np.longdouble)
        for _ in range(3):
            res = E.astype(np.longdouble)
            for j in range(6):
                np.subtract.at(res[:, j], r_, v_ * Yl[c_, j])
            Yl = Yl + lu.solve(res.astype(np.float64)).astype(np.longdouble)
        Y = Yl.astype(np.float64)
    assert np.abs(Y[:6, :6] - Y[:6, :6].T).max() <= 1e-9 * np.abs(Y[:6, :6]).max()
    th, W0 = theta(cfg), dq.weights(cfg)
    h = _steps(th)
    memo, stages = {}, []
    for k in range(N):
        yk = None if yref is None else np.asarray(yref[k], float)
        key = (X[k].tobytes(), U[k].tobytes(), None if yk is None else yk.tobytes())
        if key not in memo:
            memo[key] = dq.stage_residual(chain, cfg, X[k], U[k], yk)
        stages.append(memo[key])
    Js = []
    add = np.zeros((NWEIGHT, N, 6))
    for s in SCALES:
        Jr_ = np.zeros((NWEIGHT, 6))
        for p in range(NWEIGHT):
            t2 = th.copy()
            t2[p] += s * h[p]
            cfg2 = with_weights(cfg, t2)
            K2, rhs2, _ = dq._kkt(dq.assemble(chain, cfg2, X, U, xhat, yref), np.zeros(0, dtype=int), np.zeros(0))
            v = (rhs2 - rhs) - (K2 - K).tocsr() @ z            # D rhs_p - D K_p z: zero outside the stage blocks of the primal part
            assert not v[dq.NW * N:].any()                       # (the terminal stage and the constraints carry no weight)
            Jr_[p] = Y[:dq.NW * N].T @ v[:dq.NW * N] / (s * h[p])
            if s == SCALES[0]:
                # the same D rhs_p - D K_p z stage by stage WITHOUT the subtraction of two assembled matrices: the two lines of
                # dense_qp.assemble (H_k = dt Jr' W Jr, g_k = dt Jr' W r) applied to the weight difference itself
                dW = dq.weights(cfg2) - W0
                for k, (r, Jr) in enumerate(stages):
                    sl = slice(dq.NW * k, dq.NW * k + dq.NW)
                    add[p, k] = Y[sl].T @ (-dt * Jr.T @ (dW * r) - dt * Jr.T @ (dW[:, None] * Jr) @ z[sl]) / (s * h[p])
        Js.append(Jr_)
    J, d_ref, A = add.sum(axis=1), np.abs(Js[0] - Js[1]).max(axis=1), np.abs(add).sum(axis=1).max(axis=1)
    # one quantity, two evaluations: the re-assembled one carries the rounding of the assemblies (up to 1e-9 of the row)
    rows = slice(0, 2) if N == 1 else slice(0, NWEIGHT)
    assert (np.abs(J[rows] - Js[0][rows]).max(axis=1) <= 1e-9 * np.abs(J[rows]).max(axis=1)).all()
    if N == 1:
        # stage 0's task term is a constant of the QP (x_0 is pinned to xhat) and there is no other stage: the five task rows are
        # zero by structure, not by cancellation -- the engines must write zeros there, and the reference says so exactly
        J[2:], d_ref[2:], A[2:] = 0.0, 0.0, 0.0
    return dict(J=J, d_ref=d_ref, scale=np.abs(J).max(axis=1), A=A, u0=U[0] + ref["dU"][0])


def central_differences(chain, cfg, X, U, xhat, yref=None, rel=CD_REL_STEP):
    """[7, 6] by central differences of the full dense solve, every weight moved by +- rel h_p."""
    th = theta(cfg)
    h = _steps(th)
    J = np.zeros((NWEIGHT, 6))
    for p in range(NWEIGHT):
        u = []
        for sg in (1.0, -1.0):
            t2 = th.copy()
            t2[p] += sg * rel * h[p]
            u.append(dq.solve_equality(dq.assemble(chain, with_weights(cfg, t2), X, U, xhat, yref))["dU"][0])
        J[p] = (u[0] - u[1]) / (2.0 * rel * h[p])
    return J


def bounds(ref, eps_case):
    """b_p = 10 x max(d_ref_p, eps(case) x A_p), each of which must stay below CONDITION x scale_p (rows whose Jacobian is
    exactly zero -- the task rows at N = 1 -- have the bound 0: the engines write zeros there)."""
    b = MARGIN * np.maximum(ref["d_ref"], eps_case * ref["A"])
    assert (b <= CONDITION * ref["scale"]).all(), (b, ref["scale"])
    return b


def distances(ref, du0_dw):
    return np.abs(np.asarray(du0_dw) - ref["J"]).max(axis=1)
