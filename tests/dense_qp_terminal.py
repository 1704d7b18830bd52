"""The dense reference of tests/dense_qp.py with the joint-wise terminal cost of the controller step (mpcb_step_term):

    l_N(x) = 1/2 (x - x_e)' P (x - x_e),   P symmetric 12x12 over x = [q; qdot], not scaled by dt.

In the Gauss-Newton QP at the iterate (X, U): H_N += P, g_N += P (X_N - x_e); the cost of an iterate gains l_N(X_N).  Everything
else is dense_qp.assemble / nlp_cost / solve_equality / certify unchanged.  d u0 / d x_e comes from the same single LU as
sens_checks.dense_jacobians: x_e,i moves -g_N by +P e_i.  Plain numpy / scipy; nothing of the engines or the oracle.
"""
import numpy as np
import scipy.sparse.linalg as spla

import dense_qp as dq
import sens_checks as sc


def blocks_to_matrix(blocks):
    """[6, 3] (pqq, pqv, pvv per joint) -> the symmetric 12x12 P."""
    b = np.asarray(blocks, float)
    P = np.zeros((12, 12))
    P[np.arange(6), np.arange(6)] = b[:, 0]
    P[np.arange(6), 6 + np.arange(6)] = b[:, 1]
    P[6 + np.arange(6), np.arange(6)] = b[:, 1]
    P[6 + np.arange(6), 6 + np.arange(6)] = b[:, 2]
    return P


def assemble(chain, cfg, X, U, xhat, P, x_e, yref=None):
    qp = dq.assemble(chain, cfg, X, U, xhat, yref)
    N = qp.N
    qp.H[N][6:, 6:] += P
    qp.g[N][6:] += P @ (np.asarray(X, float)[N] - np.asarray(x_e, float))
    return qp


def terminal_cost(X, P, x_e):
    e = np.asarray(X, float)[-1] - np.asarray(x_e, float)
    return 0.5 * float(e @ P @ e)


def nlp_cost(chain, cfg, X, U, P, x_e, yref=None):
    return dq.nlp_cost(chain, cfg, X, U, yref) + terminal_cost(X, P, x_e)


def dense_jacobians(chain, cfg, X, U, xhat, P, x_e, yref=None):
    """sens_checks.dense_jacobians of the terminal QP plus Jxe [6, 12] = d u0 / d x_e; d_ref and scale cover all three."""
    X, U = np.asarray(X, float), np.asarray(U, float)
    N = U.shape[0]
    qp = assemble(chain, cfg, X, U, xhat, P, x_e, yref)
    K, rhs, n = dq._kkt(qp, np.zeros(0, dtype=int), np.zeros(0))
    lu = spla.splu(K.tocsc())
    base = lu.solve(rhs)
    ref = dq.solve_equality(qp)
    assert np.abs(base[:n] - ref["w"]).max() <= 1e-9 * max(1.0, np.abs(ref["w"]).max())
    W, dt = dq.weights(cfg), float(cfg["dt"])
    cols = []
    for j in range(12):
        v = np.zeros_like(rhs)
        v[n + j] = 1.0
        cols.append(v)
    memo = {}
    for k in range(N):
        key = (X[k].tobytes(), U[k].tobytes())
        if key not in memo:
            memo[key] = dq.stage_residual(chain, cfg, X[k], U[k], None)[1]
        Jr = memo[key]
        for c in range(5):
            v = np.zeros_like(rhs)
            e = np.zeros(dq.NR)
            e[c] = 1.0
            v[dq.NW * k:dq.NW * k + dq.NW] = dt * Jr.T @ (W * e)
            cols.append(v)
    for i in range(12):                         # x_e,i: the right-hand side -g_N gains +P e_i
        v = np.zeros_like(rhs)
        v[dq.NW * N:dq.NW * N + 12] = P[:, i]
        cols.append(v)
    D = np.stack(cols, axis=1)
    J = []
    for h in sc.STEPS:
        up = lu.solve(rhs[:, None] + h * D)[:6]
        dn = lu.solve(rhs[:, None] - h * D)[:6]
        J.append((up - dn) / (2.0 * h))
    d_ref = float(np.abs(J[0] - J[1]).max())
    Jm = J[0]
    Jx = Jm[:, :12].copy()
    Jy = Jm[:, 12:12 + 5 * N].reshape(6, N, 5).transpose(1, 2, 0).copy()
    Jxe = Jm[:, 12 + 5 * N:].copy()
    scale = float(max(np.abs(Jx).max(), np.abs(Jy).max(), np.abs(Jxe).max()))
    return dict(Jx=Jx, Jy=Jy, Jxe=Jxe, d_ref=d_ref, scale=scale, u0=U[0] + ref["dU"][0])


def distance(ref, du0_dx, du0_dyref, du0_dxe):
    N = ref["Jy"].shape[0]
    return float(max(np.abs(du0_dx - ref["Jx"]).max(), np.abs(du0_dyref[:N] - ref["Jy"]).max(), np.abs(du0_dxe - ref["Jxe"]).max()))
