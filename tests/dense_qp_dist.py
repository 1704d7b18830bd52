"""The dense reference of tests/dense_qp.py with a constant input disturbance d [6] in the prediction model (mpcb_step_dist):

    x_{k+1} = Ad x_k + Bd (u_k + d),     qddot_k = (qdot_{k+1} - qdot_k) / dt of that model = Dx x_k + Du (u_k + d).

In the Gauss-Newton QP at the iterate (X, U): b_k gains Bd d, rows 11.. of the stage residual gain Du d = (Sel Bd / dt) d, and
g_k = dt Jr'W r is rebuilt with that residual.  The Jacobian, and with it every H_k, is unchanged; the input cost row stays u and the
bounds stay on u.  Everything else is dense_qp.assemble / nlp_cost / solve_equality / certify unchanged.  Plain numpy; nothing of
the engines or the oracle.
"""
import numpy as np

import dense_qp as dq


def accel_offset(cfg, d):
    """Du d: what rows 11..16 of the stage residual gain."""
    _, B = dq.lti(cfg["wcv"], cfg["dt"])
    return (B[6:] @ np.asarray(d, float)) / float(cfg["dt"])


def assemble(chain, cfg, X, U, xhat, d, yref=None):
    X, U, d = np.asarray(X, float), np.asarray(U, float), np.asarray(d, float)
    qp = dq.assemble(chain, cfg, X, U, xhat, yref)
    N, dt = qp.N, float(cfg["dt"])
    W = dq.weights(cfg)
    off = accel_offset(cfg, d)
    memo = {}
    for k in range(N):
        yk = None if yref is None else np.asarray(yref[k], float)
        key = (X[k].tobytes(), U[k].tobytes(), None if yk is None else yk.tobytes())
        if key not in memo:
            memo[key] = dq.stage_residual(chain, cfg, X[k], U[k], yk)
        r, Jr = memo[key]
        r = r.copy()
        r[11:] += off
        qp.g[k] = dt * Jr.T @ (W * r)
        qp.b[k] = qp.b[k] + qp.B @ d
    return qp


def nlp_cost(chain, cfg, X, U, d, yref=None):
    """sum_k dt 1/2 r'W r at (X, U) with the disturbed model's qddot rows."""
    W = dq.weights(cfg)
    A, B = dq.lti(cfg["wcv"], cfg["dt"])
    d = np.asarray(d, float)
    c = 0.0
    for k in range(U.shape[0]):
        xc, uc = np.asarray(X[k], float), np.asarray(U[k], float)
        y = dq.packed_reference(cfg) if yref is None else np.asarray(yref[k], float)
        r = np.concatenate([dq.task_outputs(chain, cfg["coeffs"], cfg["t_ee"], xc) - y, uc,
                            ((A @ xc + B @ (uc + d))[6:] - xc[6:]) / cfg["dt"]])
        c += 0.5 * cfg["dt"] * float(W @ (r * r))
    return c
