"""The dense reference of tests/dense_qp.py with the terminal cost, the input disturbance and the stage-varying surface TOGETHER
(mpcb_step_combined): the three assemblies of dense_qp_terminal.py, dense_qp_dist.py and dense_qp_surf.py composed.

    stage k < N:  r_k on the quadric surf[k], rows 11.. of r_k gain Du d;  H_k = dt Jr'W Jr (+ dt lm I), g_k = dt Jr'W r_k
    dynamics:     b_k += Bd d
    stage N:      H_N += P,  g_N += P (X_N - x_e)             (not scaled by dt)

The Jacobian of the acceleration rows does not depend on d, and the task rows do not depend on u: the three changes touch disjoint
parts of the QP except g_k, which is rebuilt once from the residual that carries both.  Everything else is dense_qp.assemble /
solve_equality / certify unchanged.  Plain numpy; nothing of the engines or the oracle.
"""
import numpy as np

import dense_qp as dq
import dense_qp_dist as dd
import dense_qp_surf as ds
import dense_qp_terminal as dt_


def assemble(chain, cfg, X, U, xhat, surf, d, P, x_e, yref=None):
    X, U, surf, d = np.asarray(X, float), np.asarray(U, float), np.asarray(surf, float), np.asarray(d, float)
    qp = dq.assemble(chain, cfg, X, U, xhat, yref)
    N, dt, lm = qp.N, float(cfg["dt"]), float(cfg.get("levenberg_marquardt", 0.0))
    assert surf.shape == (N, 6)
    W = dq.weights(cfg)
    off = dd.accel_offset(cfg, d)
    for k in range(N):
        yk = None if yref is None else np.asarray(yref[k], float)
        r, Jr = dq.stage_residual(chain, ds.stage_cfg(cfg, surf[k]), X[k], U[k], yk)
        r = r.copy()
        r[11:] += off
        qp.H[k] = dt * Jr.T @ (W[:, None] * Jr) + dt * lm * np.eye(dq.NW)
        qp.g[k] = dt * Jr.T @ (W * r)
        qp.b[k] = qp.b[k] + qp.B @ d
    qp.H[N][6:, 6:] += P
    qp.g[N][6:] += P @ (X[N] - np.asarray(x_e, float))
    return qp


def nlp_cost(chain, cfg, X, U, surf, d, P, x_e, yref=None):
    """sum_k dt 1/2 r'W r with stage k's task outputs on surf[k] and the disturbed model's qddot rows, plus l_N(X_N)."""
    surf = np.asarray(surf, float)
    c = 0.0
    for k in range(U.shape[0]):
        yk = None if yref is None else np.asarray(yref[k], float)[None]
        c += dd.nlp_cost(chain, ds.stage_cfg(cfg, surf[k]), np.asarray(X[k:k + 2], float), np.asarray(U[k:k + 1], float), d, yk)
    return c + dt_.terminal_cost(X, P, x_e)
