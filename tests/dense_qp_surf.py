"""The dense reference of tests/dense_qp.py on a stage-varying surface (mpcb_step_surf): stage k of the horizon evaluates the task
outputs g1..g5 on the quadric surf[k] = (a, b, c, d, e, f) instead of cfg["coeffs"].

Built on dense_qp.stage_residual called with a per-stage copy of `cfg`: the residual r_k, its Jacobian (complex step through the
stage's own quadric) and with them H_k = dt Jr'W Jr, g_k = dt Jr'W r and the cost all change; the dynamics, the bounds and the
terminal block do not.  Everything else is dense_qp.solve_equality / certify unchanged.  Plain numpy; nothing of the engines or the
oracle.
"""
import numpy as np

import dense_qp as dq


def stage_cfg(cfg, coeffs_k):
    c = dict(cfg)
    c["coeffs"] = np.asarray(coeffs_k, float).copy()
    return c


def assemble(chain, cfg, X, U, xhat, surf, yref=None):
    """dense_qp.assemble with surf [N, 6]: H_k, g_k of stages 0..N-1 rebuilt on the stage's own quadric."""
    X, U, surf = np.asarray(X, float), np.asarray(U, float), np.asarray(surf, float)
    qp = dq.assemble(chain, cfg, X, U, xhat, yref)
    N, dt, lm = qp.N, float(cfg["dt"]), float(cfg.get("levenberg_marquardt", 0.0))
    assert surf.shape == (N, 6)
    W = dq.weights(cfg)
    for k in range(N):
        yk = None if yref is None else np.asarray(yref[k], float)
        r, Jr = dq.stage_residual(chain, stage_cfg(cfg, surf[k]), X[k], U[k], yk)
        qp.H[k] = dt * Jr.T @ (W[:, None] * Jr) + dt * lm * np.eye(dq.NW)
        qp.g[k] = dt * Jr.T @ (W * r)
    return qp


def nlp_cost(chain, cfg, X, U, surf, yref=None):
    """sum_k dt 1/2 r'W r at (X, U) with stage k's task outputs on surf[k]."""
    surf = np.asarray(surf, float)
    c = 0.0
    for k in range(U.shape[0]):
        yk = None if yref is None else np.asarray(yref[k], float)[None]
        c += dq.nlp_cost(chain, stage_cfg(cfg, surf[k]), np.asarray(X[k:k + 2], float), np.asarray(U[k:k + 1], float), yk)
    return c
