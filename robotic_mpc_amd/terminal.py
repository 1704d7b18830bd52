"""Design of a joint-wise LQR terminal cost for ``BatchController.set_terminal_cost``.

The prediction model is six decoupled two-state joints, x_j = (q_j, qdot_j) with

    A_j = [[1, a12_j], [0, a22_j]],   B_j = [b1_j, b2_j]',   a22 = exp(-wcv dt), a12 = (1 - a22) / wcv, b1 = dt - a12, b2 = 1 - a22

(prediction_model.py:87-115).  For diagonal state and input weights the discrete algebraic Riccati equation of the 12-state model
therefore separates into six 2x2 equations, and its solution is exactly six symmetric 2x2 blocks: what the controller step's
terminal cost takes.  Each joint's equation is solved here by the structure-preserving doubling algorithm in numpy alone, so the
product does not need scipy.
"""
from __future__ import annotations

from typing import Dict, Mapping

import numpy as np

from . import config as cfgmod


def _dare_2x2(A: np.ndarray, B: np.ndarray, Q: np.ndarray, r: float, tol: float = 1e-15, iters: int = 200) -> np.ndarray:
    """The stabilising solution of P = A'PA - A'PB (r + B'PB)^-1 B'PA + Q for one joint (A 2x2, B 2x1) by the
    structure-preserving doubling algorithm: A_k, G_k, H_k with H_k -> P quadratically; then Newton-free polishing by a few fixed-point
    sweeps of the Riccati map itself, which contracts at the stabilising solution."""
    Ak, G, H = A.copy(), (B @ B.T) / r, Q.copy()
    I = np.eye(2)
    for _ in range(iters):
        W = np.linalg.inv(I + G @ H)
        A1 = Ak @ W @ Ak
        G1 = G + Ak @ W @ G @ Ak.T
        H1 = H + Ak.T @ H @ W @ Ak
        done = np.abs(H1 - H).max() <= tol * np.abs(H1).max()
        Ak, G, H = A1, G1, H1
        if done:
            break
    P = 0.5 * (H + H.T)
    for _ in range(3):
        PB = P @ B
        P = A.T @ P @ A - (A.T @ PB) @ (PB.T @ A) / (r + (B.T @ PB).item()) + Q
        P = 0.5 * (P + P.T)
    return P


def lqr_terminal(cfg: Mapping, q_weight=10.0, qdot_weight=1.0, r_weight=1.0) -> Dict[str, np.ndarray]:
    """The infinite-horizon LQR cost-to-go of the prediction model of ``cfg`` (a configuration as ``BatchController`` takes it) for
    the stage cost ``x'Qx + u'Ru`` with ``Q = diag(q_weight (6), qdot_weight (6))`` and ``R = r_weight I`` -- scalars or one value per
    joint, q_weight + qdot_weight > 0 and r_weight > 0 per joint.

    Returns dict(blocks [6, 3]: (pqq, pqv, pvv) per joint, as ``set_terminal_cost`` takes them; K [6, 2]: the LQR gain of each joint,
    u_j = -K_j (x_j - x_ref,j); P [12, 12]: the same weight as a matrix over [q; qdot], exactly zero outside the joint blocks)."""
    c = cfgmod.resolve_config(cfg)
    wcv, dt = np.asarray(c["wcv"], dtype=np.float64), float(c["dt"])
    qw, vw, rw = (np.broadcast_to(np.asarray(v, dtype=np.float64), (6,)) for v in (q_weight, qdot_weight, r_weight))
    if not (np.isfinite(qw).all() and np.isfinite(vw).all() and np.isfinite(rw).all()):
        raise ValueError("the LQR weights must be finite")
    if (qw < 0).any() or (vw < 0).any() or (qw + vw <= 0).any() or (rw <= 0).any():
        raise ValueError("the LQR weights must satisfy q_weight, qdot_weight >= 0, q_weight + qdot_weight > 0 and r_weight > 0")
    a22 = np.exp(-wcv * dt)
    a12 = (1.0 - a22) / wcv
    b1, b2 = dt - a12, 1.0 - a22
    blocks, K, P = np.zeros((6, 3)), np.zeros((6, 2)), np.zeros((12, 12))
    for j in range(6):
        A = np.array([[1.0, a12[j]], [0.0, a22[j]]])
        B = np.array([[b1[j]], [b2[j]]])
        Pj = _dare_2x2(A, B, np.diag([qw[j], vw[j]]), float(rw[j]))
        blocks[j] = Pj[0, 0], Pj[0, 1], Pj[1, 1]
        K[j] = ((B.T @ Pj @ A) / (rw[j] + (B.T @ Pj @ B).item())).ravel()
        P[j, j], P[j, 6 + j], P[6 + j, j], P[6 + j, 6 + j] = Pj[0, 0], Pj[0, 1], Pj[0, 1], Pj[1, 1]
    return dict(blocks=blocks, K=K, P=P)
