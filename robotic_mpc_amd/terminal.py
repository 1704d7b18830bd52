"""Design of a joint-wise LQR terminal cost for ``BatchController.set_terminal_cost``.

The prediction model is six decoupled two-state joints, x_j = (q_j, qdot_j) with

    A_j = [[1, a12_j], [0, a22_j]],   B_j = [b1_j, b2_j]',   a22 = exp(-wcv dt), a12 = (1 - a22) / wcv, b1 = dt - a12, b2 = 1 - a22

(prediction_model.py:87-115).  For diagonal state and input weights the discrete algebraic Riccati equation of the 12-state model
therefore separates into six 2x2 equations, and its solution is exactly six symmetric 2x2 blocks: what the controller step's
terminal cost takes.  Each joint's equation is solved here by the structure-preserving doubling algorithm in numpy alone, so the
product does not need scipy.

Rollouts take the same cost through the configuration key ``terminal_cost`` (mpcb_rollout_term): a plain JSON spec

``{"weight":    {"kind": "lqr", "q_weight": .., "qdot_weight": .., "r_weight": ..}   scalars or 6 values, as lqr_terminal takes them``
``            | {"kind": "blocks", "blocks": [6][3]},                               (pqq, pqv, pvv) per joint``
`` "reference": {"kind": "constant", "value": [12]}``
``            | {"kind": "table", "rows": [Nsim][12]}}                              row t is x_ref of closed-loop step t``

with the blocks constant over the run.  ``stack`` makes the arrays of one launch, ``reference_from_run`` the table that closes a
short horizon around the logged trajectory of a long one.
"""
from __future__ import annotations

from typing import Any, Dict, Mapping, Sequence, Tuple

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
    return _lqr(np.asarray(c["wcv"], dtype=np.float64), float(c["dt"]), q_weight, qdot_weight, r_weight)


def _lqr(wcv: np.ndarray, dt: float, q_weight, qdot_weight, r_weight) -> Dict[str, np.ndarray]:
    """lqr_terminal from the model's bandwidths and sampling time."""
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


# ---- the configuration key `terminal_cost` ---------------------------------------------------------------------------------------
KEY = "terminal_cost"
NX = 12
_TOP_KEYS = ("weight", "reference")
_WEIGHT_KEYS = {"lqr": ("q_weight", "qdot_weight", "r_weight"), "blocks": ("blocks",)}
_REFERENCE_KEYS = {"constant": ("value",), "table": ("rows",)}


def _part(spec: Mapping, name: str, kinds: Mapping) -> Tuple[str, Mapping]:
    part = spec[name]
    if not isinstance(part, Mapping):
        raise ValueError(f"{KEY} {name} must be a dict with a 'kind'")
    kind = part.get("kind")
    if kind not in kinds:
        raise ValueError(f"{KEY} {name}.kind must be one of {tuple(kinds)}, got {kind!r}")
    want = ("kind",) + kinds[kind]
    if set(part) != set(want):
        raise ValueError(f"a {kind!r} {KEY} {name} has the keys {want} (got {sorted(part)})")
    return kind, part


def _numbers(value: Any, shapes: Sequence[tuple], name: str, what: str) -> np.ndarray:
    if isinstance(value, (bool, str)) or value is None:
        raise ValueError(f"{KEY} {name} must be {what}")
    try:
        v = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{KEY} {name} must be {what}") from None
    if not any(len(sh) == v.ndim and all(a is None or a == b for a, b in zip(sh, v.shape)) for sh in shapes):
        raise ValueError(f"{KEY} {name} must be {what}, got shape {v.shape}")
    if not np.all(np.isfinite(v)):
        raise ValueError(f"{KEY} {name} must be finite")
    return v


def _lqr_weights(part: Mapping):
    ws = [np.broadcast_to(_numbers(part[k], ((), (6,)), f"weight.{k}", "a number or 6 numbers"), (6,)) for k in _WEIGHT_KEYS["lqr"]]
    qw, vw, rw = ws
    if (qw < 0).any() or (vw < 0).any() or (qw + vw <= 0).any() or (rw <= 0).any():
        raise ValueError(f"{KEY} weight: the LQR weights must satisfy q_weight, qdot_weight >= 0, q_weight + qdot_weight > 0 and "
                         "r_weight > 0")
    return qw, vw, rw


def validate(spec: Any) -> None:
    """What can be said about a spec without the run length and the model: its keys, its kinds, its shapes, finite numbers, and
    every given block positive semidefinite (the rule of BatchController.set_terminal_cost)."""
    if not isinstance(spec, Mapping):
        raise ValueError(f"{KEY} must be a dict (or None)")
    if set(spec) != set(_TOP_KEYS):
        raise ValueError(f"{KEY} has the keys {_TOP_KEYS} (got {sorted(spec)})")
    kind, part = _part(spec, "weight", _WEIGHT_KEYS)
    if kind == "lqr":
        _lqr_weights(part)
    else:
        b = _numbers(part["blocks"], ((6, 3),), "weight.blocks", "[6][3] numbers (pqq, pqv, pvv per joint)")
        pqq, pqv, pvv = b[:, 0], b[:, 1], b[:, 2]
        if (pqq < 0.0).any() or (pvv < 0.0).any() or (pqq * pvv < pqv * pqv).any():
            raise ValueError(f"{KEY} weight.blocks: every joint block must be positive semidefinite: pqq >= 0, pvv >= 0, "
                             "pqq pvv >= pqv^2")
    kind, part = _part(spec, "reference", _REFERENCE_KEYS)
    if kind == "constant":
        _numbers(part["value"], ((NX,),), "reference.value", f"{NX} numbers [q; qdot]")
    else:
        _numbers(part["rows"], ((None, NX),), "reference.rows", f"[Nsim][{NX}] numbers")


def sample(cfg: Mapping) -> Dict[str, np.ndarray]:
    """The realised terminal cost of a resolved configuration (config.resolve_config) that carries one:
    {"blocks": [6, 3] (pqq, pqv, pvv) per joint, "x_ref": [Nsim, 12], row t = the terminal reference of step t}, float64."""
    spec = cfg.get(KEY)
    if spec is None:
        raise ValueError(f"this configuration has no {KEY}")
    validate(spec)
    nsim = int(cfg["Nsim"])
    w, r = spec["weight"], spec["reference"]
    if w["kind"] == "lqr":
        blocks = _lqr(np.asarray(cfg["wcv"], dtype=np.float64).reshape(6), float(cfg["dt"]), *_lqr_weights(w))["blocks"]
    else:
        blocks = np.asarray(w["blocks"], dtype=np.float64)
    if r["kind"] == "constant":
        x_ref = np.tile(np.asarray(r["value"], dtype=np.float64)[None, :], (nsim, 1))
    else:
        x_ref = np.asarray(r["rows"], dtype=np.float64)
        if x_ref.shape[0] != nsim:
            raise ValueError(f"a 'table' {KEY} reference needs exactly Nsim = {nsim} rows, got {x_ref.shape[0]}")
    return {"blocks": np.ascontiguousarray(blocks), "x_ref": np.ascontiguousarray(x_ref)}


def realised(cfg: Mapping) -> Dict[str, np.ndarray]:
    """What Simulator.get_data adds: {"terminal_reference": [Nsim, 12], "terminal_blocks": [6, 3]} ({} without a terminal cost)."""
    if cfg.get(KEY) is None:
        return {}
    s = sample(cfg)
    return {"terminal_reference": s["x_ref"], "terminal_blocks": s["blocks"]}


def stack(cfgs) -> Tuple[np.ndarray, np.ndarray]:
    """The terminal costs of one launch: (blocks [B, 18] = pqq 6 | pqv 6 | pvv 6 of each simulation, x_ref [B, Nsim, 12]), as
    mpcb_rollout_term takes them (one Nsim per bucket)."""
    parts = [sample(c) for c in cfgs]
    blocks = np.stack([p["blocks"].T.reshape(18) for p in parts])
    return np.ascontiguousarray(blocks), np.ascontiguousarray(np.stack([p["x_ref"] for p in parts]))


def reference_from_run(data: Mapping, N: int) -> np.ndarray:
    """The table that closes a horizon of ``N`` stages around a logged run: row t = [q; qdot][:, min(t + N, Nsim)] of ``data``
    (Simulator.get_data(): "q" and "qdot" [6, Nsim + 1]) -- where the logged trajectory was N steps after step t, its last column
    held once the horizon reaches past the end of the run.  [Nsim, 12], float64."""
    q, qdot = np.asarray(data["q"], dtype=np.float64), np.asarray(data["qdot"], dtype=np.float64)
    if q.ndim != 2 or q.shape[0] != 6 or q.shape != qdot.shape or q.shape[1] < 2:
        raise ValueError(f"data['q'] and data['qdot'] must be [6, Nsim + 1], got {q.shape} and {qdot.shape}")
    if int(N) < 1:
        raise ValueError("N must be >= 1")
    nsim = q.shape[1] - 1
    cols = np.minimum(np.arange(nsim) + int(N), nsim)
    return np.ascontiguousarray(np.concatenate([q[:, cols], qdot[:, cols]], axis=0).T)
