"""Surface schedules for rollouts and controller steps (mpcb_rollout_surf, mpcb_step_surf): the configuration key
``surface_schedule`` -> the rows ``[Nsim + N, 6]`` of quadric coefficients ``a, b, c, d, e, f`` of
``S(x, y) = a x^2 + b y^2 + c x y + d x + e y + f`` the closed loop works on, row ``r`` at time ``r * dt``.  Stage ``k`` of closed-loop
step ``t`` uses row ``t + k``; column ``t`` of the error log is measured against row ``t``.

Two kinds of spec, both plain JSON:

``{"kind": "table", "rows": [[a..f], ...]}``
    the rows themselves, exactly ``Nsim + N`` of them.

``{"kind": "moving", "velocity": [vx, vy, vz]}``
    the simulation's own ``surface_coeffs`` translated rigidly at a constant velocity (m/s), a workpiece on a conveyor:
    ``S_r(x, y) = S(x - vx r dt, y - vy r dt) + vz r dt``, expanded in closed form into the six global coefficients.

A free-form surface is only locally a quadric: ``osculating_table`` hands it over patch by patch along a path.
"""
from __future__ import annotations

from typing import Any, Callable, Dict, Mapping

import numpy as np

NSURF = 6
KINDS = ("table", "moving")


def validate(spec: Any) -> None:
    """What can be said about a spec without the run length: its kind, its keys, the ranges of its numbers."""
    if not isinstance(spec, Mapping):
        raise ValueError("surface_schedule must be a dict with a 'kind' (or None)")
    kind = spec.get("kind")
    if kind not in KINDS:
        raise ValueError(f"surface_schedule kind must be one of {KINDS}, got {kind!r}")
    if kind == "table":
        extra = set(spec) - {"kind", "rows"}
        if extra or "rows" not in spec:
            raise ValueError(f"a 'table' surface_schedule has the keys 'kind' and 'rows' (got {sorted(spec)})")
        try:
            rows = np.asarray(spec["rows"], dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"surface_schedule rows must be numbers: {e}") from None
        if rows.ndim != 2 or rows.shape[1] != NSURF:
            raise ValueError(f"surface_schedule rows must be [rows][{NSURF}], got shape {rows.shape}")
        if not np.all(np.isfinite(rows)):
            raise ValueError("surface_schedule rows must be finite")
        return
    extra = set(spec) - {"kind", "velocity"}
    if extra or "velocity" not in spec:
        raise ValueError(f"a 'moving' surface_schedule has the keys 'kind' and 'velocity' (got {sorted(spec)})")
    try:
        v = np.asarray(spec["velocity"], dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"surface_schedule velocity must be numbers: {e}") from None
    if v.shape != (3,):
        raise ValueError(f"surface_schedule velocity must be [vx, vy, vz], got shape {v.shape}")
    if not np.all(np.isfinite(v)):
        raise ValueError("surface_schedule velocity must be finite")


def translated(coeffs, sx, sy, sz) -> np.ndarray:
    """The coefficients of ``S(x - sx, y - sy) + sz`` for S of ``coeffs`` = a..f; sx, sy, sz scalars or arrays [rows]: [..., 6]."""
    a, b, c, d, e, f = (float(v) for v in np.asarray(coeffs, dtype=np.float64).reshape(6))
    sx, sy, sz = np.broadcast_arrays(np.asarray(sx, dtype=np.float64), np.asarray(sy, dtype=np.float64), np.asarray(sz, dtype=np.float64))
    out = np.empty(sx.shape + (NSURF,))
    out[..., 0] = a
    out[..., 1] = b
    out[..., 2] = c
    out[..., 3] = d - 2.0 * a * sx - c * sy
    out[..., 4] = e - 2.0 * b * sy - c * sx
    out[..., 5] = a * sx * sx + b * sy * sy + c * sx * sy - d * sx - e * sy + f + sz
    return out


def sample(cfg: Dict) -> np.ndarray:
    """The schedule of a resolved configuration (config.resolve_config) that carries one: [Nsim + N, 6] float64."""
    spec = cfg.get("surface_schedule")
    if spec is None:
        raise ValueError("this configuration has no surface_schedule")
    validate(spec)
    rows = int(cfg["Nsim"]) + int(cfg["N"])
    if spec["kind"] == "table":
        y = np.array(spec["rows"], dtype=np.float64)
        if y.shape[0] != rows:
            raise ValueError(f"a 'table' surface_schedule needs exactly Nsim + N = {rows} rows, got {y.shape[0]}")
        return np.ascontiguousarray(y)
    v = np.asarray(spec["velocity"], dtype=np.float64)
    t = np.arange(rows) * float(cfg["dt"])
    return np.ascontiguousarray(translated(cfg["coeffs"], v[0] * t, v[1] * t, v[2] * t))


def log_rows(cfg: Dict):
    """The rows the error log is measured against, [Nsim + 1, 6] (analysis.compute_errors coeffs=), or None without a schedule."""
    if cfg.get("surface_schedule") is None:
        return None
    return sample(cfg)[:int(cfg["Nsim"]) + 1]


def error_coeffs(cfg: Dict):
    """What analysis.compute_errors takes as `coeffs` for this configuration: the packed six, or with a schedule the rows of the
    logged columns as [6, Nsim + 1] (a..f unpack into one array per column each)."""
    rows = log_rows(cfg)
    return cfg["coeffs"] if rows is None else np.ascontiguousarray(rows.T)


def packed_rows(cfg: Dict, rows: int) -> np.ndarray:
    """The constant schedule that is the packed surface on every row."""
    return np.tile(np.asarray(cfg["coeffs"], dtype=np.float64).reshape(6), (rows, 1))


def stack(cfgs) -> np.ndarray:
    """The schedules of one launch: [batch, Nsim + Nmax, 6], Nmax the longest horizon of the bucket.  A simulation of a shorter
    horizon never reads past row Nsim + N_i - 1; its remaining rows hold its last one."""
    nmax = max(int(c["N"]) for c in cfgs)
    rows = int(cfgs[0]["Nsim"]) + nmax
    out = np.empty((len(cfgs), rows, NSURF))
    for i, c in enumerate(cfgs):
        y = sample(c)
        out[i, :y.shape[0]] = y
        out[i, y.shape[0]:] = y[-1]
    return out


def osculating_table(height: Callable, grad: Callable, hess: Callable, xy_path) -> np.ndarray:
    """The second-order Taylor patch of a free-form height field z = h(x, y) at each point of a path, in GLOBAL coefficients a..f:
    row r is the quadric that agrees with h in value, gradient and Hessian at xy_path[r] = (x_r, y_r).

    ``height(x, y) -> h``, ``grad(x, y) -> (hx, hy)``, ``hess(x, y) -> (hxx, hxy, hyy)``.  Returns [rows, 6] -- the rows of a
    ``{"kind": "table"}`` spec when the path has Nsim + N points, e.g. the tool path of a ``serpentine`` reference."""
    path = np.asarray(xy_path, dtype=np.float64)
    if path.ndim != 2 or path.shape[1] != 2:
        raise ValueError(f"xy_path must be [rows][2], got shape {path.shape}")
    out = np.empty((path.shape[0], NSURF))
    for r, (x0, y0) in enumerate(path):
        h = float(height(x0, y0))
        hx, hy = (float(v) for v in grad(x0, y0))
        hxx, hxy, hyy = (float(v) for v in hess(x0, y0))
        # h + hx (x - x0) + hy (y - y0) + 1/2 hxx (x - x0)^2 + hxy (x - x0)(y - y0) + 1/2 hyy (y - y0)^2, collected in x, y
        out[r] = (0.5 * hxx, 0.5 * hyy, hxy,
                  hx - hxx * x0 - hxy * y0,
                  hy - hyy * y0 - hxy * x0,
                  h - hx * x0 - hy * y0 + 0.5 * hxx * x0 * x0 + hxy * x0 * y0 + 0.5 * hyy * y0 * y0)
    return out
