"""Task reference schedules for rollouts (mpcb_rollout_ref): the configuration key ``reference_schedule`` -> the rows
``[Nsim + N, 5]`` of targets of the task outputs g1..g5 the closed loop tracks, row ``r`` at time ``r * dt``.

Two kinds of spec, both plain JSON:

``{"kind": "table", "rows": [[y0..y4], ...]}``
    the rows themselves, exactly ``Nsim + N`` of them.

``{"kind": "serpentine", "lanes": L, "lane_pitch": m, "lane_time": s, "turn_time": s}``
    the coverage path the reference project's surface.py sketches: L lanes along y, traversed in alternating direction at
    ``vy_ref``, ``lane_pitch`` apart in x from ``px_ref``, joined by smooth turns.  Columns 0..2 stay 0, 1, 0.
"""
from __future__ import annotations

from typing import Any, Dict, Mapping

import numpy as np

NREF = 5
KINDS = ("table", "serpentine")
_SERPENTINE_KEYS = ("lanes", "lane_pitch", "lane_time", "turn_time")


def validate(spec: Any) -> None:
    """What can be said about a spec without the run length: its kind, its keys, the ranges of its numbers."""
    if not isinstance(spec, Mapping):
        raise ValueError("reference_schedule must be a dict with a 'kind' (or None)")
    kind = spec.get("kind")
    if kind not in KINDS:
        raise ValueError(f"reference_schedule kind must be one of {KINDS}, got {kind!r}")
    if kind == "table":
        extra = set(spec) - {"kind", "rows"}
        if extra or "rows" not in spec:
            raise ValueError(f"a 'table' reference_schedule has the keys 'kind' and 'rows' (got {sorted(spec)})")
        try:
            rows = np.asarray(spec["rows"], dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"reference_schedule rows must be numbers: {e}") from None
        if rows.ndim != 2 or rows.shape[1] != NREF:
            raise ValueError(f"reference_schedule rows must be [rows][{NREF}], got shape {rows.shape}")
        if not np.all(np.isfinite(rows)):
            raise ValueError("reference_schedule rows must be finite")
        return
    extra = set(spec) - {"kind", *_SERPENTINE_KEYS}
    missing = [k for k in _SERPENTINE_KEYS if k not in spec]
    if extra or missing:
        raise ValueError(f"a 'serpentine' reference_schedule has the keys {('kind',) + _SERPENTINE_KEYS} (got {sorted(spec)})")
    lanes = spec["lanes"]
    if isinstance(lanes, bool) or not isinstance(lanes, (int, np.integer)) or lanes < 1:
        raise ValueError("reference_schedule lanes must be an integer >= 1")
    for k in ("lane_time", "turn_time"):
        v = _number(spec, k)
        if not v > 0:
            raise ValueError(f"reference_schedule {k} must be > 0")
    _number(spec, "lane_pitch")


def _number(spec: Mapping, key: str) -> float:
    try:
        v = float(spec[key])
    except (TypeError, ValueError):
        raise ValueError(f"reference_schedule {key} must be a number") from None
    if not np.isfinite(v):
        raise ValueError(f"reference_schedule {key} must be finite")
    return v


def sample(cfg: Dict) -> np.ndarray:
    """The schedule of a resolved configuration (config.resolve_config) that carries one: [Nsim + N, 5] float64."""
    spec = cfg.get("reference_schedule")
    if spec is None:
        raise ValueError("this configuration has no reference_schedule")
    validate(spec)
    rows = int(cfg["Nsim"]) + int(cfg["N"])
    if spec["kind"] == "table":
        y = np.array(spec["rows"], dtype=np.float64)
        if y.shape[0] != rows:
            raise ValueError(f"a 'table' reference_schedule needs exactly Nsim + N = {rows} rows, got {y.shape[0]}")
        return np.ascontiguousarray(y)
    L, pitch = int(spec["lanes"]), float(spec["lane_pitch"])
    lane_time, turn_time = float(spec["lane_time"]), float(spec["turn_time"])
    px_ref, vy_ref = float(cfg["px_ref"]), float(cfg["vy_ref"])
    t = np.arange(rows) * float(cfg["dt"])
    period = lane_time + turn_time
    m = np.minimum(np.floor(t / period), L - 1)
    into = t - m * period                                          # time since lane m began
    turning = (into >= lane_time) & (m < L - 1)
    tau = np.where(turning, (into - lane_time) / turn_time, 0.0)   # in [0, 1)
    s = 3.0 * tau ** 2 - 2.0 * tau ** 3
    sign = np.where(m % 2 == 0, 1.0, -1.0)
    y = np.zeros((rows, NREF))
    y[:, 1] = 1.0
    y[:, 3] = px_ref + (m + s) * pitch
    y[:, 4] = sign * vy_ref * (1.0 - 2.0 * s)
    return y


def log_rows(cfg: Dict):
    """The rows the error log is measured against, [Nsim + 1, 5] (analysis.compute_errors yref=), or None without a schedule."""
    if cfg.get("reference_schedule") is None:
        return None
    return sample(cfg)[:int(cfg["Nsim"]) + 1]


def packed_rows(cfg: Dict, rows: int) -> np.ndarray:
    """The constant schedule that is the packed reference [0, 1, 0, px_ref, vy_ref] on every row."""
    return np.tile(np.array([0.0, 1.0, 0.0, float(cfg["px_ref"]), float(cfg["vy_ref"])]), (rows, 1))


def stack(cfgs) -> np.ndarray:
    """The schedules of one launch: [batch, Nsim + Nmax, 5], Nmax the longest horizon of the bucket.  A simulation of a shorter
    horizon never reads past row Nsim + N_i - 1; its remaining rows hold its last one."""
    nmax = max(int(c["N"]) for c in cfgs)
    rows = int(cfgs[0]["Nsim"]) + nmax
    out = np.empty((len(cfgs), rows, NREF))
    for i, c in enumerate(cfgs):
        y = sample(c)
        out[i, :y.shape[0]] = y
        out[i, y.shape[0]:] = y[-1]
    return out
