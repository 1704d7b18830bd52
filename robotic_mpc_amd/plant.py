"""Plant perturbations for rollouts (mpcb_rollout_pert): the configuration key ``plant_perturbation`` -> what makes the rollout's
built-in plant differ from the model the controller predicts with.  A plain JSON spec with three optional parts:

``{"wcv_scale": 1.0 | [6],``
    the plant's actuator bandwidths are ``wcv * wcv_scale`` (the model keeps ``wcv``);

`` "input_disturbance": None | {"kind": "table", "rows": [Nsim][6]} | {"kind": "step", "start_time": s, "value": x | [6]}``
``                           | {"kind": "gaussian", "sigma": x | [6], "seed": int},``
    added to the commanded input ``u_t`` before the plant step of step ``t`` (row ``t`` at time ``t * dt``);

`` "measurement_noise": None | {"kind": "table", "rows": [Nsim][12]}``
``                           | {"kind": "gaussian", "sigma_q": x | [6], "sigma_qdot": x | [6], "seed": int}}``
    added to the true plant state ``z_t = [q; qdot]`` to form the feedback state of step ``t``.

Gaussian rows are ``numpy.random.default_rng([seed, k]).standard_normal(shape) * sigma`` with ``k = 0`` for the disturbance and
``k = 1`` for the noise: a function of the spec alone, so every rank and every resume draws the same table.
"""
from __future__ import annotations

from typing import Any, Dict, Mapping

import numpy as np

KEY = "plant_perturbation"
NU, NX = 6, 12
_TOP_KEYS = ("wcv_scale", "input_disturbance", "measurement_noise")
_DIST_KEYS = {"table": ("rows",), "step": ("start_time", "value"), "gaussian": ("sigma", "seed")}
_NOISE_KEYS = {"table": ("rows",), "gaussian": ("sigma_q", "sigma_qdot", "seed")}
_STREAM = {"input_disturbance": 0, "measurement_noise": 1}


def _vector(value: Any, n: int, name: str, positive: bool = False, nonneg: bool = False) -> np.ndarray:
    """A scalar or [n] numbers -> [n] float64."""
    if isinstance(value, (bool, str)) or value is None:
        raise ValueError(f"{KEY} {name} must be a number or {n} numbers")
    try:
        v = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{KEY} {name} must be a number or {n} numbers") from None
    if v.ndim == 0:
        v = np.full(n, float(v))
    if v.shape != (n,):
        raise ValueError(f"{KEY} {name} must be a number or {n} numbers, got shape {v.shape}")
    if not np.all(np.isfinite(v)):
        raise ValueError(f"{KEY} {name} must be finite")
    if positive and not np.all(v > 0):
        raise ValueError(f"{KEY} {name} must be > 0")
    if nonneg and not np.all(v >= 0):
        raise ValueError(f"{KEY} {name} must be >= 0")
    return v


def _seed(part: Mapping, name: str) -> int:
    s = part["seed"]
    if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or s < 0:
        raise ValueError(f"{KEY} {name}.seed must be an integer >= 0")
    return int(s)


def _rows(part: Mapping, width: int, name: str) -> np.ndarray:
    try:
        rows = np.asarray(part["rows"], dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{KEY} {name}.rows must be numbers: {e}") from None
    if rows.ndim != 2 or rows.shape[1] != width:
        raise ValueError(f"{KEY} {name}.rows must be [Nsim][{width}], got shape {rows.shape}")
    if not np.all(np.isfinite(rows)):
        raise ValueError(f"{KEY} {name}.rows must be finite")
    return rows


def _validate_part(part: Any, name: str, kinds: Mapping, width: int) -> None:
    if part is None:
        return
    if not isinstance(part, Mapping):
        raise ValueError(f"{KEY} {name} must be a dict with a 'kind' (or None)")
    kind = part.get("kind")
    if kind not in kinds:
        raise ValueError(f"{KEY} {name}.kind must be one of {tuple(kinds)}, got {kind!r}")
    want = ("kind",) + kinds[kind]
    if set(part) != set(want):
        raise ValueError(f"a {kind!r} {KEY} {name} has the keys {want} (got {sorted(part)})")
    if kind == "table":
        _rows(part, width, name)
    elif kind == "step":
        st = part["start_time"]
        if isinstance(st, (bool, str)) or st is None or np.ndim(st) != 0 or not np.isfinite(float(st)) or float(st) < 0:
            raise ValueError(f"{KEY} {name}.start_time must be a number >= 0")
        _vector(part["value"], width, f"{name}.value")
    else:
        for k in kinds[kind]:
            if k != "seed":
                _vector(part[k], 6, f"{name}.{k}", nonneg=True)
        _seed(part, name)


def validate(spec: Any) -> None:
    """What can be said about a spec without the run length: its keys, its kinds, the ranges of its numbers."""
    if not isinstance(spec, Mapping):
        raise ValueError(f"{KEY} must be a dict (or None)")
    extra = set(spec) - set(_TOP_KEYS)
    if extra:
        raise ValueError(f"{KEY} has the keys {_TOP_KEYS} (got {sorted(spec)})")
    _vector(spec.get("wcv_scale", 1.0), NU, "wcv_scale", positive=True)
    _validate_part(spec.get("input_disturbance"), "input_disturbance", _DIST_KEYS, NU)
    _validate_part(spec.get("measurement_noise"), "measurement_noise", _NOISE_KEYS, NX)


def _table(part: Any, name: str, width: int, nsim: int, dt: float) -> np.ndarray:
    if part is None:
        return np.zeros((nsim, width))
    kind = part["kind"]
    if kind == "table":
        rows = _rows(part, width, name)
        if rows.shape[0] != nsim:
            raise ValueError(f"a 'table' {KEY} {name} needs exactly Nsim = {nsim} rows, got {rows.shape[0]}")
        return np.ascontiguousarray(rows)
    if kind == "step":
        # row t acts at time t * dt: on from the first row at or after start_time
        on = np.arange(nsim) * dt >= float(part["start_time"]) - 1e-12
        return on[:, None] * _vector(part["value"], width, f"{name}.value")[None, :]
    rng = np.random.default_rng([_seed(part, name), _STREAM[name]])
    if name == "input_disturbance":
        sigma = _vector(part["sigma"], NU, f"{name}.sigma", nonneg=True)
    else:
        sigma = np.concatenate([_vector(part["sigma_q"], 6, f"{name}.sigma_q", nonneg=True),
                                _vector(part["sigma_qdot"], 6, f"{name}.sigma_qdot", nonneg=True)])
    return rng.standard_normal((nsim, width)) * sigma[None, :]


def sample(cfg: Dict) -> Dict[str, np.ndarray]:
    """The realised perturbation of a resolved configuration (config.resolve_config) that carries one:
    {"wcv": [6] the plant's bandwidths, "u_dist": [Nsim, 6], "x_noise": [Nsim, 12]}, float64."""
    spec = cfg.get(KEY)
    if spec is None:
        raise ValueError(f"this configuration has no {KEY}")
    validate(spec)
    nsim, dt = int(cfg["Nsim"]), float(cfg["dt"])
    wcv = np.asarray(cfg["wcv"], dtype=np.float64).reshape(NU) * _vector(spec.get("wcv_scale", 1.0), NU, "wcv_scale", positive=True)
    return {"wcv": wcv, "u_dist": _table(spec.get("input_disturbance"), "input_disturbance", NU, nsim, dt),
            "x_noise": _table(spec.get("measurement_noise"), "measurement_noise", NX, nsim, dt)}


def realised(cfg: Dict):
    """What Simulator.get_data adds: {"input_disturbance": [Nsim, 6]} and {"measurement_noise": [Nsim, 12]} for the parts that are
    configured ({} without a perturbation)."""
    spec = cfg.get(KEY)
    if spec is None:
        return {}
    s = sample(cfg)
    out = {}
    if spec.get("input_disturbance") is not None:
        out["input_disturbance"] = s["u_dist"]
    if spec.get("measurement_noise") is not None:
        out["measurement_noise"] = s["x_noise"]
    return out


def stack(cfgs) -> Dict[str, np.ndarray]:
    """The perturbations of one launch: {"wcv": [B, 6], "u_dist": [B, Nsim, 6], "x_noise": [B, Nsim, 12]} (one Nsim per bucket)."""
    parts = [sample(c) for c in cfgs]
    return {k: np.ascontiguousarray(np.stack([p[k] for p in parts])) for k in ("wcv", "u_dist", "x_noise")}
