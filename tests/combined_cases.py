"""Inputs shared by the combined-feature tests (emulation, API and GPU): raw configurations with combine_features in which every
simulation uses its own SUBSET of terminal cost, disturbance observer, surface schedule and shift warm start.

The draws are test_gpu_rollout_pert._raw's (initial state, px_ref, perturbed plant with a step input disturbance of 0.05 rad/s from a
third of the run on, bandwidth scale, measurement noise); on top of them simulation i gets the features of SUBSETS[i % len(SUBSETS)]:
  term   an LQR terminal cost (q 10, qdot 1, r 1) around a TABLE of terminal references off the iterate: x_e[t] = [q_0 + 0.05 (1 +
         0.1 t) s_i; 0], s_i a fixed sign pattern -- a new x_e at every step
  obs    a disturbance observer with pole 0.2
  surf   the seeded surface table of test_gpu_rollout_surf._raw (curvature, slope and offset all move)
  shift  warm_start = "shift"
The first two subsets are all four and none."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FEATURES = ("term", "obs", "surf", "shift")
SUBSETS = (FEATURES, (), ("term",), ("obs",), ("surf",), ("shift",), ("term", "shift"), ("obs", "surf"))
SIGNS = np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0])


def raw(n, N, steps, seed, subsets=SUBSETS, **kw):
    import step_surf_cases as ss
    import test_gpu_rollout_pert as tp

    out = tp._raw(n, N, steps, seed=seed, **kw)
    for i, r in enumerate(out):
        use = subsets[i % len(subsets)]
        r["combine_features"] = True
        if "term" in use:
            q0 = np.asarray(r["q_0"], dtype=np.float64)
            rows = [np.concatenate([q0 + 0.05 * (1.0 + 0.1 * t) * SIGNS * (1 if i % 2 == 0 else -1), np.zeros(6)]).tolist() for t in range(steps)]
            r["terminal_cost"] = {"weight": {"kind": "lqr", "q_weight": 10.0, "qdot_weight": 1.0, "r_weight": 1.0},
                                  "reference": {"kind": "table", "rows": rows}}
        if "obs" in use:
            r["disturbance_observer"] = {"pole": 0.2}
        if "surf" in use:
            nrows = steps + int(r["prediction_horizon"])
            base = np.array([r["surface_coeffs"][k] for k in "abcdef"])
            r["surface_schedule"] = {"kind": "table", "rows": (base[None] + ss.variation(nrows, 2000 + 10 * seed + i)).tolist()}
        if "shift" in use:
            r["warm_start"] = "shift"
    return out


def uses(cfg):
    """The features a resolved configuration uses, as a tuple of FEATURES."""
    return tuple(f for f, on in zip(FEATURES, (cfg.get("terminal_cost") is not None, cfg.get("disturbance_observer") is not None,
                                               cfg.get("surface_schedule") is not None, cfg.get("warm_start") == "shift")) if on)


def resolve(raws):
    from robotic_mpc_amd import config

    return [config.resolve_config(r) for r in raws]


def guards(cfgs, want, without, check=None):
    """From the reference loops alone (`want`: the loop; `without[f]`: the same loop with feature f switched off): every step has
    status 0, and for each feature a simulation with N >= 2 uses the loop without it ends more than 1e-4 away in z -- no feature is a
    passenger.  (With N = 1 the surface and the shift cannot reach u0: test_gpu_rollout_surf / _shift say why; not asserted there.)"""
    idx = list(range(len(cfgs))) if check is None else list(check)
    assert (want["status"] == 0).all()
    for f, loop in without.items():
        assert (loop["status"] == 0).all(), f
        for i in idx:
            if f in uses(cfgs[i]) and cfgs[i]["N"] >= 2:
                d = np.abs(loop["z"][i] - want["z"][i]).max()
                assert d > 1e-4, (f, i, d)
