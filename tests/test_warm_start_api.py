"""The configuration key warm_start ("carry" | "shift") and the C entry mpcb_rollout_warm, without a device: validation and refusal
messages, grids, buckets, sharding, checkpoints, the prototype, its ctypes declaration and its header text."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from robotic_mpc_amd import config, packing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTI = {"nlp_solver_type": "SQP_RTI"}
TERM = {"weight": {"kind": "lqr", "q_weight": 10.0, "qdot_weight": 1.0, "r_weight": 1.0},
        "reference": {"kind": "constant", "value": [0.0] * 12}}


def _raw(**kw):
    return config.base_params(**{**dict(prediction_horizon=12, simulation_time=0.3, solver_options=RTI), **kw})


def _cfg(**kw):
    return config.resolve_config(_raw(**kw))


# ------------------------------------------------------------------------------------------------------------------- the key
def test_the_key_defaults_to_carry_and_resolves():
    assert config.EXTENSION_DEFAULTS["warm_start"] == "carry" and config.WARM_STARTS == ("carry", "shift")
    assert _cfg()["warm_start"] == "carry" and _cfg(warm_start="carry")["warm_start"] == "carry"
    c = _cfg(warm_start="shift", plant_perturbation={"wcv_scale": 0.9}, surface_schedule={"kind": "moving", "velocity": [0.1, 0.0, 0.0]},
             reference_schedule={"kind": "serpentine", "lanes": 2, "lane_pitch": 0.03, "lane_time": 0.04, "turn_time": 0.05})
    assert c["warm_start"] == "shift" and c["surface_schedule"] is not None and c["plant_perturbation"] is not None
    assert _cfg(warm_start="shift", prediction_horizon=1)["N"] == 1             # a horizon of one is legal


@pytest.mark.parametrize("bad", ["Shift", "reset", "", None, 2, True, ["shift"]])
def test_other_values_are_refused_with_the_keys_name(bad):
    with pytest.raises(ValueError, match="warm_start"):
        _cfg(warm_start=bad)


def test_full_sqp_fp32_terminal_cost_observer_and_the_host_buffer_path_refuse_shift():
    from robotic_mpc_amd.engine import MpcBatchEngine

    with pytest.raises(ValueError, match=r"warm_start='shift' is offered with nlp_solver_type='SQP_RTI' only"):
        _cfg(warm_start="shift", solver_options={"nlp_solver_type": "SQP"})
    with pytest.raises(ValueError, match=r"warm_start='shift' is offered with riccati_precision='fp64' only"):
        _cfg(warm_start="shift", riccati_precision="fp32")
    with pytest.raises(ValueError, match=r"warm_start='shift' is not offered together with a terminal_cost"):
        _cfg(warm_start="shift", terminal_cost=TERM)
    with pytest.raises(ValueError, match=r"warm_start='shift' is not offered together with a disturbance_observer"):
        _cfg(warm_start="shift", disturbance_observer={"pole": 0.2})
    # "carry" goes with all of them, as it did before the key existed
    for kw in (dict(solver_options={"nlp_solver_type": "SQP"}), dict(riccati_precision="fp32"), dict(terminal_cost=TERM),
               dict(disturbance_observer={"pole": 0.2})):
        assert _cfg(warm_start="carry", **kw)["warm_start"] == "carry"
    eng = object.__new__(MpcBatchEngine)
    with pytest.raises(ValueError, match="mpcb_run takes no warm-start modes"):
        MpcBatchEngine.run_host_buffers(eng, [_cfg(warm_start="shift")], None)
    with pytest.raises(ValueError, match=r"\(warm\) is not offered together with a terminal cost \(term\)"):
        MpcBatchEngine.rollout(eng, {}, 0, 1, warm=object(), term={})
    with pytest.raises(ValueError, match=r"\(warm\) is not offered together with a disturbance observer \(obs\)"):
        MpcBatchEngine.rollout(eng, {}, 0, 1, warm=object(), obs={})


# --------------------------------------------------------------------------------------------------------- buckets and grids
def test_the_mode_is_per_simulation_not_per_bucket():
    from robotic_mpc_amd import distributed, engine

    a, b = _cfg(), _cfg(warm_start="shift")
    assert packing.bucket_key(a) == packing.bucket_key(b)
    cfgs = [a, b, _cfg(w_u=0.002), _cfg(w_u=0.002, warm_start="shift"), _cfg(prediction_horizon=8, warm_start="shift")]
    assert list(distributed.group_buckets(cfgs, merge_ragged=False).values()) == [[0, 1, 2, 3], [4]]
    np.testing.assert_array_equal(engine.warm_modes(cfgs[:4]), np.array([0, 2, 0, 2], np.int32))
    assert engine.warm_modes(cfgs[:4]).dtype == np.int32
    assert engine.warm_modes([a, cfgs[2]]) is None                               # every simulation carries: the path it took before
    assert (engine.WARM_CARRY, engine.WARM_SHIFT) == (0, 2)
    engine.make_problem(cfgs[:4])                                                # one problem for the mixed bucket


def test_plain_and_dotted_grid_keys_expand_and_leave_the_base_untouched():
    from robotic_mpc_amd.simulator import SimulationManager

    base = _raw(plant_perturbation={"wcv_scale": 1.0})
    mgr = SimulationManager(base)
    mgr.grid_search({"warm_start": ["carry", "shift"], "plant_perturbation.wcv_scale": [0.8, 1.2], "w_u": [0.01, 0.002]})
    got = [(s["config"]["warm_start"], s["config"]["plant_perturbation"]["wcv_scale"], s["config"]["w_u"]) for s in mgr.simulations]
    assert got == [(w, s, u) for w in ("carry", "shift") for s in (0.8, 1.2) for u in (0.01, 0.002)]
    assert "warm_start" not in base or base["warm_start"] == "carry"
    resolved = [config.resolve_config(s["config"]) for s in mgr.simulations]
    assert len({packing.bucket_key(c) for c in resolved}) == 1
    m2 = SimulationManager(base)
    m2.sweep("warm_start", ["shift", "carry"])
    m2.add_manual("shifted", {"warm_start": "shift"})
    assert [config.resolve_config(s["config"])["warm_start"] for s in m2.simulations] == ["shift", "carry", "shift"]
    with pytest.raises(ValueError, match="warm_start"):
        m3 = SimulationManager(base)
        m3.add_manual("bad", {"warm_start": "sideways"})
        [config.resolve_config(s["config"]) for s in m3.simulations]


def test_sharding_keeps_the_modes_with_their_simulations():
    """What each rank hands its runner is a slice of the bucket: the modes are read from that slice's own configurations."""
    from robotic_mpc_amd import distributed, engine

    order = ["carry", "shift", "shift", "carry", "carry", "carry", "shift"]
    cfgs = [_cfg(warm_start=w, w_u=0.01 + 0.001 * i) for i, w in enumerate(order)]
    (idxs,) = distributed.group_buckets(cfgs, 3).values()
    assert idxs == list(range(7))
    full = engine.warm_modes(cfgs)
    seen = []
    for lo, hi in distributed.chunk_bounds(len(idxs), 3):
        mine = [cfgs[i] for i in idxs[lo:hi]]
        m = engine.warm_modes(mine)
        if m is None:
            assert all(c["warm_start"] == "carry" for c in mine)
            m = np.zeros(len(mine), np.int32)
        seen.append(m)
        assert [("shift" if v == 2 else "carry") for v in m] == [c["warm_start"] for c in mine]
    np.testing.assert_array_equal(np.concatenate(seen), full)


def _fake_runner(seen):
    def run(cfgs, chain):
        from robotic_mpc_amd import engine
        from robotic_mpc_amd.engine import RESULT_FIELDS

        seen.append(engine.warm_modes(cfgs))
        S = cfgs[0]["Nsim"]
        out = {name: np.zeros((len(cfgs),) + shp(S, S + 1), dtype=np.float64 if ty == "f8" else np.int32) for name, ty, shp in RESULT_FIELDS}
        for i, c in enumerate(cfgs):
            out["z"][i] += 1.0 if c["warm_start"] == "shift" else 0.0            # (a runner that honours the mode)
        return out
    return run


def test_run_all_hands_one_bucket_with_its_modes_to_the_runner_and_checkpoints_carry_the_key(tmp_path):
    from robotic_mpc_amd import results_io
    from robotic_mpc_amd.simulator import SimulationManager

    path = str(tmp_path / "warm.npz")
    seen = []
    m = SimulationManager(_raw(), runner=_fake_runner(seen))
    m.grid_search({"warm_start": ["carry", "shift"], "w_u": [0.01, 0.002]})
    res = m.run_all(checkpoint=path)
    assert m.last_run_info["buckets"] == 1 and len(seen) == 1
    np.testing.assert_array_equal(seen[0], np.array([0, 0, 2, 2], np.int32))
    assert [r["simulator"].resolved["warm_start"] for r in res] == ["carry", "carry", "shift", "shift"]
    assert [float(r["data"]["q"].max()) for r in res] == [0.0, 0.0, 1.0, 1.0]
    # resume: nothing runs again, and the key comes back with its simulation
    again_seen = []
    m2 = SimulationManager(_raw(), runner=_fake_runner(again_seen))
    m2.grid_search({"warm_start": ["carry", "shift"], "w_u": [0.01, 0.002]})
    again = m2.run_all(checkpoint=path)
    assert m2.last_run_info["n_resumed"] == 4 and not again_seen
    loaded = results_io.load_results(path)
    for a, b, c in zip(res, again, loaded):
        assert a["simulator"].resolved["warm_start"] == b["simulator"].resolved["warm_start"] == c["simulator"].resolved["warm_start"]
        np.testing.assert_array_equal(a["data"]["q"], c["data"]["q"])
    raw = _raw(warm_start="shift")
    assert json.loads(results_io.config_json(raw))["warm_start"] == "shift"
    assert results_io.resume_key("a", raw) != results_io.resume_key("a", _raw())
    # a checkpoint of the other mode is not taken for this one
    m3 = SimulationManager(_raw(), runner=_fake_runner([]))
    m3.grid_search({"warm_start": ["shift"], "w_u": [0.01, 0.002]})
    m3.run_all(checkpoint=str(tmp_path / "other.npz"))
    m4 = SimulationManager(_raw(), runner=_fake_runner([]))
    m4.grid_search({"warm_start": ["carry"], "w_u": [0.01, 0.002]})
    m4.run_all(checkpoint=str(tmp_path / "other.npz"))
    assert m4.last_run_info["n_resumed"] == 0


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_the_new_entry_is_declared_exported_and_documented():
    from robotic_mpc_amd import build, engine

    build.build()
    lib = engine.load_library()
    text = open(os.path.join(ROOT, "include", "mpcbatch.h")).read()
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+mpcb_rollout_warm\s*\(\s*mpcb_handle\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+mpcb_result\s*\*\s*\w+\s*,"
                     r"\s*const\s+double\s*\*\s*\w+\s*,\s*const\s+mpcb_plant_pert\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,"
                     r"\s*const\s+int\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)", body)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    assert hasattr(lib, "mpcb_rollout_warm") and "mpcb_rollout_warm" in engine._EXPORTS
    assert lib.mpcb_rollout_warm.argtypes == [C.c_void_p, C.c_int, C.c_int, C.POINTER(engine.MpcbResult), dp,
                                              C.POINTER(engine.MpcbPlantPert), dp, ip, C.c_void_p]
    for f in ("mpc_rollout_shift.hip", "mpc_stream_rollout_shift.hip"):
        assert f in build.SOURCES and os.path.exists(os.path.join(build.CSRC, f))
    roll = text[text.index("rollouts with the shift warm start"):text.index("int mpcb_rollout_warm")]
    for word in ("mpcb_step_warm(xhat_t", "t >= 1 ? mode_i : MPCB_WARM_CARRY", "mpcb_step_surf", "absolute step number",
                 "warm == NULL is mpcb_rollout_surf exactly", "mpcb_rollout_pert", "other than MPCB_WARM_SHIFT counts", "MPCB_EINVAL",
                 "MPCB_ESTATE", "MPCB_PRECISION_FP32_RICCATI", "without yref_sched", "full-SQP", "x_N <- Ad x_N + Bd u_{N-1}", "N = 1 legal",
                 "mpcb_workspace_bytes", "mpcb_queue_used", "mpcb_last_kernel_ms", "mpcb_kernel_info", "Not offered together",
                 "mpcb_rollout_term", "mpcb_rollout_obs", "profiles/rollout_shift_rate.txt"):
        assert word in roll, word
    assert "mpcb_rollout_warm" in text[text.rindex("/*", 0, text.index("int mpcb_queue_used")):text.index("int mpcb_queue_used")]
    assert os.path.exists(os.path.join(ROOT, "profiles", "rollout_shift_rate.txt"))
    assert os.path.exists(os.path.join(ROOT, "profiles", "rollout_shift_closed_loop.txt"))
    # a null handle is refused before anything is read
    assert lib.mpcb_rollout_warm(None, 0, 1, None, None, None, None, None, None) == -1


def test_the_workspace_is_what_it_was():
    """Nothing new carries: the workspace bound of the other rollouts holds."""
    from robotic_mpc_amd import build, engine

    build.build()
    lib = engine.load_library()
    for N in (1, 12, 100):
        pb = engine.MpcbProblem(3, N, 10, 1, 100, 50, 0, 0)
        per_sim = (N + 1) * 696 + ((N + 4) // 5 + 1) * 144 + 64
        assert lib.mpcb_workspace_bytes(C.byref(pb)) >= 3 * per_sim * 8
