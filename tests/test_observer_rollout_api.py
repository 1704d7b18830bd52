"""The configuration key disturbance_observer and the rollout entry mpcb_rollout_obs on the host (robotic_mpc_amd/observer.py,
config.py, packing.py, engine.py, simulator.py, results_io.py): observer_gains against the class, validation and the four refusals,
buckets, the dotted grid key, d_hat through a runner into get_data() and through the checkpoint, and the export with its prototype
and ctypes declaration.  No device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from robotic_mpc_amd import config, observer, packing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTI = {"nlp_solver_type": "SQP_RTI"}
OBS = {"pole": 0.2}
TERM = {"weight": {"kind": "lqr", "q_weight": 10.0, "qdot_weight": 1.0, "r_weight": 1.0},
        "reference": {"kind": "constant", "value": [0.0] * 12}}


def _raw(**kw):
    return config.base_params(**{**dict(prediction_horizon=12, simulation_time=0.3, solver_options=RTI), **kw})


def _cfg(**kw):
    return config.resolve_config(_raw(**kw))


# ------------------------------------------------------------------------------------------------------------------ the gains
@pytest.mark.parametrize("pole", [0.0, 0.2, 0.9])
def test_observer_gains_are_the_gains_of_the_class(pole):
    import torch

    wcv = np.array([[200.0, 150.0, 100.0, 50.0, 20.0, 5.0], [10.0] * 6])
    obs = observer.DisturbanceObserver(wcv, 0.01, pole=pole)
    l1, l2 = observer.observer_gains(wcv, 0.01, pole)
    assert isinstance(l1, np.ndarray) and l1.shape == (2, 6) and l2.shape == (2, 6) and l1.dtype == np.float64
    # (numpy's exp and torch's may differ in the last bit: the class calls the function with its tensor, compared exactly below)
    np.testing.assert_allclose(l1, obs.l1.numpy(), rtol=1e-15)
    np.testing.assert_allclose(l2, obs.l2.numpy(), rtol=1e-15)
    a22 = np.exp(-wcv * 0.01)
    np.testing.assert_allclose(l1, a22 + 1 - 2 * pole, rtol=1e-15)
    np.testing.assert_allclose(l2, (1 - pole) ** 2 / (1 - a22), rtol=1e-15)
    # both poles of A - L C sit at `pole`
    M = obs.error_matrix().numpy().reshape(-1, 2, 2)
    for m in M:
        np.testing.assert_allclose(np.abs(np.linalg.eigvals(m)), pole, atol=2e-7)
    # a tensor in, tensors out
    t1, t2 = observer.observer_gains(torch.from_numpy(wcv), 0.01, pole)
    assert isinstance(t1, torch.Tensor) and t1.dtype == torch.float64
    np.testing.assert_array_equal(t1.numpy(), obs.l1.numpy())
    np.testing.assert_array_equal(t2.numpy(), obs.l2.numpy())
    with pytest.raises(ValueError, match="pole"):
        observer.observer_gains(wcv, 0.01, 1.0)
    with pytest.raises(ValueError, match="dt"):
        observer.observer_gains(wcv, 0.0, 0.5)


def test_stack_is_l1_then_l2_of_each_simulations_own_model():
    cfgs = [_cfg(disturbance_observer={"pole": 0.0}), _cfg(disturbance_observer={"pole": 0.5}, wcv=[100.0] * 6, dt=0.02, simulation_time=0.6)]
    g = observer.stack(cfgs)
    assert g.shape == (2, 12) and g.dtype == np.float64 and g.flags["C_CONTIGUOUS"]
    for i, c in enumerate(cfgs):
        l1, l2 = observer.observer_gains(c["wcv"], c["dt"], c["disturbance_observer"]["pole"])
        np.testing.assert_array_equal(g[i, :6], l1)
        np.testing.assert_array_equal(g[i, 6:], l2)
    assert np.abs(g[0] - g[1]).min() > 0


# ------------------------------------------------------------------------------------------------- validation and refusals
@pytest.mark.parametrize("spec", [0.2, {"pole": 1.0}, {"pole": -0.1}, {"pole": "fast"}, {"pole": None}, {}, {"pole": 0.2, "gain": 1.0},
                                  [0.2], {"pole": float("nan")}])
def test_bad_specs_are_refused_with_the_keys_name(spec):
    with pytest.raises(ValueError, match="disturbance_observer"):
        observer.validate(spec)
    with pytest.raises(ValueError, match="disturbance_observer"):
        _cfg(disturbance_observer=spec)


def test_the_key_resolves_and_defaults_to_none():
    assert _cfg()["disturbance_observer"] is None
    for p in (0, 0.0, 0.2, 0.999):
        c = _cfg(disturbance_observer={"pole": p})
        assert c["disturbance_observer"] == {"pole": float(p)} and isinstance(c["disturbance_observer"]["pole"], float)
    spec = {"pole": 0.3}
    assert _cfg(disturbance_observer=spec)["disturbance_observer"] is not spec
    # with and without a perturbed plant
    assert _cfg(disturbance_observer=OBS, plant_perturbation={"wcv_scale": 0.8})["disturbance_observer"] == OBS
    # the model's record does not see the key
    np.testing.assert_array_equal(packing.pack_params(_cfg(disturbance_observer=OBS)), packing.pack_params(_cfg()))


def test_terminal_cost_full_sqp_fp32_and_the_host_buffer_path_refuse_the_key():
    from robotic_mpc_amd.engine import MpcBatchEngine

    with pytest.raises(ValueError, match="a disturbance_observer is not offered together with a terminal_cost"):
        _cfg(disturbance_observer=OBS, terminal_cost=TERM)
    with pytest.raises(ValueError, match="a disturbance_observer is offered with nlp_solver_type='SQP_RTI' only"):
        _cfg(disturbance_observer=OBS, solver_options={"nlp_solver_type": "SQP"})
    with pytest.raises(ValueError, match="a disturbance_observer is offered with riccati_precision='fp64' only"):
        _cfg(disturbance_observer=OBS, riccati_precision="fp32")
    eng = object.__new__(MpcBatchEngine)                                      # no handle: the refusal comes first
    with pytest.raises(ValueError, match="mpcb_run takes no disturbance observer.*disturbance_observer"):
        MpcBatchEngine.run_host_buffers(eng, [_cfg(disturbance_observer=OBS)], None)
    with pytest.raises(ValueError, match="not offered together with a terminal cost"):
        MpcBatchEngine.rollout(eng, {}, 0, 1, obs={}, term={})


# ------------------------------------------------------------------------------------------ buckets, grid, runner, checkpoint
def test_bucket_key_separates_simulations_with_an_observer_whatever_their_pole():
    from robotic_mpc_amd import distributed
    from robotic_mpc_amd.engine import make_problem

    pert = {"wcv_scale": 0.9}
    plain, a, b = _cfg(), _cfg(disturbance_observer={"pole": 0.0}), _cfg(disturbance_observer={"pole": 0.7})
    p, both = _cfg(plant_perturbation=pert), _cfg(plant_perturbation=pert, disturbance_observer=OBS)
    assert packing.bucket_key(a) == packing.bucket_key(b)
    assert len({packing.bucket_key(c) for c in (plain, a, p, both, _cfg(terminal_cost=TERM))}) == 5
    short = _cfg(disturbance_observer=OBS, prediction_horizon=8)
    assert packing.bucket_key(a) != packing.bucket_key(short) and packing.bucket_key(a, ragged=True) == packing.bucket_key(short, ragged=True)
    assert list(distributed.group_buckets([plain, a, plain, b, both]).values()) == [[0, 2], [1, 3], [4]]
    with pytest.raises(ValueError):
        make_problem([plain, a])


def test_dotted_grid_key_reaches_the_pole_and_leaves_the_base_untouched():
    from robotic_mpc_amd.simulator import SimulationManager

    base = _raw(disturbance_observer={"pole": 0.5}, plant_perturbation={"wcv_scale": 0.8})
    mgr = SimulationManager(base)
    mgr.grid_search({"disturbance_observer.pole": [0.0, 0.2, 0.6], "prediction_horizon": [8, 12]})
    got = [(s["config"]["disturbance_observer"]["pole"], s["config"]["prediction_horizon"]) for s in mgr.simulations]
    assert got == [(p, N) for p in (0.0, 0.2, 0.6) for N in (8, 12)]
    assert base["disturbance_observer"] == {"pole": 0.5} and mgr.base_config["disturbance_observer"] == {"pole": 0.5}
    assert len({id(s["config"]["disturbance_observer"]) for s in mgr.simulations}) == 6
    resolved = [config.resolve_config(s["config"]) for s in mgr.simulations]
    assert len({packing.bucket_key(c, ragged=True) for c in resolved}) == 1 and len({packing.bucket_key(c) for c in resolved}) == 2
    g = observer.stack(resolved)
    assert np.abs(g[0] - g[2]).min() > 0 and (g[0] == g[1]).all()             # the horizon does not enter the gains
    # from a base without the key, too
    m2 = SimulationManager(_raw())
    m2.grid_search({"disturbance_observer.pole": [0.1, 0.3]})
    assert [config.resolve_config(s["config"])["disturbance_observer"] for s in m2.simulations] == [{"pole": 0.1}, {"pole": 0.3}]


def _fake_runner(cfgs, chain):
    """Logs of zeros, and for a bucket with observers d_hat[i, t, j] = 100 pole_i + t + j / 10."""
    from robotic_mpc_amd.engine import RESULT_FIELDS

    S = cfgs[0]["Nsim"]
    out = {name: np.zeros((len(cfgs),) + shp(S, S + 1), dtype=np.float64 if ty == "f8" else np.int32) for name, ty, shp in RESULT_FIELDS}
    if cfgs[0]["disturbance_observer"] is not None:
        out["d_hat"] = np.stack([100.0 * c["disturbance_observer"]["pole"] + np.arange(S)[:, None] + np.arange(6)[None, :] / 10 for c in cfgs])
    return out


def test_d_hat_travels_from_the_runner_to_get_data_and_through_the_checkpoint(tmp_path):
    from robotic_mpc_amd import results_io
    from robotic_mpc_amd.simulator import SimulationManager

    path = str(tmp_path / "obs.npz")
    m = SimulationManager(_raw(), runner=_fake_runner)
    m.grid_search({"disturbance_observer.pole": [0.1, 0.3]})
    m.add_manual("plain")                                                   # a simulation without the key, in the same archive
    res = m.run_all(checkpoint=path)
    assert [r["name"] for r in res] == ["pole=0.1", "pole=0.3", "plain"]
    for r, p in zip(res[:2], (0.1, 0.3)):
        d = r["data"]["d_hat"]
        assert d.shape == (6, 30)
        np.testing.assert_array_equal(d, (100.0 * p + np.arange(30)[:, None] + np.arange(6)[None, :] / 10).T)
        np.testing.assert_array_equal(r["simulator"].get_data()["d_hat"], d)
    assert "d_hat" not in res[2]["data"]
    # the archive holds it, and a resumed run returns it without running
    arch = results_io.load_archive(path)
    assert arch["d_hat"].shape == (3, 30, 6) and arch["has_d_hat"].tolist() == [1, 1, 0]
    called = []
    m2 = SimulationManager(_raw(), runner=lambda cfgs, chain: called.append(1) or _fake_runner(cfgs, chain))
    m2.grid_search({"disturbance_observer.pole": [0.1, 0.3]})
    m2.add_manual("plain")
    again = m2.run_all(checkpoint=path)
    assert m2.last_run_info["n_resumed"] == 3 and not called
    for a, b in zip(res[:2], again[:2]):
        np.testing.assert_array_equal(a["data"]["d_hat"], b["data"]["d_hat"])
    assert "d_hat" not in again[2]["data"]
    loaded = results_io.load_results(path)
    np.testing.assert_array_equal(loaded[1]["data"]["d_hat"], res[1]["data"]["d_hat"])
    assert "d_hat" not in loaded[2]["data"]
    # the config round trip of the resume key
    raw = _raw(disturbance_observer=OBS)
    assert json.loads(results_io.config_json(raw))["disturbance_observer"] == OBS
    assert results_io.resume_key("a", raw) != results_io.resume_key("a", _raw(disturbance_observer={"pole": 0.3}))
    assert results_io.resume_key("a", raw) != results_io.resume_key("a", _raw())


def test_an_archive_without_observers_has_no_d_hat(tmp_path):
    from robotic_mpc_amd import results_io
    from robotic_mpc_amd.simulator import SimulationManager

    path = str(tmp_path / "plain.npz")
    m = SimulationManager(_raw(), runner=_fake_runner)
    m.add_manual("plain")
    m.run_all(checkpoint=path)
    assert "d_hat" not in results_io.load_archive(path)


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_the_new_entry_is_declared_and_exported():
    from robotic_mpc_amd import build, engine

    build.build()
    lib = engine.load_library()
    text = open(os.path.join(ROOT, "include", "mpcbatch.h")).read()
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+mpcb_rollout_obs\s*\(\s*mpcb_handle\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+mpcb_result\s*\*\s*\w+\s*,"
                     r"\s*const\s+double\s*\*\s*\w+\s*,\s*const\s+mpcb_plant_pert\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,"
                     r"\s*double\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)", body)
    assert hasattr(lib, "mpcb_rollout_obs") and "mpcb_rollout_obs" in engine._EXPORTS
    # header <-> ctypes: handle, step0, step1, out, yref_sched, pert, obs_gain, d_hat, stream
    dp = C.POINTER(C.c_double)
    assert lib.mpcb_rollout_obs.argtypes == [C.c_void_p, C.c_int, C.c_int, C.POINTER(engine.MpcbResult), dp,
                                             C.POINTER(engine.MpcbPlantPert), dp, dp, C.c_void_p]
    for f in ("mpc_rollout_obs.hip", "mpc_stream_rollout_obs.hip"):
        assert f in build.SOURCES and os.path.exists(os.path.join(build.CSRC, f))
    doc = text[text.index("rollouts with an on-device disturbance observer"):text.index("int mpcb_rollout_obs")]
    for word in ("mpcb_step_dist", "obs_gain == NULL", "MPCB_EINVAL", "MPCB_ESTATE", "d_hat", "mpcb_workspace_bytes"):
        assert word in doc
    assert "nor a rollout with an on-device observer" not in text
    # a null handle is refused before anything is read
    assert lib.mpcb_rollout_obs(None, 0, 1, None, None, None, None, None, None) == -1


def test_the_observers_slots_fit_the_state_block_and_the_workspace_is_what_it_was():
    """ST_OBS = 48 .. 59 of the 64 state doubles, past the profile counters: the workspace per simulation has not grown."""
    from robotic_mpc_amd import build, engine

    build.build()
    lib = engine.load_library()
    text = open(os.path.join(build.CSRC, "mpc_layout.h")).read()
    val = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))   # noqa: E731
    assert val("ST_OBS") >= val("ST_PROF") + val("NPROF") and val("ST_OBS") + 12 <= val("STATE_DOUBLES") == 64
    # (N + 1) x 696 stage doubles + the chunk transition matrices + 64 state doubles, as before
    for N in (1, 12, 100):
        pb = engine.MpcbProblem(3, N, 10, 1, 100, 50, 0, 0)
        per_sim = (N + 1) * 696 + ((N + 4) // 5 + 1) * 144 + 64
        assert lib.mpcb_workspace_bytes(C.byref(pb)) >= 3 * per_sim * 8
        assert lib.mpcb_workspace_bytes(C.byref(pb)) < 3 * (per_sim + 64) * 8
