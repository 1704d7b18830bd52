"""The configuration key surface_schedule and the entries mpcb_step_surf / mpcb_rollout_surf on the host (robotic_mpc_amd/surface.py,
config.py, packing.py, engine.py, simulator.py, distributed.py, results_io.py): the `moving` kind against direct evaluation of the
translated quadric, osculating_table against the height field it osculates, validation and every refusal, buckets, dotted grid keys,
the three host recomputations of the task errors against the per-column rows, the checkpoint round trip, two-rank gloo sharding
against the unsharded run, and the exports with their prototypes, ctypes declarations and documentation.  No device."""
import ctypes as C
import json
import os
import re
import shutil
import socket
import sys

import numpy as np
import pytest

from robotic_mpc_amd import analysis, config, packing, surface

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTI = {"nlp_solver_type": "SQP_RTI"}
MOVING = {"kind": "moving", "velocity": [0.1, -0.2, 0.05]}
TERM = {"weight": {"kind": "lqr", "q_weight": 10.0, "qdot_weight": 1.0, "r_weight": 1.0},
        "reference": {"kind": "constant", "value": [0.0] * 12}}


def _raw(**kw):
    return config.base_params(**{**dict(prediction_horizon=12, simulation_time=0.3, solver_options=RTI), **kw})


def _cfg(**kw):
    return config.resolve_config(_raw(**kw))


# ------------------------------------------------------------------------------------------------------------------ surface.py
def test_moving_is_the_translated_quadric_at_random_points():
    c = _cfg(surface_schedule=MOVING, surface_coeffs={"a": -0.2, "b": 0.1, "c": 0.05, "d": 0.03, "e": -0.02, "f": 0.4})
    rows = surface.sample(c)
    assert rows.shape == (c["Nsim"] + c["N"], 6) and rows.dtype == np.float64 and rows.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(rows[0], c["coeffs"])
    rng = np.random.default_rng(0)
    vx, vy, vz = MOVING["velocity"]
    for r in (0, 1, 7, 41):
        x, y = rng.uniform(-1, 1, 50), rng.uniform(-1, 1, 50)
        t = r * c["dt"]
        want = analysis.surface_value(c["coeffs"], x - vx * t, y - vy * t) + vz * t
        np.testing.assert_allclose(analysis.surface_value(rows[r], x, y), want, rtol=0, atol=1e-15)
    # the curvature does not move; the slope and the height do
    assert (rows[:, :3] == c["coeffs"][:3]).all() and (np.ptp(rows[:, 3:], axis=0) > 1e-3).all()
    np.testing.assert_array_equal(surface.log_rows(c), rows[:c["Nsim"] + 1])
    np.testing.assert_array_equal(surface.error_coeffs(c), rows[:c["Nsim"] + 1].T)
    assert surface.log_rows(_cfg()) is None
    np.testing.assert_array_equal(surface.error_coeffs(_cfg()), _cfg()["coeffs"])


def test_osculating_table_of_a_quadratic_is_that_quadratic_on_every_row():
    q = np.array([-0.15, 0.2, 0.03, 0.01, -0.04, 0.3])
    a, b, c, d, e, f = q
    path = np.random.default_rng(1).uniform(-1, 1, (9, 2))
    tab = surface.osculating_table(lambda x, y: analysis.surface_value(q, x, y), lambda x, y: (2 * a * x + c * y + d, 2 * b * y + c * x + e),
                                   lambda x, y: (2 * a, c, 2 * b), path)
    assert tab.shape == (9, 6)
    np.testing.assert_allclose(tab, np.tile(q, (9, 1)), rtol=0, atol=1e-15)


def test_osculating_table_of_a_cubic_matches_value_gradient_and_hessian_at_each_path_point():
    h = lambda x, y: 0.3 * x ** 3 - 0.2 * x * y ** 2 + 0.1 * y ** 3 + 0.05 * x * y + 0.2 * x - 0.1       # noqa: E731
    g = lambda x, y: (0.9 * x ** 2 - 0.2 * y ** 2 + 0.05 * y + 0.2, -0.4 * x * y + 0.3 * y ** 2 + 0.05 * x)   # noqa: E731
    H = lambda x, y: (1.8 * x, -0.4 * y + 0.05, -0.4 * x + 0.6 * y)                                            # noqa: E731
    path = np.random.default_rng(2).uniform(-0.8, 0.8, (7, 2))
    tab = surface.osculating_table(h, g, H, path)
    for (x0, y0), (a, b, c, d, e, f) in zip(path, tab):
        assert analysis.surface_value((a, b, c, d, e, f), x0, y0) == pytest.approx(h(x0, y0), abs=1e-15)
        np.testing.assert_allclose((2 * a * x0 + c * y0 + d, 2 * b * y0 + c * x0 + e), g(x0, y0), rtol=0, atol=1e-15)
        np.testing.assert_allclose((2 * a, c, 2 * b), H(x0, y0), rtol=0, atol=1e-15)
    assert np.ptp(tab[:, 0]) > 1e-2                      # a cubic's patches differ from point to point
    with pytest.raises(ValueError, match="xy_path"):
        surface.osculating_table(h, g, H, np.zeros((3, 3)))


def test_stack_pads_shorter_horizons_with_their_last_row():
    tab = lambda n: (np.arange(6.0)[None] + np.arange(n)[:, None]).tolist()      # noqa: E731
    a = _cfg(surface_schedule={"kind": "table", "rows": tab(42)})
    b = _cfg(prediction_horizon=8, surface_schedule={"kind": "table", "rows": tab(38)})
    s = surface.stack([a, b])
    assert s.shape == (2, 42, 6) and s.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(s[0], np.array(tab(42)))
    np.testing.assert_array_equal(s[1, :38], np.array(tab(38)))
    assert (s[1, 38:] == s[1, 37]).all()
    np.testing.assert_array_equal(surface.packed_rows(a, 3), np.tile(a["coeffs"], (3, 1)))


# ------------------------------------------------------------------------------------------------- validation and refusals
@pytest.mark.parametrize("spec", [0.2, {}, {"kind": "plane"}, {"kind": "table"}, {"kind": "table", "rows": [[0.0] * 5]},
                                  {"kind": "table", "rows": [[0.0] * 6], "extra": 1}, {"kind": "table", "rows": "abc"},
                                  {"kind": "table", "rows": [[float("nan")] * 6]}, {"kind": "moving"}, {"kind": "moving", "velocity": [0, 0]},
                                  {"kind": "moving", "velocity": [0, 0, float("inf")]}, {"kind": "moving", "velocity": "fast"},
                                  {"kind": "moving", "velocity": [0, 0, 0], "rows": []}, [1, 2, 3]])
def test_bad_specs_are_refused_with_the_keys_name(spec):
    with pytest.raises(ValueError, match="surface_schedule"):
        surface.validate(spec)
    with pytest.raises(ValueError, match="surface_schedule"):
        _cfg(surface_schedule=spec)


def test_a_table_needs_exactly_nsim_plus_n_rows():
    ok = {"kind": "table", "rows": [[0.0] * 6] * 42}
    assert _cfg(surface_schedule=ok)["surface_schedule"] == ok
    with pytest.raises(ValueError, match=r"surface_schedule needs exactly Nsim \+ N = 42 rows, got 41"):
        _cfg(surface_schedule={"kind": "table", "rows": [[0.0] * 6] * 41})


def test_the_key_resolves_defaults_to_none_and_combines():
    assert _cfg()["surface_schedule"] is None
    c = _cfg(surface_schedule=MOVING)
    assert c["surface_schedule"] == MOVING and c["surface_schedule"] is not MOVING
    serp = {"kind": "serpentine", "lanes": 2, "lane_pitch": 0.03, "lane_time": 0.1, "turn_time": 0.05}
    both = _cfg(surface_schedule=MOVING, reference_schedule=serp, plant_perturbation={"wcv_scale": 0.8})
    assert both["surface_schedule"] == MOVING and both["reference_schedule"] == serp and both["plant_perturbation"] == {"wcv_scale": 0.8}
    # the model's record does not see the key
    np.testing.assert_array_equal(packing.pack_params(c), packing.pack_params(_cfg()))


def test_terminal_cost_observer_full_sqp_fp32_and_the_host_buffer_path_refuse_the_key():
    from robotic_mpc_amd.engine import MpcBatchEngine

    with pytest.raises(ValueError, match="a surface_schedule is not offered together with a terminal_cost"):
        _cfg(surface_schedule=MOVING, terminal_cost=TERM)
    with pytest.raises(ValueError, match="a surface_schedule is not offered together with a disturbance_observer"):
        _cfg(surface_schedule=MOVING, disturbance_observer={"pole": 0.2})
    with pytest.raises(ValueError, match="a surface_schedule is offered with nlp_solver_type='SQP_RTI' only"):
        _cfg(surface_schedule=MOVING, solver_options={"nlp_solver_type": "SQP"})
    with pytest.raises(ValueError, match="a surface_schedule is offered with riccati_precision='fp64' only"):
        _cfg(surface_schedule=MOVING, riccati_precision="fp32")
    eng = object.__new__(MpcBatchEngine)                                      # no handle: the refusal comes first
    with pytest.raises(ValueError, match="mpcb_run takes no surface schedule.*surface_schedule"):
        MpcBatchEngine.run_host_buffers(eng, [_cfg(surface_schedule=MOVING)], None)
    with pytest.raises(ValueError, match=r"surface schedule \(surf\) is not offered together with a terminal cost \(term\)"):
        MpcBatchEngine.rollout(eng, {}, 0, 1, surf=object(), term={})
    with pytest.raises(ValueError, match=r"surface schedule \(surf\) is not offered together with a disturbance observer \(obs\)"):
        MpcBatchEngine.rollout(eng, {}, 0, 1, surf=object(), obs={})


# --------------------------------------------------------------------------------------------------------- buckets and grids
def test_bucket_key_separates_simulations_over_a_schedule_whatever_the_schedule():
    from robotic_mpc_amd import distributed
    from robotic_mpc_amd.engine import make_problem

    plain, a, b = _cfg(), _cfg(surface_schedule=MOVING), _cfg(surface_schedule={"kind": "moving", "velocity": [0, 0, 0.1]})
    p, both = _cfg(plant_perturbation={"wcv_scale": 0.9}), _cfg(plant_perturbation={"wcv_scale": 0.9}, surface_schedule=MOVING)
    assert packing.bucket_key(a) == packing.bucket_key(b)
    assert len({packing.bucket_key(c) for c in (plain, a, p, both, _cfg(terminal_cost=TERM), _cfg(disturbance_observer={"pole": 0.1}))}) == 6
    short = _cfg(surface_schedule=MOVING, prediction_horizon=8)
    assert packing.bucket_key(a) != packing.bucket_key(short) and packing.bucket_key(a, ragged=True) == packing.bucket_key(short, ragged=True)
    assert list(distributed.group_buckets([plain, a, plain, b, both]).values()) == [[0, 2], [1, 3], [4]]
    with pytest.raises(ValueError):
        make_problem([plain, a])


def test_dotted_grid_keys_reach_the_schedule_and_leave_the_base_untouched():
    from robotic_mpc_amd.simulator import SimulationManager

    base = _raw(surface_schedule={"kind": "moving", "velocity": [0.0, 0.0, 0.0]})
    vels = [[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.0, 0.0, 0.05]]
    mgr = SimulationManager(base)
    mgr.grid_search({"surface_schedule.velocity": vels, "prediction_horizon": [8, 12]})
    got = [(s["config"]["surface_schedule"]["velocity"], s["config"]["prediction_horizon"]) for s in mgr.simulations]
    assert got == [(v, N) for v in vels for N in (8, 12)]
    assert base["surface_schedule"]["velocity"] == [0.0, 0.0, 0.0] and mgr.base_config["surface_schedule"]["velocity"] == [0.0, 0.0, 0.0]
    assert len({id(s["config"]["surface_schedule"]) for s in mgr.simulations}) == 6
    resolved = [config.resolve_config(s["config"]) for s in mgr.simulations]
    assert len({packing.bucket_key(c, ragged=True) for c in resolved}) == 1 and len({packing.bucket_key(c) for c in resolved}) == 2
    st = surface.stack(resolved)
    assert st.shape == (6, 30 + 12, 6) and np.abs(st[1] - st[3]).max() > 1e-3
    # sweep() and add_manual() take the same dotted key
    m2 = SimulationManager(base)
    m2.sweep("surface_schedule.velocity", vels[1:])
    m2.add_manual("up", {"surface_schedule.velocity": [0.0, 0.0, 0.2]})
    assert [config.resolve_config(s["config"])["surface_schedule"]["velocity"] for s in m2.simulations] == vels[1:] + [[0.0, 0.0, 0.2]]


# -------------------------------------------------------------------------------------------------- host error recomputation
def _fake_runner(cfgs, chain):
    """Logs with a moving end effector and NO `errors` array: the sharding layer recomputes them (distributed.complete_runner_output)."""
    from robotic_mpc_amd.engine import RESULT_FIELDS

    S = cfgs[0]["Nsim"]
    out = {name: np.zeros((len(cfgs),) + shp(S, S + 1), dtype=np.float64 if ty == "f8" else np.int32) for name, ty, shp in RESULT_FIELDS
           if name not in ("errors", "plant_time")}
    t = np.arange(S + 1) * cfgs[0]["dt"]
    for i in range(len(cfgs)):
        out["ee_pose"][i, 0], out["ee_pose"][i, 1], out["ee_pose"][i, 2] = 0.4 + 0.1 * t, -0.2 + 0.3 * t, 0.1 * (i + 1) + 0.0 * t
        out["ee_pose"][i, 3], out["ee_pose"][i, 7], out["ee_pose"][i, 11] = 1.0, 1.0, 1.0
    return out


def _expected_errors(cfg, pose, vel):
    """Column t against row t, written out: the per-column loop the three sites must agree with."""
    rows = surface.sample(cfg)
    cols = []
    for t in range(cfg["Nsim"] + 1):
        e = analysis.compute_errors(pose[:, t:t + 1], vel[:, t:t + 1], rows[t], cfg["t_ee"], cfg["px_ref"], cfg["vy_ref"])
        cols.append(analysis.errors_rows(e)[:, 0])
    return np.stack(cols, axis=1)


def test_the_three_host_sites_measure_column_t_against_row_t(tmp_path):
    from robotic_mpc_amd import distributed, results_io
    from robotic_mpc_amd.simulator import SimulationManager, Simulator

    cfgs = [_cfg(surface_schedule=MOVING), _cfg(surface_schedule={"kind": "moving", "velocity": [0.0, 0.0, 0.3]})]
    out = _fake_runner(cfgs, None)
    want = [_expected_errors(c, out["ee_pose"][i], out["ee_vel"][i]) for i, c in enumerate(cfgs)]
    packed = analysis.errors_rows(analysis.compute_errors(out["ee_pose"][0], out["ee_vel"][0], cfgs[0]["coeffs"], cfgs[0]["t_ee"],
                                                           cfgs[0]["px_ref"], cfgs[0]["vy_ref"]))
    assert np.abs(packed - want[0]).max() > 1e-3                              # (the packed coefficients give other errors)
    # 1. distributed.complete_runner_output
    done = distributed.complete_runner_output(out, cfgs)
    for i in range(2):
        np.testing.assert_allclose(done["errors"][i], want[i], rtol=0, atol=1e-15)
    # 2. Simulator.errors from attached logs without an errors array; get_data()["surface_coeffs"]
    sim = Simulator(**_raw(surface_schedule=MOVING))
    sim._attach({k: v[0] for k, v in out.items()})
    np.testing.assert_allclose(analysis.errors_rows(sim.errors), want[0], rtol=0, atol=1e-15)
    rows = sim.get_data()["surface_coeffs"]
    assert rows.shape == (6, 31)
    np.testing.assert_array_equal(rows, surface.sample(cfgs[0])[:31].T)
    # 3. results_io.load_archive of a format-1 archive (no errors stored)
    path = str(tmp_path / "v1.npz")
    m = SimulationManager(_raw(), runner=_fake_runner)
    m.add_manual("moving", {"surface_schedule": MOVING})
    m.add_manual("plain")
    res = m.run_all(checkpoint=path)
    np.testing.assert_allclose(analysis.errors_rows(res[0]["simulator"].errors), want[0], rtol=0, atol=1e-15)
    assert "surface_coeffs" in res[0]["data"] and "surface_coeffs" not in res[1]["data"]
    with np.load(path, allow_pickle=False) as f:
        arch = {k: f[k] for k in f.files}
    arch = {k: v for k, v in arch.items() if k not in ("errors", "plant_time")}
    arch["format_version"] = np.int64(1)
    np.savez_compressed(path, **arch)
    old = results_io.load_archive(path)
    np.testing.assert_allclose(old["errors"][0], want[0], rtol=0, atol=1e-15)


def test_checkpoint_round_trip(tmp_path):
    from robotic_mpc_amd import results_io
    from robotic_mpc_amd.simulator import SimulationManager

    path = str(tmp_path / "surf.npz")
    vels = [[0.1, 0.0, 0.0], [0.0, 0.0, 0.05]]
    m = SimulationManager(_raw(surface_schedule={"kind": "moving", "velocity": [0.0, 0.0, 0.0]}), runner=_fake_runner)
    m.grid_search({"surface_schedule.velocity": vels})
    res = m.run_all(checkpoint=path)
    called = []
    m2 = SimulationManager(_raw(surface_schedule={"kind": "moving", "velocity": [0.0, 0.0, 0.0]}),
                           runner=lambda cfgs, chain: called.append(1) or _fake_runner(cfgs, chain))
    m2.grid_search({"surface_schedule.velocity": vels})
    again = m2.run_all(checkpoint=path)
    assert m2.last_run_info["n_resumed"] == 2 and not called
    loaded = results_io.load_results(path)
    for a, b, c, v in zip(res, again, loaded, vels):
        assert a["simulator"].resolved["surface_schedule"]["velocity"] == v == c["simulator"].resolved["surface_schedule"]["velocity"]
        np.testing.assert_array_equal(a["data"]["surface_coeffs"], b["data"]["surface_coeffs"])
        np.testing.assert_array_equal(a["data"]["surface_coeffs"], c["data"]["surface_coeffs"])
        for k in ("e1", "e2"):
            np.testing.assert_array_equal(a["simulator"].errors[k], c["simulator"].errors[k])
    assert np.abs(res[0]["data"]["surface_coeffs"] - res[1]["data"]["surface_coeffs"]).max() > 1e-3
    raw = _raw(surface_schedule=MOVING)
    assert json.loads(results_io.config_json(raw))["surface_schedule"] == MOVING
    assert results_io.resume_key("a", raw) != results_io.resume_key("a", _raw(surface_schedule={"kind": "moving", "velocity": [0, 0, 0]}))
    assert results_io.resume_key("a", raw) != results_io.resume_key("a", _raw())


# ----------------------------------------------------------------------------------------------------------- gloo sharding
def emu_runner(cfgs, chain):
    """A host runner that honours the schedule: the emulated latency-engine rollout (tests/emu/emu_rollsurf.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import emu_rollsurf
    from robotic_mpc_amd import reference

    rows = cfgs[0]["Nsim"] + cfgs[0]["N"]
    sched = np.stack([reference.packed_rows(c, rows) for c in cfgs])
    return emu_rollsurf.rollout(cfgs, chain, sched, surface.stack(cfgs), waves=4)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import torch.distributed as dist

    from robotic_mpc_amd import SimulationManager, base_params
    from test_surface_api import emu_runner

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        m = SimulationManager(base_params(prediction_horizon=5, simulation_time=0.06, solver_options={"nlp_solver_type": "SQP_RTI"},
                                          surface_schedule={"kind": "moving", "velocity": [0.0, 0.0, 0.0]}), runner=emu_runner)
        m.grid_search({"surface_schedule.velocity": [[0.0, 0.0, 0.0], [0.2, 0.0, 0.0], [0.0, 0.3, 0.1]]})     # one bucket of 3 over 2 ranks
        res = m.run_all(distributed=True)
        if rank == 0:
            single = m.run_all(distributed=False)
            assert [r["name"] for r in res] == [r["name"] for r in single] and len(res) == 3
            for a, b in zip(res, single):
                for k in ("q", "qdot", "u", "ee_pose", "surface_coeffs"):
                    assert np.array_equal(a["data"][k], b["data"][k]), (a["name"], k)
                for k in ("e1", "e2", "e4"):
                    assert np.array_equal(a["simulator"].errors[k], b["simulator"].errors[k]), (a["name"], k)
            assert np.abs(res[0]["data"]["q"] - res[2]["data"]["q"]).max() > 1e-6      # the schedule reaches the closed loop
            open(os.path.join(outdir, "ok"), "w").write("ok")
        else:
            assert res == []
    finally:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")
def test_two_rank_gloo_sharded_equals_unsharded(tmp_path):
    import torch.multiprocessing as mp

    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import emu_rollsurf

    emu_rollsurf.build()                                       # once, before two ranks would both try
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / "ok").exists()


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_the_new_entries_are_declared_exported_and_documented():
    from robotic_mpc_amd import build, engine

    build.build()
    lib = engine.load_library()
    text = open(os.path.join(ROOT, "include", "mpcbatch.h")).read()
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+mpcb_step_surf\s*\(\s*mpcb_handle\s*\*\s*\w+\s*,\s*const\s+mpcb_step_io\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,"
                     r"\s*int\s+\w+\s*,\s*const\s+int\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*void\s*\*\s*\w+\s*\)", body)
    assert re.search(r"\bint\s+mpcb_rollout_surf\s*\(\s*mpcb_handle\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+mpcb_result\s*\*\s*\w+\s*,"
                     r"\s*const\s+double\s*\*\s*\w+\s*,\s*const\s+mpcb_plant_pert\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,"
                     r"\s*void\s*\*\s*\w+\s*\)", body)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    for name in ("mpcb_step_surf", "mpcb_rollout_surf"):
        assert hasattr(lib, name) and name in engine._EXPORTS
    assert lib.mpcb_step_surf.argtypes == [C.c_void_p, C.POINTER(engine.MpcbStepIO), dp, C.c_int, ip, C.c_int, dp, C.c_int, C.c_void_p]
    assert lib.mpcb_rollout_surf.argtypes == [C.c_void_p, C.c_int, C.c_int, C.POINTER(engine.MpcbResult), dp,
                                              C.POINTER(engine.MpcbPlantPert), dp, C.c_void_p]
    for f in ("mpc_step_surf.hip", "mpc_stream_step_surf.hip", "mpc_rollout_surf.hip", "mpc_stream_rollout_surf.hip"):
        assert f in build.SOURCES and os.path.exists(os.path.join(build.CSRC, f))
    assert re.search(r"#define\s+MPCB_NSURF\s+6\b", text)
    step = text[text.index("a scheduled, stage-varying surface in the controller step"):text.index("int mpcb_step_surf")]
    for word in ("surf_changed != 0", "surf == NULL && surf_changed == 0 is mpcb_step_warm exactly", "MPCB_EINVAL", "MPCB_ESTATE",
                 "mpcb_step_sens", "mpcb_step_term", "mpcb_step_dist", "are not offered together"):
        assert word in step, word
    roll = text[text.index("rollouts over a scheduled, stage-varying surface"):text.index("int mpcb_rollout_surf")]
    for word in ("surf_sched[i][t + k]", "surface row t and reference row t", "mpcb_step_surf(xhat_t", "surf_sched == NULL is mpcb_rollout_pert exactly",
                 "every row equals the packed", "MPCB_EINVAL", "MPCB_ESTATE", "MPCB_PRECISION_FP32_RICCATI", "without yref_sched", "there is no shift",
                 "mpcb_workspace_bytes", "mpcb_kernel_info", "Not offered together", "profiles/rollout_surf_rate.txt"):
        assert word in roll, word
    assert "mpcb_rollout_surf" in text[text.rindex("/*", 0, text.index("int mpcb_queue_used")):text.index("int mpcb_queue_used")]
    # a null handle is refused before anything is read
    assert lib.mpcb_rollout_surf(None, 0, 1, None, None, None, None, None) == -1
    assert lib.mpcb_step_surf(None, None, None, 0, None, 0, None, 0, None) == -1


def test_the_workspace_is_what_it_was():
    """Nothing carries: (N + 1) x 696 stage doubles + the chunk transition matrices + 64 state doubles, as before."""
    from robotic_mpc_amd import build, engine

    build.build()
    lib = engine.load_library()
    for N in (1, 12, 100):
        pb = engine.MpcbProblem(3, N, 10, 1, 100, 50, 0, 0)
        per_sim = (N + 1) * 696 + ((N + 4) // 5 + 1) * 144 + 64
        assert lib.mpcb_workspace_bytes(C.byref(pb)) >= 3 * per_sim * 8
        assert lib.mpcb_workspace_bytes(C.byref(pb)) < 3 * (per_sim + 64) * 8
