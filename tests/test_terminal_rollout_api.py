"""The configuration key terminal_cost and the rollout entry mpcb_rollout_term on the host (robotic_mpc_amd/terminal.py, config.py,
packing.py, engine.py): validation and refusals, stack, reference_from_run, buckets, dotted grid keys, the checkpoint's config round
trip, and the export with its prototype and ctypes declaration.  No device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from robotic_mpc_amd import config, packing, terminal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LQR = {"kind": "lqr", "q_weight": 10.0, "qdot_weight": 1.0, "r_weight": 1.0}
XE = [0.1 * i for i in range(12)]
CONST = {"kind": "constant", "value": XE}
SPEC = {"weight": LQR, "reference": CONST}
RTI = {"nlp_solver_type": "SQP_RTI"}


def _cfg(**kw):
    return config.resolve_config(config.base_params(**{**dict(prediction_horizon=12, simulation_time=0.3, solver_options=RTI), **kw}))


def _blocks(pqq=2.0, pqv=0.5, pvv=1.0):
    return [[pqq, pqv, pvv]] * 6


# ------------------------------------------------------------------------------------------------------------- validation
@pytest.mark.parametrize("spec,word", [
    ([1.0], "terminal_cost must be a dict"),
    ({"weight": LQR}, "terminal_cost has the keys"),
    ({"weight": LQR, "reference": CONST, "horizon": 3}, "terminal_cost has the keys"),
    ({"weight": 3.0, "reference": CONST}, "weight must be a dict"),
    ({"weight": {"kind": "dare"}, "reference": CONST}, "weight.kind"),
    ({"weight": {"kind": "lqr", "q_weight": 1.0, "r_weight": 1.0}, "reference": CONST}, "'lqr' terminal_cost weight has the keys"),
    ({"weight": dict(LQR, q_weight=[1.0] * 5), "reference": CONST}, "weight.q_weight"),
    ({"weight": dict(LQR, q_weight=float("nan")), "reference": CONST}, "weight.q_weight must be finite"),
    ({"weight": dict(LQR, r_weight=0.0), "reference": CONST}, "r_weight > 0"),
    ({"weight": dict(LQR, q_weight=0.0, qdot_weight=0.0), "reference": CONST}, "q_weight \\+ qdot_weight > 0"),
    ({"weight": {"kind": "blocks", "blocks": [[1.0, 0.0, 1.0]] * 5}, "reference": CONST}, "weight.blocks must be \\[6\\]\\[3\\]"),
    ({"weight": {"kind": "blocks", "blocks": _blocks(pqq=float("inf"))}, "reference": CONST}, "weight.blocks must be finite"),
    ({"weight": {"kind": "blocks", "blocks": _blocks(pqq=-1.0)}, "reference": CONST}, "positive semidefinite"),
    ({"weight": {"kind": "blocks", "blocks": _blocks(pqq=1.0, pqv=1.5, pvv=1.0)}, "reference": CONST}, "positive semidefinite"),
    ({"weight": {"kind": "blocks", "blocks": _blocks(), "scale": 2}, "reference": CONST}, "'blocks' terminal_cost weight has the keys"),
    ({"weight": LQR, "reference": {"kind": "spline"}}, "reference.kind"),
    ({"weight": LQR, "reference": {"kind": "constant", "value": [0.0] * 6}}, "reference.value must be 12 numbers"),
    ({"weight": LQR, "reference": {"kind": "constant", "value": [float("nan")] * 12}}, "reference.value must be finite"),
    ({"weight": LQR, "reference": {"kind": "constant", "rows": [[0.0] * 12]}}, "'constant' terminal_cost reference has the keys"),
    ({"weight": LQR, "reference": {"kind": "table", "rows": [[0.0] * 6] * 30}}, "reference.rows must be \\[Nsim\\]\\[12\\]"),
    ({"weight": LQR, "reference": {"kind": "table", "rows": "all"}}, "reference.rows"),
])
def test_bad_specs_are_refused_with_the_keys_name_when_the_config_is_resolved(spec, word):
    with pytest.raises(ValueError, match=word):
        terminal.validate(spec)
    with pytest.raises(ValueError, match=word):
        _cfg(terminal_cost=spec)


def test_table_row_count_is_checked_against_the_run_length():
    assert _cfg()["Nsim"] == 30
    rows = np.arange(30 * 12, dtype=np.float64).reshape(30, 12)
    s = terminal.sample(_cfg(terminal_cost={"weight": LQR, "reference": {"kind": "table", "rows": rows.tolist()}}))
    np.testing.assert_array_equal(s["x_ref"], rows)
    for n in (29, 31):
        with pytest.raises(ValueError, match=f"reference needs exactly Nsim = 30 rows, got {n}"):
            _cfg(terminal_cost={"weight": LQR, "reference": {"kind": "table", "rows": np.zeros((n, 12)).tolist()}})


def test_full_sqp_fp32_and_the_host_buffer_path_refuse_the_key():
    from robotic_mpc_amd.engine import MpcBatchEngine

    with pytest.raises(ValueError, match="a terminal_cost is offered with nlp_solver_type='SQP_RTI' only"):
        _cfg(terminal_cost=SPEC, solver_options={"nlp_solver_type": "SQP"})
    with pytest.raises(ValueError, match="a terminal_cost is offered with riccati_precision='fp64' only"):
        _cfg(terminal_cost=SPEC, riccati_precision="fp32")
    assert _cfg()["terminal_cost"] is None and terminal.realised(_cfg()) == {}
    with pytest.raises(ValueError, match="no terminal_cost"):
        terminal.sample(_cfg())
    eng = object.__new__(MpcBatchEngine)                                      # no handle: the refusal comes first
    with pytest.raises(ValueError, match="mpcb_run takes no terminal cost"):
        MpcBatchEngine.run_host_buffers(eng, [_cfg(terminal_cost=SPEC)], None)


# ------------------------------------------------------------------------------------------------- sample, stack, the table
def test_sample_is_the_lqr_design_of_the_configurations_own_model():
    raw = config.base_params(prediction_horizon=12, simulation_time=0.3, solver_options=RTI, terminal_cost=SPEC)
    s = terminal.sample(config.resolve_config(raw))
    want = terminal.lqr_terminal(config.base_params(prediction_horizon=12, simulation_time=0.3), 10.0, 1.0, 1.0)["blocks"]
    np.testing.assert_array_equal(s["blocks"], want)
    assert s["blocks"].shape == (6, 3) and 400 < s["blocks"][0, 0] < 500      # pqq ~ 456
    assert s["x_ref"].shape == (30, 12) and (s["x_ref"] == np.asarray(XE)[None, :]).all()
    # per-joint weights, and a slower model has another cost-to-go
    v = terminal.sample(_cfg(terminal_cost={"weight": dict(LQR, r_weight=[1, 2, 3, 4, 5, 6]), "reference": CONST}))["blocks"]
    np.testing.assert_array_equal(v[0], s["blocks"][0])
    assert (np.diff(v[:, 0]) > 0).all()
    slow = terminal.sample(_cfg(terminal_cost=SPEC, wcv=[100.0] * 6))["blocks"]
    assert np.abs(slow - s["blocks"]).max() > 1.0
    # given blocks pass through
    b = np.array(_blocks()) * np.arange(1.0, 7.0)[:, None]
    given = terminal.sample(_cfg(terminal_cost={"weight": {"kind": "blocks", "blocks": b.tolist()}, "reference": CONST}))
    np.testing.assert_array_equal(given["blocks"], b)
    r = terminal.realised(_cfg(terminal_cost=SPEC))
    assert sorted(r) == ["terminal_blocks", "terminal_reference"]
    assert r["terminal_reference"].shape == (30, 12) and r["terminal_blocks"].shape == (6, 3)


def test_stack_orders_the_blocks_as_the_device_record_and_a_chunk_is_the_stack_of_its_configs():
    from robotic_mpc_amd import distributed

    cfgs = []
    for i in range(5):
        b = (np.array(_blocks()) * (1.0 + i)) + np.arange(6.0)[:, None] * np.array([1.0, 0.0, 1.0])[None, :]
        rows = np.full((30, 12), float(i)) + np.arange(30.0)[:, None]
        cfgs.append(_cfg(terminal_cost={"weight": {"kind": "blocks", "blocks": b.tolist()}, "reference": {"kind": "table", "rows": rows.tolist()}}))
    blocks, x_ref = terminal.stack(cfgs)
    assert blocks.shape == (5, 18) and x_ref.shape == (5, 30, 12) and blocks.flags["C_CONTIGUOUS"] and x_ref.flags["C_CONTIGUOUS"]
    assert blocks.dtype == np.float64 and x_ref.dtype == np.float64
    for i, c in enumerate(cfgs):
        b = terminal.sample(c)["blocks"]
        np.testing.assert_array_equal(blocks[i, 0:6], b[:, 0])                # pqq 6 | pqv 6 | pvv 6
        np.testing.assert_array_equal(blocks[i, 6:12], b[:, 1])
        np.testing.assert_array_equal(blocks[i, 12:18], b[:, 2])
        assert x_ref[i, 7, 3] == i + 7.0
    for rank in range(2):
        for idxs in distributed.group_buckets(cfgs, 2).values():
            lo, hi = distributed.chunk_bounds(len(idxs), 2)[rank]
            mine = list(idxs[lo:hi])
            pb, px = terminal.stack([cfgs[i] for i in mine])
            np.testing.assert_array_equal(pb, blocks[mine])
            np.testing.assert_array_equal(px, x_ref[mine])


def test_reference_from_run_reads_the_log_a_horizon_ahead_and_holds_its_last_column():
    S = 9
    q = np.arange(6.0)[:, None] * 100 + np.arange(S + 1.0)[None, :]           # q[j, t] = 100 j + t
    qdot = -q
    tab = terminal.reference_from_run({"q": q, "qdot": qdot}, 4)
    assert tab.shape == (S, 12) and tab.flags["C_CONTIGUOUS"] and tab.dtype == np.float64
    for t in range(S):
        col = min(t + 4, S)
        np.testing.assert_array_equal(tab[t, :6], q[:, col])
        np.testing.assert_array_equal(tab[t, 6:], qdot[:, col])
    np.testing.assert_array_equal(tab[5], tab[8])                             # rows 5 .. 8 hold column Nsim
    assert (tab[4] != tab[5]).all()
    # a horizon beyond the run: every row is the last column
    np.testing.assert_array_equal(terminal.reference_from_run({"q": q, "qdot": qdot}, 50), np.tile(tab[8], (S, 1)))
    # ... and it is a table the key takes for a run of that length
    c = _cfg(simulation_time=0.09 + 1e-9, terminal_cost={"weight": LQR, "reference": {"kind": "table", "rows": tab.tolist()}})
    np.testing.assert_array_equal(terminal.sample(c)["x_ref"], tab)
    with pytest.raises(ValueError, match="Nsim \\+ 1"):
        terminal.reference_from_run({"q": q[:5], "qdot": qdot[:5]}, 4)
    with pytest.raises(ValueError, match="N must be >= 1"):
        terminal.reference_from_run({"q": q, "qdot": qdot}, 0)


# ------------------------------------------------------------------------------------------ config, buckets, grid, checkpoint
def test_config_key_survives_json_and_the_checkpoints_config_round_trip():
    from robotic_mpc_amd import results_io

    raw = config.base_params(terminal_cost=SPEC, prediction_horizon=12, simulation_time=0.3, solver_options=RTI)
    c = config.resolve_config(raw)
    assert c["terminal_cost"] == SPEC and c["terminal_cost"] is not SPEC and c["terminal_cost"]["weight"] is not LQR
    back = json.loads(results_io.config_json(raw))
    assert back["terminal_cost"] == SPEC
    for k, v in terminal.sample(config.resolve_config(back)).items():
        np.testing.assert_array_equal(v, terminal.sample(c)[k])
    other = config.base_params(terminal_cost={"weight": dict(LQR, r_weight=2.0), "reference": CONST}, prediction_horizon=12,
                               simulation_time=0.3, solver_options=RTI)
    assert results_io.resume_key("a", raw) != results_io.resume_key("a", other)
    assert results_io.resume_key("a", raw) != results_io.resume_key("a", config.base_params(prediction_horizon=12, simulation_time=0.3,
                                                                                        solver_options=RTI))
    # the model's record does not see the key
    np.testing.assert_array_equal(packing.pack_params(c), packing.pack_params(_cfg()))


def test_bucket_key_separates_simulations_with_a_terminal_cost():
    from robotic_mpc_amd import distributed
    from robotic_mpc_amd.engine import make_problem

    pert = {"wcv_scale": 0.9}
    plain, term, term2 = _cfg(), _cfg(terminal_cost=SPEC), _cfg(terminal_cost={"weight": dict(LQR, r_weight=3.0), "reference": CONST})
    p, both = _cfg(plant_perturbation=pert), _cfg(plant_perturbation=pert, terminal_cost=SPEC)
    assert packing.bucket_key(term) == packing.bucket_key(term2)              # the spec itself is per-simulation data
    assert len({packing.bucket_key(c) for c in (plain, term, p, both)}) == 4
    assert len({packing.bucket_key(c, ragged=True) for c in (plain, term, p, both)}) == 4
    short = _cfg(terminal_cost=SPEC, prediction_horizon=8)
    assert packing.bucket_key(term) != packing.bucket_key(short) and packing.bucket_key(term, ragged=True) == packing.bucket_key(short, ragged=True)
    assert list(distributed.group_buckets([plain, term, plain, term2, both]).values()) == [[0, 2], [1, 3], [4]]
    with pytest.raises(ValueError):
        make_problem([plain, term])


def test_dotted_grid_keys_reach_the_weight_and_leave_the_base_untouched():
    from robotic_mpc_amd.simulator import SimulationManager

    base = config.base_params(terminal_cost={"weight": dict(LQR), "reference": dict(CONST)}, simulation_time=0.3, prediction_horizon=12,
                              solver_options=RTI)
    mgr = SimulationManager(base)
    mgr.grid_search({"terminal_cost.weight.r_weight": [0.5, 2.0], "terminal_cost.weight.q_weight": [1.0, 10.0], "prediction_horizon": [8, 12]})
    got = [(s["config"]["terminal_cost"]["weight"]["r_weight"], s["config"]["terminal_cost"]["weight"]["q_weight"],
            s["config"]["prediction_horizon"]) for s in mgr.simulations]
    assert got == [(r, q, N) for r in (0.5, 2.0) for q in (1.0, 10.0) for N in (8, 12)]
    assert base["terminal_cost"] == {"weight": LQR, "reference": CONST} and mgr.base_config["terminal_cost"] == {"weight": LQR, "reference": CONST}
    assert len({id(s["config"]["terminal_cost"]["weight"]) for s in mgr.simulations}) == 8
    resolved = [config.resolve_config(s["config"]) for s in mgr.simulations]
    assert len({packing.bucket_key(c, ragged=True) for c in resolved}) == 1
    b = [terminal.sample(c)["blocks"] for c in resolved]
    np.testing.assert_array_equal(b[0], b[1])                                 # the horizon does not enter the design
    assert np.abs(b[0] - b[2]).max() > 1.0 and np.abs(b[0] - b[4]).max() > 0.1


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_the_new_entry_is_declared_and_exported():
    from robotic_mpc_amd import build, engine

    build.build()
    lib = engine.load_library()
    text = open(os.path.join(ROOT, "include", "mpcbatch.h")).read()
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+mpcb_rollout_term\s*\(\s*mpcb_handle\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*const\s+mpcb_result\s*\*\s*\w+\s*,"
                     r"\s*const\s+double\s*\*\s*\w+\s*,\s*const\s+mpcb_plant_pert\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,"
                     r"\s*const\s+double\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)", body)
    assert hasattr(lib, "mpcb_rollout_term") and "mpcb_rollout_term" in engine._EXPORTS
    # header <-> ctypes: handle, step0, step1, out, yref_sched, pert, term_blocks, term_xref, stream
    dp = C.POINTER(C.c_double)
    assert lib.mpcb_rollout_term.argtypes == [C.c_void_p, C.c_int, C.c_int, C.POINTER(engine.MpcbResult), dp,
                                              C.POINTER(engine.MpcbPlantPert), dp, dp, C.c_void_p]
    for f in ("mpc_rollout_term.hip", "mpc_stream_rollout_term.hip"):
        assert f in build.SOURCES and os.path.exists(os.path.join(build.CSRC, f))
    doc = text[text.index("rollouts with the joint-wise terminal cost"):text.index("int mpcb_rollout_term")]
    for word in ("mpcb_step_term", "term_blocks == NULL", "MPCB_EINVAL", "MPCB_ESTATE", "term_xref"):
        assert word in doc
    assert "mpcb_rollout_term" in text[text.index("int mpcb_rollout_term"):text.index("int mpcb_queue_used")]
    # a null handle is refused before anything is read
    assert lib.mpcb_rollout_term(None, 0, 1, None, None, None, None, None, None) == -1
