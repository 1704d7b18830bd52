"""The controller-step API (mpcb_setup_controller / mpcb_step, BatchController) without a device: exports, struct layout,
and the configurations it refuses before it touches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from robotic_mpc_amd import build, engine

    build.build()
    return engine.load_library()


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpcbatch.h")).read(), flags=re.S)


def test_controller_symbols_are_declared_and_exported(lib):
    body = _header()
    for name in ("mpcb_setup_controller", "mpcb_step"):
        assert re.search(r"\bint\s+%s\s*\(" % name, body), name
        assert hasattr(lib, name), name


def test_step_io_struct_matches_header():
    from robotic_mpc_amd import engine

    m = re.search(r"typedef struct \{([^{}]*)\} mpcb_step_io;", _header())
    fields = re.findall(r"(const double|double|int)\s*\*\s*(\w+);", m.group(1))
    assert [n for _, n in fields] == [n for n, _ in engine.MpcbStepIO._fields_]
    assert [n for n, _, _ in engine.STEP_FIELDS] == [n for n, _ in engine.MpcbStepIO._fields_]
    for (ty, n), (_, cty) in zip(fields, engine.MpcbStepIO._fields_):
        assert cty == (C.POINTER(C.c_int) if ty == "int" else C.POINTER(C.c_double)), n
    assert C.sizeof(engine.MpcbStepIO) == 10 * 8


def test_batch_controller_is_exported():
    import robotic_mpc_amd
    from robotic_mpc_amd.controller import BatchController

    assert robotic_mpc_amd.BatchController is BatchController and "BatchController" in robotic_mpc_amd.__all__


@pytest.mark.skipif(__import__("conftest").has_gpu(), reason="checks the no-device behaviour")
def test_batch_controller_without_device_fails_loudly(lib):
    from robotic_mpc_amd import BatchController, base_params
    from robotic_mpc_amd.engine import EngineError

    with pytest.raises(EngineError):
        BatchController([base_params(prediction_horizon=20) for _ in range(3)])


@pytest.mark.parametrize("variant", ["horizons", "solver", "max_iter", "dt_steps", "fp32"])
def test_batch_controller_refuses_before_any_device_call(monkeypatch, variant):
    from robotic_mpc_amd import base_params, controller

    def no_device(*a, **k):
        raise AssertionError("the device was touched before the configurations were validated")
    monkeypatch.setattr(controller, "MpcBatchEngine", no_device)
    good = base_params(prediction_horizon=30)
    bad = {"horizons": base_params(prediction_horizon=31),
           "solver": base_params(prediction_horizon=30, solver_options={"nlp_solver_type": "SQP"}),
           "max_iter": base_params(prediction_horizon=30, solver_options={"nlp_solver_max_iter": 7}),
           "dt_steps": base_params(prediction_horizon=30, simulation_time=good["simulation_time"] * 2),
           "fp32": base_params(prediction_horizon=30, riccati_precision="fp32")}[variant]
    cfgs = [bad] if variant == "fp32" else [good, good, bad]
    with pytest.raises(ValueError):
        controller.BatchController(cfgs)
    with pytest.raises(ValueError):
        controller.BatchController([])


def test_controller_entry_points_reject_a_null_handle(lib):
    """mpcb_setup_controller and mpcb_step return MPCB_EINVAL for a NULL handle, without a device.  (The refusals of ragged
    horizons, fp32 Riccati and the wrong handle kind need a handle, i.e. a GPU: tests/test_gpu_controller.py
    test_call_order_refusals; BatchController's own refusals are test_batch_controller_refuses_before_any_device_call.)"""
    from robotic_mpc_amd import engine

    pb = engine.MpcbProblem(4, 20, 10, 1, 100, 50, 0, 0)
    assert lib.mpcb_setup_controller(None, C.byref(pb), None, None) == -1
    assert lib.mpcb_step(None, None, 0, None) == -1


def test_check_asm_holds_step_kernels_to_the_rollout_budgets():
    """scripts/check_asm.py applies its scratch budgets to the step module too: a step kernel is held to the budget of the
    rollout kernel of the same geometry, its passes to the budgets of the same passes."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("check_asm", os.path.join(ROOT, "scripts", "check_asm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    def fn(name, n):
        return "\n".join([name + ":"] + ["\tscratch_load_dword v1, off, s32"] * n + [".Lfunc_end0:"])
    for geom, budget in (("ILi8ELi1E", "18mpc_rollout_kernelILi8ELi1E"), ("ILi4ELi2E", "18mpc_rollout_kernelILi4ELi2E"),
                         ("ILi4ELi1E", "18mpc_rollout_kernelILi4ELi1E")):
        k = "_Z15mpc_step_kernel" + geom + "EvN4mpcb7ProblemE"
        limit = mod.BUDGET[budget]
        assert mod.scratch_ops(fn(k, limit)) == {}
        assert mod.scratch_ops(fn(k, limit + 1)) == {k: (limit + 1, limit)}
    hot = "_ZN4mpcb6EngineI7DevExecILi8ELi1EEE12fwd_residentILb0ELb0ELb0ELb0EEEdv"
    assert mod.scratch_ops(fn(hot, 94)) == {hot: (94, mod.MAX_SCRATCH_OPS)}
    assert "mpc_step.hip" in mod.STEP_SRC
