"""The controller step on either kernel family (mpcb_setup_controller_on / mpcb_controller_engine_for, BatchController(engine=))
without a device: exports, the engine choice of MPCB_ENGINE_AUTO, the configurations each engine takes or refuses before it touches
a GPU, and the scratch budget of the throughput engine's step kernel."""
import ctypes as C
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from robotic_mpc_amd import build, engine

    build.build()
    return engine.load_library()


def _header():
    return open(os.path.join(ROOT, "include", "mpcbatch.h")).read()


def _define(name):
    m = re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, _header())
    assert m, name
    return int(m.group(1))


def test_entry_points_are_declared_and_exported(lib):
    body = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("mpcb_setup_controller_on", "mpcb_controller_engine_for"):
        assert re.search(r"\bint\s+%s\s*\(" % name, body), name
        assert hasattr(lib, name), name


def test_engine_values_match_the_header():
    from robotic_mpc_amd import engine

    assert engine.CONTROLLER_ENGINES == {"auto": _define("MPCB_ENGINE_AUTO"), "latency": _define("MPCB_ENGINE_LATENCY"),
                                         "stream": _define("MPCB_ENGINE_STREAM")}
    assert engine.CONTROLLER_ENGINES == {"auto": -1, "latency": 0, "stream": 1}


def _pb(batch, N=100, Nsim=600, solver=1):
    from robotic_mpc_amd import engine

    return engine.MpcbProblem(batch, N, Nsim, solver, 100, 50, 0, 0)


def test_auto_choice(lib, monkeypatch):
    monkeypatch.delenv("MPCB_ENGINE", raising=False)
    t = _define("MPCB_STREAM_MIN_BATCH_STEP")
    f = lib.mpcb_controller_engine_for
    # ragged: the throughput engine whatever the size
    for b in (1, 7, t - 1, t):
        assert f(C.byref(_pb(b)), 1) == 1, b
    # uniform SQP_RTI: crossover at MPCB_STREAM_MIN_BATCH_STEP
    assert f(C.byref(_pb(1)), 0) == 0
    assert f(C.byref(_pb(t - 1)), 0) == 0
    assert f(C.byref(_pb(t)), 0) == 1
    assert f(C.byref(_pb(2 * t)), 0) == 1
    # uniform full SQP: the latency engine at every size (include/mpcbatch.h: it never crossed over)
    for b in (1, t, 4096, 65536):
        assert f(C.byref(_pb(b, solver=0)), 0) == 0, b
    # a controller has no run length: Nsim does not matter
    for b in (t - 1, t):
        assert len({f(C.byref(_pb(b, Nsim=s)), 0) for s in (1, 10, 300, 100000)}) == 1, b
    # the environment overrides a uniform choice; a ragged batch stays on the only engine that runs it
    monkeypatch.setenv("MPCB_ENGINE", "latency")
    assert f(C.byref(_pb(t)), 0) == 0 and f(C.byref(_pb(t)), 1) == 1
    monkeypatch.setenv("MPCB_ENGINE", "stream")
    assert f(C.byref(_pb(1)), 0) == 1
    assert f(None, 0) == -1


def test_python_helper_agrees(lib, monkeypatch):
    from robotic_mpc_amd import engine

    monkeypatch.delenv("MPCB_ENGINE", raising=False)
    t = _define("MPCB_STREAM_MIN_BATCH_STEP")
    assert engine.controller_engine_for(t - 1, 100, lib=lib) == 0
    assert engine.controller_engine_for(t, 100, lib=lib) == 1
    assert engine.controller_engine_for(3, 100, ragged=True, lib=lib) == 1


def _grid(solver="SQP_RTI", **kw):
    from robotic_mpc_amd import base_params

    return [base_params(prediction_horizon=N, solver_options={"nlp_solver_type": solver}, **kw) for N in (10, 20, 35)]


@pytest.fixture
def no_device(monkeypatch):
    """BatchController with the device monkeypatched away: what reaches MpcBatchEngine is recorded, nothing runs."""
    from robotic_mpc_amd import controller

    calls = []

    class Fake:
        device = 0

        def __init__(self, device):
            calls.append(("create", device))

        def setup_controller(self, cfgs, chain, engine="latency"):
            calls.append(("setup", engine, [c["N"] for c in cfgs]))
    monkeypatch.setattr(controller, "MpcBatchEngine", Fake)
    return calls


@pytest.mark.parametrize("eng", ["stream", "auto"])
def test_ragged_rti_grid_is_accepted(no_device, eng):
    from robotic_mpc_amd import controller

    ctl = controller.BatchController(_grid(), engine=eng)
    assert list(ctl.horizons) == [10, 20, 35] and ctl.N == 35 and ctl.batch == 3
    assert no_device[-1] == ("setup", eng, [10, 20, 35])


def test_default_engine_is_latency(no_device):
    from robotic_mpc_amd import base_params, controller

    ctl = controller.BatchController([base_params(prediction_horizon=30)] * 2)
    assert no_device[-1] == ("setup", "latency", [30, 30]) and ctl.N == 30 and list(ctl.horizons) == [30, 30]


@pytest.mark.parametrize("case", ["ragged_latency", "ragged_sqp_stream", "ragged_sqp_auto", "fp32_latency", "fp32_stream",
                                  "fp32_auto", "unknown_engine", "mixed_solver_stream"])
def test_refused_before_any_device_call(no_device, case):
    from robotic_mpc_amd import base_params, controller

    cfgs, eng = {
        "ragged_latency": (_grid(), "latency"),
        "ragged_sqp_stream": (_grid("SQP"), "stream"),
        "ragged_sqp_auto": (_grid("SQP"), "auto"),
        "fp32_latency": ([base_params(prediction_horizon=30, riccati_precision="fp32")], "latency"),
        "fp32_stream": ([base_params(prediction_horizon=30, riccati_precision="fp32")], "stream"),
        "fp32_auto": ([base_params(prediction_horizon=30, riccati_precision="fp32")], "auto"),
        "unknown_engine": ([base_params(prediction_horizon=30)], "throughput"),
        "mixed_solver_stream": ([base_params(prediction_horizon=30),
                                 base_params(prediction_horizon=30, solver_options={"nlp_solver_type": "SQP"})], "stream"),
    }[case]
    with pytest.raises(ValueError):
        controller.BatchController(cfgs, engine=eng)
    assert no_device == []


def test_null_handle(lib):
    from robotic_mpc_amd import engine

    pb = _pb(4, 20, 10)
    for e in (-1, 0, 1):
        assert lib.mpcb_setup_controller_on(None, C.byref(pb), None, None, e) == -1


def _check_asm():
    spec = importlib.util.spec_from_file_location("check_asm", os.path.join(ROOT, "scripts", "check_asm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_check_asm_holds_the_stream_step_kernel_to_the_stream_budget():
    """scripts/check_asm.py scans mpc_stream_step.hip: its kernel is held to mpc_stream_kernel<double>'s budget, its passes to
    the throughput engine's hot-pass limit."""
    mod = _check_asm()

    def fn(name, n):
        return "\n".join([name + ":"] + ["\tscratch_load_dword v1, off, s32"] * n + [".Lfunc_end0:"])
    k = "_Z22mpc_stream_step_kernelN4mpcb7ProblemEPKNS_5RobotEPKNS_10InstParamsEPdmNS_6StepIOEi"
    limit = mod.BUDGET["17mpc_stream_kernelId"]
    assert mod.scratch_ops(fn(k, limit)) == {}
    assert mod.scratch_ops(fn(k, limit + 1)) == {k: (limit + 1, limit)}
    hot = "_ZN4mpcb2se9fact_passIdLb0EEEvv"
    assert mod.scratch_ops(fn(hot, mod.MAX_SCRATCH_OPS + 1)) == {hot: (mod.MAX_SCRATCH_OPS + 1, mod.MAX_SCRATCH_OPS)}
    assert any(os.path.basename(s) == "mpc_stream_step.hip" for s in mod.SOURCES)
    for s in mod.SOURCES:
        assert os.path.exists(s), s


def test_stream_step_module_is_built():
    from robotic_mpc_amd import build

    assert "mpc_stream_step.hip" in build.SOURCES
