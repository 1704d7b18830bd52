"""The task-reference API of the controller step (mpcb_step_ref, BatchController.set_reference / step(yref=...)) without a device:
the export and declaration, the NULL-handle refusal, and the references BatchController refuses before it touches a GPU."""
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


def test_step_ref_is_declared_and_exported(lib):
    from robotic_mpc_amd import engine

    body = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mpcbatch.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mpcb_step_ref\s*\(\s*mpcb_handle\s*\*\s*\w+\s*,\s*const\s+mpcb_step_io\s*\*\s*\w+\s*,\s*const\s+double\s*\*"
                     r"\s*\w+\s*,\s*int\s+\w+\s*,\s*int\s+\w+\s*,\s*void\s*\*\s*\w+\s*\)", body)
    assert re.search(r"#define\s+MPCB_NREF\s+5\b", body)
    assert hasattr(lib, "mpcb_step_ref") and "mpcb_step_ref" in engine._EXPORTS


def test_step_ref_rejects_a_null_handle(lib):
    y = (C.c_double * 5)()
    assert lib.mpcb_step_ref(None, None, None, 0, 0, None) == -1
    assert lib.mpcb_step_ref(None, None, y, 1, 1, None) == -1


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the device was touched ({name}) before the reference was validated")


def _controller(horizons=(20, 20, 20)):
    """A BatchController as construction leaves it, with an engine that fails on any use."""
    from robotic_mpc_amd import base_params, config
    from robotic_mpc_amd.controller import BatchController

    ctl = object.__new__(BatchController)
    ctl.configs = [config.resolve_config(base_params(prediction_horizon=n)) for n in horizons]
    ctl.horizons = np.array(horizons, dtype=np.int64)
    ctl.batch, ctl.N = len(horizons), int(max(horizons))
    ctl.engine, ctl.device = _NoDevice(), 0
    ctl._bufs, ctl._reset = None, True
    ctl._yref, ctl._ref_on, ctl._ref_changed, ctl._ref_stream, ctl._step_stream = None, False, False, None, None
    return ctl


@pytest.mark.parametrize("bad", ["shape", "shape2", "dtype", "list", "nan_active", "inf_2d", "cpu_tensor", "tensor_dtype"])
def test_bad_references_are_refused_before_any_device_call(bad):
    torch = pytest.importorskip("torch")
    ctl = _controller()
    good = np.tile([0.0, 1.0, 0.0, 0.35, 0.04], (3, 20, 1))
    y = {"shape": good[:, :19], "shape2": good[:2], "dtype": good.astype(np.float32), "list": good.tolist(),
         "nan_active": np.where(np.arange(20)[None, :, None] == 7, np.nan, good),
         "inf_2d": np.array([[0.0, 1.0, 0.0, np.inf, 0.0]] * 3),
         "cpu_tensor": torch.from_numpy(good), "tensor_dtype": torch.from_numpy(good.astype(np.float32))}[bad]
    with pytest.raises(ValueError):
        ctl.set_reference(y)
    with pytest.raises(ValueError):
        ctl.step(np.zeros((3, 12)), yref=y)
    assert not ctl._ref_on and not ctl._ref_changed


def test_rows_past_a_ragged_horizon_are_not_checked():
    ctl = _controller(horizons=(5, 20, 12))
    y = np.tile([0.0, 1.0, 0.0, 0.35, 0.04], (3, 20, 1))
    y[0, 5:] = np.nan
    y[2, 12:] = np.inf
    assert ctl._check_reference(y).shape == (3, 20, 5)
    assert ctl._check_reference(y[:, 0]).shape == (3, 1, 5)
    y[2, 11, 4] = np.nan
    with pytest.raises(ValueError):
        ctl._check_reference(y)


def test_reverting_to_the_packed_reference_is_host_state_only():
    ctl = _controller()
    ctl.set_reference(None)                # nothing in force: nothing changes
    assert not ctl._ref_on and not ctl._ref_changed
    ctl._ref_on = True
    ctl.set_reference(None)
    assert not ctl._ref_on and ctl._ref_changed
