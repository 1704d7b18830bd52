"""The input-disturbance API of the controller step (mpcb_step_dist, BatchController.set_input_disturbance / input_disturbance /
step(dist=...)) without a device: the export, prototype and ctypes declaration, the NULL refusals, and everything BatchController
refuses before it touches a GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from robotic_mpc_amd import build, engine

    build.build()
    return engine.load_library()


def test_the_new_entry_is_declared_and_exported(lib):
    from robotic_mpc_amd import build, engine

    text = open(os.path.join(ROOT, "include", "mpcbatch.h")).read()
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+mpcb_step_dist\s*\(\s*mpcb_handle\s*\*\s*\w+\s*,\s*const\s+mpcb_step_io\s*\*\s*\w+\s*,\s*const\s+double\s*\*"
                     r"\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+int\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*int\s+\w+\s*,"
                     r"\s*void\s*\*\s*\w+\s*\)", body)
    assert re.search(r"#define\s+MPCB_VERSION\s+200\b", body)
    assert hasattr(lib, "mpcb_step_dist") and "mpcb_step_dist" in engine._EXPORTS
    # header <-> ctypes: handle, io, yref, ref_changed, warm, reset, dist, dist_changed, stream
    assert lib.mpcb_step_dist.argtypes == [C.c_void_p, C.POINTER(engine.MpcbStepIO), C.POINTER(C.c_double), C.c_int,
                                           C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double), C.c_int, C.c_void_p]
    for f in ("mpc_step_dist.hip", "mpc_stream_step_dist.hip"):
        assert f in build.SOURCES and os.path.exists(os.path.join(build.CSRC, f))
    # the model, the QP terms and what is not offered are documented in the header
    doc = text[text.index("input disturbance in the prediction model"):text.index("int mpcb_step_dist")]
    for word in ("Bd (u_k + d)", "b_k", "g_k", "H_k is unchanged", "dist_changed", "MPCB_WARM_SHIFT", "MPCB_EINVAL", "MPCB_ESTATE",
                 "mpcb_step_sens", "mpcb_step_sens_w", "mpcb_step_term", "not offered"):
        assert word in doc, word
    for name in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "mpcb_step_dist" in open(os.path.join(ROOT, name)).read(), name


def test_null_handles_are_refused(lib):
    d = (C.c_double * 6)()
    assert lib.mpcb_step_dist(None, None, None, 0, None, 0, d, 1, None) == -1
    assert lib.mpcb_step_dist(None, None, None, 0, None, 0, None, 0, None) == -1


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the device was touched ({name}) before the arguments were validated")


def _controller(B=3, N=20, solver="SQP_RTI"):
    """A BatchController as construction leaves it, with an engine that fails on any use."""
    from robotic_mpc_amd import base_params, config
    from robotic_mpc_amd.controller import BatchController

    ctl = object.__new__(BatchController)
    so = {"nlp_solver_type": solver}
    ctl.configs = [config.resolve_config(base_params(prediction_horizon=N, solver_options=so)) for _ in range(B)]
    ctl.horizons = np.array([N] * B, dtype=np.int64)
    ctl.batch, ctl.N = B, N
    ctl.engine, ctl.device = _NoDevice(), 0
    ctl._bufs, ctl._reset = None, True
    ctl._yref, ctl._ref_on, ctl._ref_changed, ctl._ref_stream, ctl._step_stream = None, False, False, None, None
    ctl._reset_mask, ctl._warm, ctl._sens = None, None, None
    return ctl


def test_valid_inputs_pass_validation_in_every_accepted_shape():
    ctl = _controller()
    for d in (np.linspace(-0.1, 0.1, 6), np.tile(np.linspace(-0.1, 0.1, 6), (3, 1))):
        out = ctl._check_disturbance(d)
        assert out.shape[1:] == (6,)
        np.testing.assert_array_equal(out[0], np.linspace(-0.1, 0.1, 6))
    assert ctl.input_disturbance() is None
    ctl.set_input_disturbance(None)                           # off while off: nothing to do, nothing touched
    assert ctl._dist_changed is False and ctl._dist_on is False


@pytest.mark.parametrize("d,msg", [
    (np.zeros(5), "shape"),
    (np.zeros((2, 6)), "shape"),
    (np.zeros((3, 6, 1)), "shape"),
    (np.zeros(6, dtype=np.float32), "float64"),
    ([0.0] * 6, "torch tensor, a numpy array or None"),
    (np.array([0.0, np.nan, 0, 0, 0, 0]), "non-finite"),
    (np.full((3, 6), np.inf), "non-finite"),
])
def test_invalid_disturbances_are_refused_before_the_device(d, msg):
    ctl = _controller()
    with pytest.raises(ValueError, match=msg):
        ctl.set_input_disturbance(d)
    with pytest.raises(ValueError, match=msg):
        ctl.step(np.zeros((3, 12)), dist=d)
    assert ctl._dist_on is False


def test_a_tensor_on_the_wrong_device_is_refused():
    import torch

    ctl = _controller()
    with pytest.raises(ValueError, match="must live on cuda:0"):
        ctl.set_input_disturbance(torch.zeros((3, 6), dtype=torch.float64))


def test_full_sqp_is_refused():
    ctl = _controller(solver="SQP")
    with pytest.raises(ValueError, match="SQP_RTI"):
        ctl.set_input_disturbance(np.zeros(6))
    with pytest.raises(ValueError, match="SQP_RTI"):
        ctl.step(np.zeros((3, 12)), dist=np.zeros(6))


def test_not_together_with_sensitivities_or_a_terminal_cost():
    ctl = _controller()
    for kw in (dict(sens=True), dict(sens_w=True)):
        with pytest.raises(ValueError, match="input disturbance"):
            ctl.step(np.zeros((3, 12)), dist=np.zeros(6), **kw)
    ctl._dist_on = True                                       # one in force from an earlier call
    for kw in (dict(sens=True), dict(sens_w=True)):
        with pytest.raises(ValueError, match="input disturbance"):
            ctl.step(np.zeros((3, 12)), **kw)
    with pytest.raises(ValueError, match="input disturbance"):
        ctl.set_terminal_cost(np.array([[4.0, 0.5, 1.0]] * 6), np.zeros(12))
    ctl._dist_on = False
    ctl._term_on = True                                       # a terminal cost in force
    with pytest.raises(ValueError, match="terminal cost"):
        ctl.set_input_disturbance(np.zeros(6))
    with pytest.raises(ValueError, match="terminal cost"):
        ctl.step(np.zeros((3, 12)), dist=np.zeros(6))
