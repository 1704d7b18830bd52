"""The run-time weights and weight-sensitivity API of the controller step (mpcb_set_weights, mpcb_step_sens_w,
BatchController.set_weights / weights / step(sens_w=True), differentiable_step(weights=...)) without a device: the exports and
declarations, the NULL refusals, what BatchController refuses before it touches a GPU, and differentiable_step on a stub controller
of CPU tensors whose u0 is a known smooth function of the weights."""
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


def test_the_new_entries_are_declared_and_exported(lib):
    from robotic_mpc_amd import engine

    text = open(os.path.join(ROOT, "include", "mpcbatch.h")).read()
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+MPCB_NWEIGHT\s+7\b", body)
    assert re.search(r"\bint\s+mpcb_set_weights\s*\(\s*mpcb_handle\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)", body)
    assert re.search(r"\bint\s+mpcb_step_sens_w\s*\(\s*mpcb_handle\s*\*\s*\w+\s*,\s*const\s+mpcb_step_io\s*\*\s*\w+\s*,\s*const\s+double\s*\*"
                     r"\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+int\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+mpcb_step_sens_out\s*\*\s*\w+\s*,"
                     r"\s*double\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*\)", body)
    for name in ("mpcb_set_weights", "mpcb_step_sens_w"):
        assert hasattr(lib, name) and name in engine._EXPORTS
    assert lib.mpcb_set_weights.argtypes == [C.c_void_p, C.POINTER(C.c_double), C.c_void_p]
    # header <-> ctypes: handle, io, yref, ref_changed, warm, reset, sens, du0_dw, stream
    assert lib.mpcb_step_sens_w.argtypes == [C.c_void_p, C.POINTER(engine.MpcbStepIO), C.POINTER(C.c_double), C.c_int,
                                             C.POINTER(C.c_int), C.c_int, C.POINTER(engine.MpcbStepSensOut), C.POINTER(C.c_double),
                                             C.c_void_p]
    from robotic_mpc_amd import controller

    assert controller.NWEIGHT == 7


def test_null_handles_are_refused(lib):
    from robotic_mpc_amd import engine

    w = (C.c_double * 7)()
    assert lib.mpcb_set_weights(None, w, None) == -1
    so = engine.MpcbStepSensOut()
    assert lib.mpcb_step_sens_w(None, None, None, 0, None, 0, C.byref(so), w, None) == -1


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the device was touched ({name}) before the arguments were validated")


def _controller(B=3, N=20, solver="SQP_RTI", lm=0.0):
    """A BatchController as construction leaves it, with an engine that fails on any use."""
    from robotic_mpc_amd import base_params, config
    from robotic_mpc_amd.controller import BatchController

    ctl = object.__new__(BatchController)
    so = {"nlp_solver_type": solver, "levenberg_marquardt": lm}
    ctl.configs = [config.resolve_config(base_params(prediction_horizon=N, solver_options=so, w_u=0.01 * (i + 1))) for i in range(B)]
    ctl.horizons = np.array([N] * B, dtype=np.int64)
    ctl.batch, ctl.N = B, N
    ctl.engine, ctl.device = _NoDevice(), 0
    ctl._bufs, ctl._reset = None, True
    ctl._yref, ctl._ref_on, ctl._ref_changed, ctl._ref_stream, ctl._step_stream = None, False, False, None, None
    ctl._reset_mask, ctl._warm, ctl._sens = None, None, None
    return ctl


def test_packed_weights_are_the_configurations():
    ctl = _controller()
    w = ctl.packed_weights()
    assert w.shape == (3, 7) and w.dtype == np.float64
    np.testing.assert_array_equal(w[:, 0], [0.01, 0.02, 0.03])
    np.testing.assert_array_equal(w[:, 1], [c["w_qddot"] for c in ctl.configs])
    np.testing.assert_array_equal(w[:, 2:], np.stack([c["w_task"] for c in ctl.configs]))
    w[:] = 0.0
    assert ctl.packed_weights()[0, 0] == 0.01                       # a new array per call


GOOD = np.array([0.01, 0.02, 50.0, 40.0, 0.0, 20.0, 10.0])


@pytest.mark.parametrize("bad,match", [
    (lambda: np.tile(GOOD, (2, 1)), r"shape \(3, 7\) or \(7,\)"),
    (lambda: np.tile(GOOD[:6], (3, 1)), r"shape \(3, 7\) or \(7,\)"),
    (lambda: np.tile(GOOD, (3, 1)).astype(np.float32), "float64"),
    (lambda: np.where(np.arange(7) == 3, np.nan, np.tile(GOOD, (3, 1))), "non-finite"),
    (lambda: np.where(np.arange(7) == 5, np.inf, GOOD), "non-finite"),
    (lambda: np.where(np.arange(7) == 4, -1e-9, np.tile(GOOD, (3, 1))), ">= 0"),
    (lambda: np.where(np.arange(7) < 2, 0.0, GOOD), "levenberg_marquardt must be > 0"),
    (lambda: [0.01] * 7, "torch tensor, a numpy array or None"),
], ids=["batch", "columns", "dtype", "nan", "inf", "negative", "singular", "type"])
def test_set_weights_validates_before_the_device_is_touched(bad, match):
    pytest.importorskip("torch")
    ctl = _controller()
    with pytest.raises(ValueError, match=match):
        ctl.set_weights(bad())
    assert ctl._weights is None and ctl._weights_stream is None


def test_zero_input_weights_are_legal_with_a_levenberg_marquardt_term():
    pytest.importorskip("torch")
    ctl = _controller(lm=1e-4)
    w = ctl._check_weights(np.where(np.arange(7) < 2, 0.0, GOOD))
    assert w.shape == (1, 7)
    assert ctl._check_weights(np.tile(GOOD, (3, 1))).shape == (3, 7)


def test_a_tensor_on_another_device_is_refused():
    torch = pytest.importorskip("torch")
    ctl = _controller()
    with pytest.raises(ValueError, match="cuda:0"):
        ctl.set_weights(torch.zeros(3, 7, dtype=torch.float64))


def test_sens_w_on_a_full_sqp_batch_is_refused_before_any_device_call():
    pytest.importorskip("torch")
    ctl = _controller(solver="SQP")
    with pytest.raises(ValueError, match="SQP_RTI"):
        ctl.step(np.zeros((3, 12)), sens_w=True)
    assert ctl._sens is None and ctl._sensw is None and ctl._bufs is None and ctl._reset


class _Stub:
    """u0 = c + Jx xhat + tanh(w) Jw on CPU tensors: smooth in the weights, with du0_dw[b, p, u] = (1 - tanh(w_bp)^2) Jw[b, p, u];
    the outputs of BatchController.step(sens_w=True).  Records every call."""

    def __init__(self, torch, B=3, N=4, invalid=()):
        g = torch.Generator().manual_seed(13)
        self.Jx = torch.randn(B, 6, 12, generator=g, dtype=torch.float64)
        self.Jy = torch.randn(B, N, 5, 6, generator=g, dtype=torch.float64)
        self.Jw = torch.randn(B, 7, 6, generator=g, dtype=torch.float64)
        self.c = torch.randn(B, 6, generator=g, dtype=torch.float64)
        self.w = torch.zeros(B, 7, dtype=torch.float64)
        self.invalid, self.calls, self.torch = list(invalid), [], torch

    def set_weights(self, w):
        assert not w.requires_grad
        self.calls.append(("set_weights",))
        self.w = w.clone()

    def step(self, xhat, predict=False, yref=None, shift=False, sens=False, sens_w=False):
        torch = self.torch
        assert (sens or sens_w) and not xhat.requires_grad
        self.calls.append(("step", dict(predict=predict, shift=shift, sens=sens, sens_w=sens_w)))
        u0 = self.c + torch.einsum("bux,bx->bu", self.Jx, xhat) + torch.einsum("bp,bpu->bu", torch.tanh(self.w), self.Jw)
        if yref is not None:
            u0 = u0 + torch.einsum("bkcu,bkc->bu", self.Jy, yref)
        jx, jy, ok = self.Jx.clone(), self.Jy.clone(), torch.ones(xhat.shape[0], dtype=torch.int32)
        jw = (1.0 - torch.tanh(self.w) ** 2)[:, :, None] * self.Jw
        for i in self.invalid:
            jx[i], jy[i], jw[i], ok[i] = float("nan"), float("nan"), float("nan"), 0
        out = dict(u0=u0, du0_dx=jx, du0_dyref=jy, sens_valid=ok)
        if sens_w:
            out["du0_dw"] = jw
        return out


def test_gradcheck_of_differentiable_step_with_weights():
    torch = pytest.importorskip("torch")
    from robotic_mpc_amd.autograd import differentiable_step

    stub = _Stub(torch)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(3, 12, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.randn(3, 4, 5, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.rand(3, 7, generator=g, dtype=torch.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b, c: differentiable_step(stub, a, b, c), (x, y, w), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda a, c: differentiable_step(stub, a, weights=c), (x, w), eps=1e-6, atol=1e-7)
    stub.calls.clear()
    u0 = differentiable_step(stub, x, y, w, shift=True)
    assert stub.calls == [("set_weights",), ("step", dict(predict=False, shift=True, sens=False, sens_w=True))]
    (gw,) = torch.autograd.grad(u0.sum(), (w,))
    torch.testing.assert_close(gw, ((1.0 - torch.tanh(w) ** 2)[:, :, None] * stub.Jw).sum(2).detach(), rtol=0, atol=1e-13)


def test_without_weights_the_controller_is_touched_through_step_alone():
    torch = pytest.importorskip("torch")
    from robotic_mpc_amd.autograd import differentiable_step

    stub = _Stub(torch)
    x = torch.zeros(3, 12, dtype=torch.float64, requires_grad=True)
    differentiable_step(stub, x).sum().backward()
    assert stub.calls == [("step", dict(predict=False, shift=False, sens=True, sens_w=False))]


def test_invalid_modes_and_refusals_with_weights():
    torch = pytest.importorskip("torch")
    from robotic_mpc_amd.autograd import differentiable_step

    stub = _Stub(torch, invalid=[1])
    x = torch.zeros(3, 12, dtype=torch.float64)
    w = torch.full((3, 7), 0.3, dtype=torch.float64, requires_grad=True)
    (gw,) = torch.autograd.grad(differentiable_step(stub, x, weights=w, invalid="nan").sum(), (w,))
    assert torch.isnan(gw[1]).all() and torch.isfinite(gw[[0, 2]]).all()
    (gw,) = torch.autograd.grad(differentiable_step(stub, x, weights=w, invalid="zero").sum(), (w,))
    assert (gw[1] == 0).all() and (gw[[0, 2]] != 0).all()
    with pytest.raises(ValueError, match=r"\[B, 7\]"):
        differentiable_step(stub, x, weights=torch.zeros(7, dtype=torch.float64))
    with pytest.raises(ValueError):
        differentiable_step(stub, x, weights=w, sens_w=True)
