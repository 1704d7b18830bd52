"""The sensitivity API of the controller step (mpcb_step_sens, BatchController.step(sens=True), robotic_mpc_amd.autograd) without a
device: the export and declaration, the NULL-handle refusal, what BatchController refuses before it touches a GPU, and
differentiable_step on a stub controller of CPU tensors that implements a known affine map."""
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


def test_step_sens_is_declared_and_exported(lib):
    from robotic_mpc_amd import engine

    text = open(os.path.join(ROOT, "include", "mpcbatch.h")).read()
    body = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"typedef\s+struct\s*\{\s*double\s*\*\s*du0_dx\s*;\s*double\s*\*\s*du0_dyref\s*;\s*int\s*\*\s*valid\s*;\s*\}\s*"
                     r"mpcb_step_sens_out\s*;", body)
    assert re.search(r"\bint\s+mpcb_step_sens\s*\(\s*mpcb_handle\s*\*\s*\w+\s*,\s*const\s+mpcb_step_io\s*\*\s*\w+\s*,\s*const\s+double\s*\*"
                     r"\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+int\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+mpcb_step_sens_out\s*\*\s*\w+\s*,"
                     r"\s*void\s*\*\s*\w+\s*\)", body)
    assert hasattr(lib, "mpcb_step_sens") and "mpcb_step_sens" in engine._EXPORTS
    assert [f[0] for f in engine.MpcbStepSensOut._fields_] == ["du0_dx", "du0_dyref", "valid"]
    assert C.sizeof(engine.MpcbStepSensOut) == 3 * C.sizeof(C.c_void_p)
    # header <-> ctypes: handle, io, yref, ref_changed, warm, reset, sens, stream
    assert lib.mpcb_step_sens.argtypes == [C.c_void_p, C.POINTER(engine.MpcbStepIO), C.POINTER(C.c_double), C.c_int,
                                           C.POINTER(C.c_int), C.c_int, C.POINTER(engine.MpcbStepSensOut), C.c_void_p]


def test_step_sens_rejects_a_null_handle(lib):
    from robotic_mpc_amd import engine

    so = engine.MpcbStepSensOut()
    assert lib.mpcb_step_sens(None, None, None, 0, None, 0, None, None) == -1
    assert lib.mpcb_step_sens(None, None, None, 0, None, 0, C.byref(so), None) == -1


class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the device was touched ({name}) before the arguments were validated")


def _controller(B=3, N=20, solver="SQP"):
    """A BatchController as construction leaves it, with an engine that fails on any use."""
    from robotic_mpc_amd import base_params, config
    from robotic_mpc_amd.controller import BatchController

    ctl = object.__new__(BatchController)
    ctl.configs = [config.resolve_config(base_params(prediction_horizon=N, solver_options={"nlp_solver_type": solver})) for _ in range(B)]
    ctl.horizons = np.array([N] * B, dtype=np.int64)
    ctl.batch, ctl.N = B, N
    ctl.engine, ctl.device = _NoDevice(), 0
    ctl._bufs, ctl._reset = None, True
    ctl._yref, ctl._ref_on, ctl._ref_changed, ctl._ref_stream, ctl._step_stream = None, False, False, None, None
    ctl._reset_mask, ctl._warm, ctl._sens = None, None, None
    return ctl


def test_sens_on_a_full_sqp_batch_is_refused_before_any_device_call():
    pytest.importorskip("torch")
    ctl = _controller(solver="SQP")
    with pytest.raises(ValueError, match="SQP_RTI"):
        ctl.step(np.zeros((3, 12)), sens=True)
    assert ctl._sens is None and ctl._bufs is None and ctl._reset


@pytest.mark.parametrize("bad", ["xhat_shape", "xhat_dtype", "yref_shape", "shift_dtype"])
def test_bad_arguments_with_sens_are_refused_before_any_device_call(bad):
    pytest.importorskip("torch")
    ctl = _controller(solver="SQP_RTI")
    kw = dict(xhat=np.zeros((3, 12)))
    kw.update({"xhat_shape": dict(xhat=np.zeros((2, 12))), "xhat_dtype": dict(xhat=np.zeros((3, 12), np.float32)),
               "yref_shape": dict(yref=np.zeros((3, 19, 5))), "shift_dtype": dict(shift=np.zeros(3))}[bad])
    with pytest.raises(ValueError):
        ctl.step(kw.pop("xhat"), sens=True, **kw)
    assert ctl._sens is None and ctl._bufs is None


class _Stub:
    """u0 = c + Jx xhat + sum_k Jy[k]' yref_k on CPU tensors, with the outputs of BatchController.step(sens=True); the simulations
    of `invalid` report no sensitivities (NaN, sens_valid 0) as the device does."""

    def __init__(self, torch, B=3, N=4, invalid=()):
        g = torch.Generator().manual_seed(11)
        self.Jx = torch.randn(B, 6, 12, generator=g, dtype=torch.float64)
        self.Jy = torch.randn(B, N, 5, 6, generator=g, dtype=torch.float64)
        self.c = torch.randn(B, 6, generator=g, dtype=torch.float64)
        self.invalid, self.calls, self.torch = list(invalid), [], torch

    def step(self, xhat, predict=False, yref=None, shift=False, sens=False):
        torch = self.torch
        assert sens and not xhat.requires_grad and (yref is None or not yref.requires_grad)
        self.calls.append(dict(predict=predict, shift=shift))
        u0 = self.c + torch.einsum("bux,bx->bu", self.Jx, xhat)
        if yref is not None:
            u0 = u0 + torch.einsum("bkcu,bkc->bu", self.Jy, yref)
        jx, jy, ok = self.Jx.clone(), self.Jy.clone(), torch.ones(xhat.shape[0], dtype=torch.int32)
        for i in self.invalid:
            jx[i], jy[i], ok[i] = float("nan"), float("nan"), 0
        return dict(u0=u0, du0_dx=jx, du0_dyref=jy, sens_valid=ok)


def test_gradcheck_of_differentiable_step_on_an_affine_stub():
    torch = pytest.importorskip("torch")
    from robotic_mpc_amd.autograd import differentiable_step

    stub = _Stub(torch)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 12, generator=g, dtype=torch.float64, requires_grad=True)
    y = torch.randn(3, 4, 5, generator=g, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda a, b: differentiable_step(stub, a, b), (x, y), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda a: differentiable_step(stub, a), (x,), eps=1e-6, atol=1e-7)
    # the gradient of u0.sum() is the column sums of the Jacobians; step's keyword arguments are passed on
    u0 = differentiable_step(stub, x, y, shift=True, predict=True)
    assert stub.calls[-1] == dict(predict=True, shift=True)
    gx, gy = torch.autograd.grad(u0.sum(), (x, y))
    torch.testing.assert_close(gx, stub.Jx.sum(1), rtol=0, atol=1e-13)
    torch.testing.assert_close(gy, stub.Jy.sum(3), rtol=0, atol=1e-13)
    # only x requires a gradient: none is formed for the reference
    u0 = differentiable_step(stub, x, y.detach())
    (gx2,) = torch.autograd.grad(u0.sum(), (x,))
    torch.testing.assert_close(gx2, gx, rtol=0, atol=0)


def test_both_invalid_modes():
    torch = pytest.importorskip("torch")
    from robotic_mpc_amd.autograd import differentiable_step

    stub = _Stub(torch, invalid=[1])
    x = torch.zeros(3, 12, dtype=torch.float64, requires_grad=True)
    y = torch.zeros(3, 4, 5, dtype=torch.float64, requires_grad=True)
    gx, gy = torch.autograd.grad(differentiable_step(stub, x, y, invalid="nan").sum(), (x, y))
    assert torch.isnan(gx[1]).all() and torch.isnan(gy[1]).all()
    assert torch.isfinite(gx[[0, 2]]).all() and torch.isfinite(gy[[0, 2]]).all()
    gx, gy = torch.autograd.grad(differentiable_step(stub, x, y, invalid="zero").sum(), (x, y))
    assert (gx[1] == 0).all() and (gy[1] == 0).all()
    torch.testing.assert_close(gx[[0, 2]], stub.Jx.sum(1)[[0, 2]], rtol=0, atol=1e-13)
    torch.testing.assert_close(gy[[0, 2]], stub.Jy.sum(3)[[0, 2]], rtol=0, atol=1e-13)
    with pytest.raises(ValueError):
        differentiable_step(stub, x, y, invalid="skip")
    with pytest.raises(ValueError):
        differentiable_step(stub, x, y, sens=True)
