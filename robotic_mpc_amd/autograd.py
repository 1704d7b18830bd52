"""The controller step as a differentiable torch function.

``differentiable_step(ctl, xhat, yref)`` runs ``ctl.step(xhat, yref=yref, sens=True)`` and returns ``u0`` with a backward pass
built from the step's own sensitivities: ``du0_dx`` = d u0 / d xhat and ``du0_dyref[:, k]`` = (d u0 / d yref_k)'.  They are the
exact Jacobians of the step's QP with its linearisation point held fixed -- the derivative of one real-time iteration, not of a
converged solve -- and exist where the bound-inactive fast path solved the QP (``sens_valid``).  Elsewhere the controller
returns NaN: ``invalid="nan"`` lets it reach the gradients, ``invalid="zero"`` gives those simulations a zero gradient.

Cotangents flow to ``xhat`` and ``yref`` only (not through ``x_pred`` / ``u_pred``, not through active bounds).  The function
touches the controller through ``step`` alone, so anything with that method -- a stub on CPU tensors -- can drive it.
"""
from __future__ import annotations


def differentiable_step(ctl, xhat, yref=None, invalid: str = "nan", **step_kw):
    """``u0`` [B, 6] of ``ctl.step(xhat, yref=yref, sens=True, **step_kw)``, differentiable with respect to ``xhat`` [B, 12] and
    ``yref`` [B, N, 5] (a clone: the controller's buffers are overwritten by its next step)."""
    import torch

    if invalid not in ("nan", "zero"):
        raise ValueError(f"invalid must be 'nan' or 'zero', got {invalid!r}")
    if "sens" in step_kw:
        raise ValueError("differentiable_step asks for the sensitivities itself: do not pass sens")
    if yref is not None and (yref.dim() != 3 or yref.shape[-1] != 5):
        raise ValueError(f"a differentiable reference has shape [B, N, 5], got {tuple(yref.shape)}")

    class _Step(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, y):
            out = ctl.step(x.detach(), yref=None if y is None else y.detach(), sens=True, **step_kw)
            jx, jy, ok = out["du0_dx"].clone(), out["du0_dyref"].clone(), out["sens_valid"] != 0
            if invalid == "zero":
                jx = torch.where(ok[:, None, None], jx, torch.zeros_like(jx))
                jy = torch.where(ok[:, None, None, None], jy, torch.zeros_like(jy))
            ctx.save_for_backward(jx, jy)
            ctx.has_y = y is not None
            return out["u0"].clone()

        @staticmethod
        def backward(ctx, g):
            jx, jy = ctx.saved_tensors
            gx = torch.einsum("bu,bux->bx", g, jx) if ctx.needs_input_grad[0] else None
            gy = torch.einsum("bu,bkcu->bkc", g, jy) if ctx.has_y and ctx.needs_input_grad[1] else None
            return gx, gy

    return _Step.apply(xhat, yref)
