"""The controller step as a differentiable torch function.

``differentiable_step(ctl, xhat, yref)`` runs ``ctl.step(xhat, yref=yref, sens=True)`` and returns ``u0`` with a backward pass
built from the step's own sensitivities: ``du0_dx`` = d u0 / d xhat and ``du0_dyref[:, k]`` = (d u0 / d yref_k)'.  They are the
exact Jacobians of the step's QP with its linearisation point held fixed -- the derivative of one real-time iteration, not of a
converged solve -- and exist where the bound-inactive fast path solved the QP (``sens_valid``).  Elsewhere the controller
returns NaN: ``invalid="nan"`` lets it reach the gradients, ``invalid="zero"`` gives those simulations a zero gradient.

Cotangents flow to ``xhat`` and ``yref`` only (not through ``x_pred`` / ``u_pred``, not through active bounds).  The function
touches the controller through ``step`` alone, so anything with that method -- a stub on CPU tensors -- can drive it.

``differentiable_step(ctl, xhat, yref, weights=w)`` also sets the cost weights ``w`` [B, 7] (``ctl.set_weights``) before the step,
asks it for ``du0_dw`` (``sens_w=True``) and lets cotangents flow to ``w``: gradient tuning of the weights of a batch of
controllers.  The same caveat holds: ``du0_dw`` is the derivative of one real-time iteration with its linearisation point fixed;
over several closed-loop steps the dependence of the carried iterate on the weights of earlier steps is not included.
"""
from __future__ import annotations


def differentiable_step(ctl, xhat, yref=None, weights=None, invalid: str = "nan", **step_kw):
    """``u0`` [B, 6] of ``ctl.step(xhat, yref=yref, sens=True, **step_kw)``, differentiable with respect to ``xhat`` [B, 12] and
    ``yref`` [B, N, 5] (a clone: the controller's buffers are overwritten by its next step).  With ``weights`` [B, 7] the step is
    preceded by ``ctl.set_weights(weights.detach())``, runs with ``sens_w=True`` and is differentiable with respect to them too;
    ``weights=None`` leaves the controller's weights alone and touches it through ``step`` only."""
    import torch

    if invalid not in ("nan", "zero"):
        raise ValueError(f"invalid must be 'nan' or 'zero', got {invalid!r}")
    if "sens" in step_kw or "sens_w" in step_kw:
        raise ValueError("differentiable_step asks for the sensitivities itself: do not pass sens or sens_w")
    if yref is not None and (yref.dim() != 3 or yref.shape[-1] != 5):
        raise ValueError(f"a differentiable reference has shape [B, N, 5], got {tuple(yref.shape)}")
    if weights is not None and (weights.dim() != 2 or weights.shape[-1] != 7):
        raise ValueError(f"differentiable weights have shape [B, 7], got {tuple(weights.shape)}")

    class _Step(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, y, w):
            if w is None:
                out = ctl.step(x.detach(), yref=None if y is None else y.detach(), sens=True, **step_kw)
            else:
                ctl.set_weights(w.detach())
                out = ctl.step(x.detach(), yref=None if y is None else y.detach(), sens_w=True, **step_kw)
            jx, jy, ok = out["du0_dx"].clone(), out["du0_dyref"].clone(), out["sens_valid"] != 0
            jw = None if w is None else out["du0_dw"].clone()
            if invalid == "zero":
                jx = torch.where(ok[:, None, None], jx, torch.zeros_like(jx))
                jy = torch.where(ok[:, None, None, None], jy, torch.zeros_like(jy))
                if jw is not None:
                    jw = torch.where(ok[:, None, None], jw, torch.zeros_like(jw))
            ctx.save_for_backward(*((jx, jy) if jw is None else (jx, jy, jw)))
            ctx.has_y, ctx.has_w = y is not None, w is not None
            return out["u0"].clone()

        @staticmethod
        def backward(ctx, g):
            jx, jy = ctx.saved_tensors[:2]
            gx = torch.einsum("bu,bux->bx", g, jx) if ctx.needs_input_grad[0] else None
            gy = torch.einsum("bu,bkcu->bkc", g, jy) if ctx.has_y and ctx.needs_input_grad[1] else None
            gw = torch.einsum("bu,bpu->bp", g, ctx.saved_tensors[2]) if ctx.has_w and ctx.needs_input_grad[2] else None
            return gx, gy, gw

    return _Step.apply(xhat, yref, weights)
