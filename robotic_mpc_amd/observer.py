"""DisturbanceObserver: the input-disturbance estimate that ``BatchController.step(x, dist=d_hat)`` takes (offset-free MPC).

Per joint the prediction model's velocity state obeys ``v+ = a22 v + b2 (u + d)`` with ``a22 = exp(-wcv dt)``, ``b2 = 1 - a22``
(the exact discretisation behind ``mpcb_step_dist``, include/mpcbatch.h), and a constant input disturbance obeys ``d+ = d``.  The
observer is a two-state Luenberger predictor on ``(v, d)`` with the measured joint velocity as its output:

    [v^; d^]+ = A [v^; d^] + B u + L (v_meas - v^),     A = [[a22, b2], [0, 1]],  B = [b2; 0],  C = [1, 0],

whose estimation error obeys ``e+ = (A - L C) e`` exactly while the plant is that model with a constant ``d``.  Both error poles are
placed at ``pole``, in closed form: ``l1 = a22 + 1 - 2 pole``, ``l2 = (1 - pole)^2 / b2``; ``pole = 0`` is deadbeat (the error is
zero after two updates).  Pole placement rather than a steady-state Kalman gain: without process noise on ``q`` and ``v`` the latter
leaves a pole at 0.99 for ``dt = 0.01`` whatever the covariances, 1800 steps to 1e-8.

Batched ``[B, 6]`` torch tensors on whatever device ``wcv`` / the measurements live on, so a closed loop stays on the GPU; CPU tensors
work the same.

    obs = DisturbanceObserver(wcv, dt, pole=0.2)
    u_prev = torch.zeros(B, 6, dtype=torch.float64, device="cuda")
    for k in range(steps):
        d_hat = obs.update(x, u_prev)                # x = measured [q; qdot] at step k, u_prev = the input applied over step k-1
        u_prev = ctl.step(x, dist=d_hat)["u0"].clone()
        x = my_plant(x, u_prev)

Rollouts run the same observer on the device (configuration key ``disturbance_observer``: ``{"pole": p}``, mpcb_rollout_obs), with
the gains of ``observer_gains``: the closed loop above in one launch, over the plant of ``plant_perturbation``.

Not offered: measurement-noise tuning beyond the choice of ``pole``, a disturbance that varies over the horizon.
"""
from __future__ import annotations

import numpy as np


KEY = "disturbance_observer"


def observer_gains(wcv, dt: float, pole: float):
    """The gains that place both error poles of the per-joint predictor at ``pole``: ``l1 = a22 + 1 - 2 pole``,
    ``l2 = (1 - pole)^2 / b2`` with ``a22 = exp(-wcv dt)``, ``b2 = 1 - a22``.  ``wcv`` [..., 6] a sequence, numpy array or torch
    tensor; returns ``(l1, l2)`` of its kind and shape (float64)."""
    if not (0.0 <= float(pole) < 1.0):
        raise ValueError(f"pole must lie in [0, 1), got {pole!r}")
    if not float(dt) > 0.0:
        raise ValueError(f"dt must be > 0, got {dt!r}")
    if hasattr(wcv, "exp") and hasattr(wcv, "dim"):      # a torch tensor
        a22 = (-wcv.double() * float(dt)).exp()
    else:
        a22 = np.exp(-np.asarray(wcv, dtype=np.float64) * float(dt))
    b2 = 1.0 - a22                                        # (as the engines pack it: mpc_pack.h)
    return a22 + 1.0 - 2.0 * float(pole), (1.0 - float(pole)) ** 2 / b2


def validate(spec) -> None:
    """The configuration key ``disturbance_observer``: ``{"pole": p}``, 0 <= p < 1 (ValueError otherwise)."""
    if not isinstance(spec, dict) or set(spec) != {"pole"}:
        raise ValueError(f"{KEY} must be {{'pole': p}} or None, got {spec!r}")
    try:
        p = float(spec["pole"])
    except (TypeError, ValueError):
        raise ValueError(f"{KEY}.pole must be a number in [0, 1), got {spec['pole']!r}") from None
    if not (0.0 <= p < 1.0):
        raise ValueError(f"{KEY}.pole must lie in [0, 1), got {spec['pole']!r}")


def stack(cfgs) -> np.ndarray:
    """The gain array of a bucket of resolved configurations as mpcb_rollout_obs takes it: [B, 12] = l1 [6] | l2 [6], from each
    simulation's MODEL bandwidths, dt and pole."""
    out = np.zeros((len(cfgs), 12))
    for i, c in enumerate(cfgs):
        l1, l2 = observer_gains(c["wcv"], c["dt"], c[KEY]["pole"])
        out[i, :6], out[i, 6:] = l1, l2
    return out


class DisturbanceObserver:
    """``wcv``: the model's joint bandwidths, [6] or [B, 6] (a sequence, numpy array or torch tensor; its device becomes the
    observer's); ``dt``: the sampling time; ``pole``: where both poles of the error dynamics sit, 0 <= pole < 1."""

    def __init__(self, wcv, dt: float, pole: float = 0.5):
        import torch

        if not (0.0 <= float(pole) < 1.0):
            raise ValueError(f"pole must lie in [0, 1), got {pole!r}")
        if not float(dt) > 0.0:
            raise ValueError(f"dt must be > 0, got {dt!r}")
        w = wcv if isinstance(wcv, torch.Tensor) else torch.as_tensor(np.asarray(wcv, dtype=np.float64))
        w = w.to(torch.float64)
        if w.shape[-1] != 6 or w.dim() not in (1, 2):
            raise ValueError(f"wcv must have shape (6,) or (B, 6), got {tuple(w.shape)}")
        if not bool((w > 0).all()):
            raise ValueError("wcv must be > 0")
        self.dt, self.pole = float(dt), float(pole)
        self.a22 = torch.exp(-w * self.dt)
        self.b2 = 1.0 - self.a22                          # (as the engines pack it: mpc_pack.h)
        self.l1, self.l2 = observer_gains(w, self.dt, self.pole)
        self.reset()

    def reset(self):
        """Forgets the estimate: the next ``update`` starts again from its measurement with ``d_hat = 0``."""
        self._v = None      # v^ of the last measurement's time
        self._d = None      # d^ likewise
        self._y = None      # the last measured velocity

    def update(self, x_meas, u_applied):
        """One step of the predictor.  ``x_meas`` [B, 12] = [q; qdot] measured now, ``u_applied`` [B, 6] the input that was applied
        over the sampling interval that ends now.  Returns ``d_hat`` [B, 6] (a new tensor), the estimate for the interval that
        starts now.  The first call after construction or ``reset()`` has no interval behind it: it takes the measured velocity as
        ``v^``, returns zeros and does not read ``u_applied``; from then on every call propagates the estimate with the innovation
        of the previous measurement, so that the error obeys ``e+ = (A - L C) e`` from the first call on."""
        import torch

        y = x_meas[..., 6:].to(torch.float64)
        if self._v is None:
            self._v, self._d, self._y = y.clone(), torch.zeros_like(y), y.clone()
            return self._d.clone()
        u = u_applied.to(torch.float64)
        innov = self._y - self._v
        v = self.a22 * self._v + self.b2 * (u + self._d) + self.l1 * innov
        d = self._d + self.l2 * innov
        self._v, self._d, self._y = v, d, y.clone()
        return d.clone()

    def error_matrix(self):
        """``A - L C`` per joint: [..., 6, 2, 2] (leading dimensions those of ``wcv``), rows and columns ordered (v, d)."""
        import torch

        one, zero = torch.ones_like(self.a22), torch.zeros_like(self.a22)
        return torch.stack([torch.stack([self.a22 - self.l1, self.b2], dim=-1), torch.stack([-self.l2, one + zero], dim=-1)], dim=-2)
