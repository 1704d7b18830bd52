"""BatchController: the MPC solve as a batched controller for a plant the caller owns.

Where ``Simulator.run`` closes the loop over the engine's own plant, a controller takes B measured states and returns B
controls -- acados' ``set(0, 'lbx', x); solve(); get(0, 'u')`` (simulator.py:210-221) for a whole batch in one launch
(``mpcb_setup_controller_on`` / ``mpcb_step``, include/mpcbatch.h), on the latency engine or the throughput engine.  Between
steps every simulation keeps its iterate, linearisation and QP memory on the device: step k warm-starts from step k-1, as
acados does.

    ctl = BatchController([base_params(prediction_horizon=50) for _ in range(256)])
    x = torch.tensor(x0, dtype=torch.float64, device="cuda")     # [256, 12] q; qdot
    for k in range(steps):
        u = ctl.step(x)["u0"]                                       # [256, 6] on the device
        x = my_plant(x, u)

A controller regulates to the task reference packed from each configuration (``px_ref``, ``vy_ref``) unless it is given one
with ``set_reference`` / ``step(..., yref=...)``: per simulation and per stage of the horizon, like acados'
``set(k, 'yref', ...)`` between solves, and in force until it is changed (``default_reference()`` is the packed one).

Each simulation chooses per step how its solver memory enters the step: ``step(..., shift=True)`` (or a [B] bool mask) moves
the previous solution one stage towards stage 0 first -- the shift initialisation of a receding horizon whose schedule
advances one stage per step -- and ``reset(mask)`` restarts the masked simulations alone (an episode that ended, a solve that
failed) while the others keep their warm start.

``step(..., sens=True)`` also returns the local law behind ``u0``: the feedback gain ``du0_dx`` and the sensitivity to the task
reference ``du0_dyref`` of the step's QP, exact wherever the bound-inactive fast path solved it (``sens_valid``);
``robotic_mpc_amd.autograd.differentiable_step`` wraps them into a torch autograd function.

``set_weights(w)`` changes the seven cost weights (w_u, w_qddot and the task weights of g1..g5) between steps without building
another controller -- the warm start carries -- and ``step(..., sens_w=True)`` also returns ``du0_dw``, the sensitivity of ``u0``
to them: what a gradient-based tuning of a batch of controllers needs (``differentiable_step(..., weights=w)``).

``set_terminal_cost(P, x_ref)`` closes the horizon with a joint-wise quadratic terminal cost around a terminal reference (SQP_RTI
controllers): one 2x2 block per joint, the shape of the discrete LQR cost-to-go of the prediction model
(``robotic_mpc_amd.terminal.lqr_terminal`` designs one).  While it is in force ``step(..., sens=True)`` also returns ``du0_dxe``.

``set_input_disturbance(d)`` / ``step(x, dist=d)`` tell the prediction model about a constant input disturbance (SQP_RTI
controllers): it becomes ``x+ = Ad x + Bd (u + d)``, and with an estimate of ``d`` (``robotic_mpc_amd.observer.DisturbanceObserver``)
the controller tracks without the offset a disturbed plant otherwise leaves -- offset-free MPC.  Not offered together with ``sens``,
``sens_w`` or a terminal cost; ``d u0 / d d``, a per-stage disturbance profile and full SQP are not offered either.  Rollouts run
the same observer on the device (configuration key ``disturbance_observer``, mpcb_rollout_obs).

``set_surface(coeffs)`` / ``step(x, surface=coeffs)`` put a stage-varying surface under the horizon (SQP_RTI controllers): stage
``k`` evaluates the task functions on the quadric ``coeffs[:, k]`` = a..f instead of the packed ``surface_coeffs`` -- a workpiece
that moves, or a free-form surface handed over patch by patch (``robotic_mpc_amd.surface``).  Not offered together with ``sens``,
``sens_w``, a terminal cost or an input disturbance.  Rollouts take the whole table (configuration key ``surface_schedule``,
mpcb_rollout_surf).
"""
from __future__ import annotations

from typing import Dict, Mapping, Optional, Sequence

import numpy as np

from . import config as cfgmod, packing
from .engine import CONTROLLER_ENGINES, STEP_FIELDS, WARM_RESET, WARM_SHIFT, MpcBatchEngine

NREF = 5    # task outputs with a reference (MPCB_NREF, include/mpcbatch.h)
NWEIGHT = 7  # cost weights that can change at run time (MPCB_NWEIGHT): w_u, w_qddot, the task weights of g1..g5
NTERM = 30   # doubles of a simulation's terminal cost (MPCB_NTERM): pqq[6] pqv[6] pvv[6] x_e[12]


class BatchController:
    """One MPC controller per configuration, all solved together on one GPU.

    ``configs`` are the per-simulation dicts ``Simulator`` / ``SimulationManager`` take (``config.base_params``); they must
    share one launch bucket (same solver options, robot and ``simulation_time / dt``) and use fp64 Riccati.  Their ``q_0`` /
    ``qdot_0`` seed the initial guess of the iterate (x_k = [q_0; qdot_0], u_k = 0), exactly as in a rollout.

    ``engine`` picks the kernel family of the step:

    * ``"latency"`` (the default): one workgroup of 4-8 wavefronts per simulation; one prediction horizon for the batch.
    * ``"stream"``: the throughput engine, one wavefront per simulation -- the faster one for large batches.  It also takes
      configurations of DIFFERENT prediction horizons with SQP_RTI (a ragged batch, e.g. a grid over ``prediction_horizon``).
    * ``"auto"``: ragged batches go to the throughput engine, the only one that runs them; a uniform batch goes there from
      ``MPCB_STREAM_MIN_BATCH_STEP`` (1280) SQP_RTI simulations on, the batch size from which it measured faster, and to the
      latency engine below; a uniform full-SQP batch always goes to the latency engine, since one step launch lasts as long as its
      slowest simulation's SQP iterations, which four wavefronts run faster than one (include/mpcbatch.h).
      ``launch_info()["engine"]`` tells which.

    ``horizons`` holds each configuration's horizon and ``N`` the longest: the prediction buffers have N + 1 / N rows, and the
    rows beyond a configuration's own horizon are NaN.  Anything the chosen engine cannot run raises ``ValueError`` before
    the device is touched; without a GPU, construction raises ``EngineError``.
    """

    # run-time cost weights (set_weights): the controller's own [B, 7] device buffer (None: the packed weights are in force) and
    # the stream that last wrote the device records; the du0_dw buffer of step(sens_w=True), from the first use
    _weights = None
    _weights_stream = None
    _sensw = None
    # terminal cost (set_terminal_cost): the controller's own [B, 30] device buffer, whether it is in force, whether the next step
    # must tell the device that it changed, the stream that last wrote it; the du0_dxe buffer of step(sens=True), from the first use
    _term = None
    _term_on = False
    _term_changed = False
    _term_stream = None
    _sensxe = None
    # input disturbance (set_input_disturbance): the controller's own [B, 6] device buffer, whether it is in force, whether the next
    # step must tell the device that it changed, the stream that last wrote it
    _dist = None
    _dist_on = False
    _dist_changed = False
    _dist_stream = None
    # surface window (set_surface): the controller's own [B, N, 6] device buffer, whether it is in force, whether the next step must
    # linearise again because of it, the stream of the last copy into it
    _surf = None
    _surf_on = False
    _surf_changed = False
    _surf_stream = None
    # BatchController(combined=True): the three above and the shift may be in force together (mpcb_step_combined)
    _combined = False

    def __init__(self, configs: Sequence[Mapping], device: int = 0, engine: str = "latency", combined: bool = False):
        """``combined=True`` (opt-in, SQP_RTI only): ``set_terminal_cost``, ``set_input_disturbance`` / ``step(dist=)``,
        ``set_surface`` / ``step(surface=)`` and ``step(shift=)`` may all be in force together; every step then runs the combined
        controller step (include/mpcbatch.h, mpcb_step_combined), with neutral data for whatever is switched off, and
        ``sens`` / ``sens_w`` are refused.  Without it nothing changes: each of the three refuses the other two."""
        if engine not in CONTROLLER_ENGINES:
            raise ValueError(f"engine must be one of {sorted(CONTROLLER_ENGINES)}, got {engine!r}")
        if len(configs) == 0:
            raise ValueError("BatchController needs at least one configuration")
        cfgs = [cfgmod.resolve_config(c) for c in configs]
        horizons = np.array([c["N"] for c in cfgs], dtype=np.int64)
        ragged = bool((horizons != horizons[0]).any())
        if ragged and engine == "latency":
            raise ValueError("configurations of different prediction horizons need engine='stream' or 'auto': the latency "
                             "engine's controller step needs one horizon for the whole batch")
        key0 = packing.bucket_key(cfgs[0], ragged=engine != "latency")
        for i, c in enumerate(cfgs[1:], 1):
            if packing.bucket_key(c, ragged=engine != "latency") != key0:
                raise ValueError(f"configuration {i} does not share the bucket of configuration 0: one controller batch needs "
                                 "the same solver options, robot and simulation_time / dt (and, on the latency engine, one "
                                 "prediction horizon)")
        if ragged and cfgs[0]["solver_type"] != packing.SOLVER_RTI:
            raise ValueError("configurations of different prediction horizons share a controller batch only with SQP_RTI")
        if cfgs[0]["precision"] != 0:
            raise ValueError("riccati_precision='fp32' is refused by the controller step on every engine: it is fp64 only")
        from .simulator import chain_for

        if combined and cfgs[0]["solver_type"] != packing.SOLVER_RTI:
            raise ValueError("BatchController(combined=True) needs SQP_RTI configurations: the combined step is not offered with full SQP")
        self._combined = bool(combined)
        chain = chain_for(cfgs[0])
        self.configs = cfgs
        self.horizons = horizons
        self.batch, self.N = len(cfgs), int(horizons.max())
        self.engine = MpcBatchEngine(device)
        self.device = self.engine.device
        self.engine.setup_controller(cfgs, chain, engine=engine)
        self._bufs: Optional[Dict] = None
        self._reset = True
        # task reference: the controller's own [B, N, 5] device buffer, whether it is in force, whether the next step must tell
        # the device that it changed, and the streams that last wrote / read it
        self._yref = None
        self._ref_on = False
        self._ref_changed = False
        self._ref_stream = None
        self._step_stream = None
        # per-simulation warm start: the simulations reset(mask) marked for the next step ([B] bool, host or device), and the
        # controller's own int32 [B] mode buffer the step composes on its stream
        self._reset_mask = None
        self._warm = None
        # sensitivities of u0 (step(sens=True)): the controller's own du0_dx / du0_dyref / sens_valid buffers, from the first use
        self._sens = None

    def _check_mask(self, mask, name):
        """Validates a per-simulation mask ([B] bool, a numpy array or a tensor on the controller's device) without touching the
        device; returns it."""
        import torch

        if isinstance(mask, np.ndarray):
            shape, dtype_ok = tuple(mask.shape), mask.dtype == np.bool_
        elif isinstance(mask, torch.Tensor):
            shape, dtype_ok = tuple(mask.shape), mask.dtype == torch.bool
            if mask.device.type != "cuda" or mask.device.index != self.device:
                raise ValueError(f"{name} must live on cuda:{self.device}, got {mask.device}")
        else:
            raise ValueError(f"{name} must be a bool torch tensor or numpy array of shape ({self.batch},), got {type(mask).__name__}")
        if shape != (self.batch,):
            raise ValueError(f"{name} must have shape ({self.batch},), got {shape}")
        if not dtype_ok:
            raise ValueError(f"{name} must be bool, got {mask.dtype}")
        return mask

    def _buffers(self, predict: bool):
        """The output buffers of a step; x_pred / u_pred ([B, N+1, 12] + [B, N, 6], N the longest horizon) only from the first step
        that asks for them."""
        import torch

        if self._bufs is None:
            self._bufs = {}
        want = [f for f in STEP_FIELDS if f[0] != "xhat" and (predict or f[0] not in ("x_pred", "u_pred"))]
        for name, ty, shp in want:
            if name not in self._bufs:
                self._bufs[name] = torch.zeros((self.batch,) + shp(self.N), dtype=torch.float64 if ty == "f8" else torch.int32,
                                               device=torch.device("cuda", self.device))
        return {name: self._bufs[name] for name, _, _ in want}

    def _xhat(self, xhat):
        import torch

        if isinstance(xhat, np.ndarray):
            if xhat.dtype != np.float64 or xhat.shape != (self.batch, 12):
                raise ValueError(f"xhat must be float64 of shape ({self.batch}, 12), got {xhat.dtype} {xhat.shape}")
            return torch.from_numpy(np.ascontiguousarray(xhat)).to(torch.device("cuda", self.device))
        if not isinstance(xhat, torch.Tensor):
            raise ValueError(f"xhat must be a torch tensor or a numpy array, got {type(xhat).__name__}")
        if xhat.dtype != torch.float64 or tuple(xhat.shape) != (self.batch, 12):
            raise ValueError(f"xhat must be float64 of shape ({self.batch}, 12), got {xhat.dtype} {tuple(xhat.shape)}")
        if xhat.device.type != "cuda" or xhat.device.index != self.device:
            raise ValueError(f"xhat must live on cuda:{self.device}, got {xhat.device}")
        return xhat.contiguous()

    def default_reference(self):
        """Each configuration's packed task reference g_ref = [0, 1, 0, px_ref, vy_ref] on every stage: a [B, N, 5] float64
        tensor on the controller's device (a new one per call), the natural start for a reference schedule."""
        import torch

        g = np.zeros((self.batch, NREF))
        g[:, 1] = 1.0
        g[:, 3] = [c["px_ref"] for c in self.configs]
        g[:, 4] = [c["vy_ref"] for c in self.configs]
        return torch.from_numpy(np.repeat(g[:, None, :], self.N, axis=1)).to(torch.device("cuda", self.device))

    def _check_reference(self, yref):
        """Validates a reference ([B, N, 5] or [B, 5], float64, a numpy array or a tensor on the controller's device) without
        touching the device; returns it as a [B, N, 5] or [B, 1, 5] array / tensor."""
        import torch

        B, N = self.batch, self.N
        if isinstance(yref, np.ndarray):
            arr, shape, dtype_ok = yref, tuple(yref.shape), yref.dtype == np.float64
        elif isinstance(yref, torch.Tensor):
            arr, shape, dtype_ok = yref, tuple(yref.shape), yref.dtype == torch.float64
            if yref.device.type != "cuda" or yref.device.index != self.device:
                raise ValueError(f"yref must live on cuda:{self.device}, got {yref.device}")
        else:
            raise ValueError(f"yref must be a torch tensor, a numpy array or None, got {type(yref).__name__}")
        if shape not in ((B, N, NREF), (B, NREF)):
            raise ValueError(f"yref must have shape ({B}, {N}, {NREF}) or ({B}, {NREF}), got {shape}")
        if not dtype_ok:
            raise ValueError(f"yref must be float64, got {yref.dtype}")
        if isinstance(arr, np.ndarray):
            # the rows a simulation's horizon reads must be finite (a ragged batch never reads rows k >= horizons[i])
            rows = arr if len(shape) == 2 else arr[np.arange(N)[None, :] < self.horizons[:, None]]
            if not np.isfinite(rows).all():
                raise ValueError("yref has non-finite entries in rows a simulation's horizon reads")
        return arr[:, None, :] if len(shape) == 2 else arr

    def set_reference(self, yref):
        """Sets the task reference the following steps track: ``yref[i, k]`` is the target of the task outputs g1..g5 of
        simulation i at stage k = 0..N-1 (N the longest horizon; on a ragged batch rows k >= ``horizons[i]`` are not read), in
        place of the packed ``[0, 1, 0, px_ref, vy_ref]``; a [B, 5] reference holds for the whole horizon.  The targets of the
        input and joint-acceleration cost rows stay 0.  The reference is copied into the controller's own device buffer (later
        edits of ``yref`` have no effect) and stays in force until it is set again -- ``reset()`` keeps it; ``None`` returns to
        the packed references.  The next step linearises again first, since its carried linearisation was formed against the
        old reference."""
        import torch

        if yref is None:
            if self._ref_on:
                self._ref_on, self._ref_changed = False, True
            return
        arr = self._check_reference(yref)
        dev = torch.device("cuda", self.device)
        cur = torch.cuda.current_stream(self.device)
        if self._yref is None:
            self._yref = torch.empty((self.batch, self.N, NREF), dtype=torch.float64, device=dev)
        if self._step_stream is not None and self._step_stream != cur:
            cur.wait_stream(self._step_stream)        # a step still reading the buffer on another stream finishes first
        src = torch.from_numpy(np.ascontiguousarray(arr)).to(dev) if isinstance(arr, np.ndarray) else arr
        self._yref.copy_(src.expand(self.batch, self.N, NREF))
        self._ref_stream = cur
        self._ref_on, self._ref_changed = True, True

    def packed_weights(self) -> np.ndarray:
        """The cost weights of the configurations the controller was built from: [B, 7] float64 (w_u, w_qddot, the task weights
        of g1..g5), a new numpy array."""
        return np.array([[c["w_u"], c["w_qddot"], *np.asarray(c["w_task"], dtype=np.float64)] for c in self.configs], dtype=np.float64)

    def _check_weights(self, w):
        """Validates cost weights ([B, 7] or [7], float64, a numpy array or a tensor on the controller's device) without touching
        the device; returns them as a [B, 7] or [1, 7] array / tensor."""
        import torch

        B = self.batch
        if isinstance(w, np.ndarray):
            shape, dtype_ok = tuple(w.shape), w.dtype == np.float64
        elif isinstance(w, torch.Tensor):
            shape, dtype_ok = tuple(w.shape), w.dtype == torch.float64
            if w.device.type != "cuda" or w.device.index != self.device:
                raise ValueError(f"weights must live on cuda:{self.device}, got {w.device}")
        else:
            raise ValueError(f"weights must be a torch tensor, a numpy array or None, got {type(w).__name__}")
        if shape not in ((B, NWEIGHT), (NWEIGHT,)):
            raise ValueError(f"weights must have shape ({B}, {NWEIGHT}) or ({NWEIGHT},), got {shape}")
        if not dtype_ok:
            raise ValueError(f"weights must be float64, got {w.dtype}")
        w = w[None, :] if len(shape) == 1 else w
        if isinstance(w, np.ndarray):
            if not np.isfinite(w).all():
                raise ValueError("weights has non-finite entries")
            if (w < 0.0).any():
                raise ValueError("weights must be >= 0")
            lm = np.array([c.get("levenberg_marquardt", 0.0) for c in self.configs], dtype=np.float64)
            if not (w[:, 0] + w[:, 1] + lm > 0.0).all():
                raise ValueError("w_u + w_qddot + levenberg_marquardt must be > 0 for every simulation: the input Hessian is singular otherwise")
        return w

    def set_weights(self, w):
        """Sets the cost weights the following steps use: ``w[i]`` = (w_u, w_qddot, the task weights of g1..g5) of simulation i,
        [B, 7] float64, or [7] for the whole batch; a numpy array or a tensor on the controller's device.  The weights are copied
        into the controller's own device buffer (later edits of ``w`` have no effect) and from there into the device's parameter
        records, and stay in force -- across ``reset()`` too -- until they are set again; ``None`` returns to the weights of the
        configurations.  The next step linearises again first, as after a new reference; the iterate, the multipliers, the QP
        memory and the fast-path suspension carry.  A numpy array is validated before the device is touched (shape, dtype, finite,
        every weight >= 0, w_u + w_qddot + levenberg_marquardt > 0); the values of a device tensor are the caller's to keep valid."""
        import torch

        arr = self.packed_weights() if w is None else self._check_weights(w)
        dev = torch.device("cuda", self.device)
        cur = torch.cuda.current_stream(self.device)
        if self._weights is None:
            self._weights = torch.empty((self.batch, NWEIGHT), dtype=torch.float64, device=dev)
        # a step still running on another stream finishes first (it reads the records), and so does an earlier update
        for other in (self._step_stream, self._weights_stream):
            if other is not None and other != cur:
                cur.wait_stream(other)
        src = torch.from_numpy(np.ascontiguousarray(arr)).to(dev) if isinstance(arr, np.ndarray) else arr
        self._weights.copy_(src.expand(self.batch, NWEIGHT))
        self.engine.set_weights(self._weights, stream=cur.cuda_stream)
        self._weights_stream = cur

    def weights(self):
        """The cost weights in force: a new [B, 7] float64 tensor on the controller's device."""
        import torch

        if self._weights is None:
            return torch.from_numpy(self.packed_weights()).to(torch.device("cuda", self.device))
        cur = torch.cuda.current_stream(self.device)
        if self._weights_stream is not None and self._weights_stream != cur:
            cur.wait_stream(self._weights_stream)
        return self._weights.clone()

    def _check_terminal(self, P, x_ref):
        """Validates a terminal cost without touching the device -- ``P`` as blocks [B, 6, 3] / [6, 3] (pqq, pqv, pvv per joint) or
        as a symmetric matrix [B, 12, 12] / [12, 12] over [q; qdot], ``x_ref`` [B, 12] / [12]; float64, numpy arrays or tensors on the
        controller's device -- and returns (blocks [B or 1, 6, 3], x_ref [B or 1, 12]) of the same kind."""
        import torch

        B = self.batch
        if self.configs[0]["solver_type"] != packing.SOLVER_RTI:
            raise ValueError("set_terminal_cost needs an SQP_RTI controller: the terminal cost is not offered with full SQP")
        out = []
        for name, a, shapes in (("P", P, ((B, 6, 3), (6, 3), (B, 12, 12), (12, 12))), ("x_ref", x_ref, ((B, 12), (12,)))):
            if isinstance(a, np.ndarray):
                shape, dtype_ok = tuple(a.shape), a.dtype == np.float64
            elif isinstance(a, torch.Tensor):
                shape, dtype_ok = tuple(a.shape), a.dtype == torch.float64
                if a.device.type != "cuda" or a.device.index != self.device:
                    raise ValueError(f"{name} must live on cuda:{self.device}, got {a.device}")
            else:
                raise ValueError(f"{name} must be a torch tensor or a numpy array, got {type(a).__name__}")
            if shape not in shapes:
                raise ValueError(f"{name} must have one of the shapes {shapes}, got {shape}")
            if not dtype_ok:
                raise ValueError(f"{name} must be float64, got {a.dtype}")
            if isinstance(a, np.ndarray) and not np.isfinite(a).all():
                raise ValueError(f"{name} has non-finite entries")
            out.append(a if len(shape) == len(shapes[0]) else a[None])
        Pm, xe = out
        if Pm.shape[-1] == 12:
            j = np.arange(6)
            if isinstance(Pm, np.ndarray):
                # the joint-block pattern exactly: nothing outside the (q_j, qdot_j) blocks, and the two off-diagonal entries of a
                # block equal up to rounding (the upper one is taken)
                rest = Pm.copy()
                rest[:, j, j] = 0.0; rest[:, 6 + j, 6 + j] = 0.0; rest[:, j, 6 + j] = 0.0; rest[:, 6 + j, j] = 0.0
                if (rest != 0.0).any():
                    b, r, c = (int(v[0]) for v in np.nonzero(rest))
                    raise ValueError(f"P[{r}, {c}] = {rest[b, r, c]!r} (simulation {b}) lies outside the joint blocks (q_j, qdot_j): the "
                                     "terminal cost is joint-wise; full 12x12 weights are not offered")
                asym = np.abs(Pm[:, j, 6 + j] - Pm[:, 6 + j, j])
                if (asym > 1e-12 * max(float(np.abs(Pm).max()), 1e-300)).any():
                    b, jj = (int(v[0]) for v in np.nonzero(asym > 1e-12 * np.abs(Pm).max()))
                    raise ValueError(f"P is not symmetric: P[{jj}, {6 + jj}] != P[{6 + jj}, {jj}] (simulation {b})")
                blocks = np.stack([Pm[:, j, j], Pm[:, j, 6 + j], Pm[:, 6 + j, 6 + j]], axis=2)
            else:
                blocks = torch.stack([Pm[:, j, j], Pm[:, j, 6 + j], Pm[:, 6 + j, 6 + j]], dim=2)
        else:
            blocks = Pm
        if isinstance(blocks, np.ndarray):
            pqq, pqv, pvv = blocks[..., 0], blocks[..., 1], blocks[..., 2]
            if (pqq < 0.0).any() or (pvv < 0.0).any() or (pqq * pvv < pqv * pqv).any():
                raise ValueError("every joint block of P must be positive semidefinite: pqq >= 0, pvv >= 0, pqq pvv >= pqv^2")
        return blocks, xe

    def set_terminal_cost(self, P, x_ref=None):
        """Puts a joint-wise terminal cost in force (SQP_RTI controllers; ``ValueError`` on a full-SQP one): the following steps
        minimise, besides the stage costs, ``1/2 (x_N - x_ref)' P (x_N - x_ref)`` at the last stage of each simulation's own horizon,
        not scaled by dt.  ``P`` is given as blocks [B, 6, 3] or [6, 3] -- (pqq, pqv, pvv) of the symmetric 2x2 block of joint j over
        (q_j, qdot_j) -- or as a symmetric matrix [B, 12, 12] or [12, 12] over [q; qdot] that has exactly that pattern (any other
        non-zero entry raises ``ValueError`` naming it); ``x_ref`` is [B, 12] or [12].  float64 numpy arrays or tensors on the
        controller's device; they are copied into the controller's own buffer (later edits have no effect).  The setting stays in
        force across steps and ``reset()`` until it is set again; ``set_terminal_cost(None)`` switches the terminal cost off.  The
        next step linearises again first, as after a new reference; everything else carries.  A numpy input is validated before the
        device is touched (shape, dtype, finite, every block positive semidefinite: pqq, pvv >= 0, pqq pvv >= pqv^2); the values of a
        device tensor are the caller's to keep valid.  All-zero blocks are exactly no terminal cost.
        ``robotic_mpc_amd.terminal.lqr_terminal`` designs the blocks of an LQR terminal weight."""
        import torch

        if P is None:
            if self._term_on:
                self._term_on, self._term_changed = False, True
            return
        if x_ref is None:
            raise ValueError("set_terminal_cost needs the terminal reference x_ref with P")
        if self._surf_on and not self._combined:
            raise ValueError("a terminal cost is not offered while a surface window is in force (set_surface(None) switches it off)")
        if self._dist_on and not self._combined:
            raise ValueError("a terminal cost is not offered while an input disturbance is in force (set_input_disturbance(None) "
                             "switches it off)")
        blocks, xe = self._check_terminal(P, x_ref)
        dev = torch.device("cuda", self.device)
        cur = torch.cuda.current_stream(self.device)
        if self._term is None:
            self._term = torch.empty((self.batch, NTERM), dtype=torch.float64, device=dev)
        if self._step_stream is not None and self._step_stream != cur:
            cur.wait_stream(self._step_stream)        # a step still reading the buffer on another stream finishes first
        on_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if isinstance(a, np.ndarray) else a
        b = on_dev(blocks).expand(self.batch, 6, 3)
        self._term[:, 0:6].copy_(b[:, :, 0]); self._term[:, 6:12].copy_(b[:, :, 1]); self._term[:, 12:18].copy_(b[:, :, 2])
        self._term[:, 18:30].copy_(on_dev(xe).expand(self.batch, 12))
        self._term_stream = cur
        self._term_on, self._term_changed = True, True

    def terminal_cost(self):
        """The terminal cost in force: ``None``, or dict(blocks [B, 6, 3], x_ref [B, 12]) of new float64 tensors on the controller's
        device."""
        import torch

        if not self._term_on:
            return None
        cur = torch.cuda.current_stream(self.device)
        if self._term_stream is not None and self._term_stream != cur:
            cur.wait_stream(self._term_stream)
        t = self._term
        return dict(blocks=torch.stack([t[:, 0:6], t[:, 6:12], t[:, 12:18]], dim=2).clone(), x_ref=t[:, 18:30].clone())

    def _check_disturbance(self, d):
        """Validates an input disturbance ([B, 6] or [6], float64, a numpy array or a tensor on the controller's device) without
        touching the device; returns it as a [B, 6] or [1, 6] array / tensor."""
        import torch

        B = self.batch
        if self.configs[0]["solver_type"] != packing.SOLVER_RTI:
            raise ValueError("set_input_disturbance needs an SQP_RTI controller: the input disturbance is not offered with full SQP")
        if self._term_on and not self._combined:
            raise ValueError("an input disturbance is not offered while a terminal cost is in force (set_terminal_cost(None) "
                             "switches it off)")
        if self._surf_on and not self._combined:
            raise ValueError("an input disturbance is not offered while a surface window is in force (set_surface(None) switches it off)")
        if isinstance(d, np.ndarray):
            shape, dtype_ok = tuple(d.shape), d.dtype == np.float64
        elif isinstance(d, torch.Tensor):
            shape, dtype_ok = tuple(d.shape), d.dtype == torch.float64
            if d.device.type != "cuda" or d.device.index != self.device:
                raise ValueError(f"the input disturbance must live on cuda:{self.device}, got {d.device}")
        else:
            raise ValueError(f"the input disturbance must be a torch tensor, a numpy array or None, got {type(d).__name__}")
        if shape not in ((B, 6), (6,)):
            raise ValueError(f"the input disturbance must have shape ({B}, 6) or (6,), got {shape}")
        if not dtype_ok:
            raise ValueError(f"the input disturbance must be float64, got {d.dtype}")
        if isinstance(d, np.ndarray) and not np.isfinite(d).all():
            raise ValueError("the input disturbance has non-finite entries")
        return d[None, :] if len(shape) == 1 else d

    def set_input_disturbance(self, d):
        """Puts a constant input disturbance into the prediction model of the following steps (SQP_RTI controllers; ``ValueError``
        on a full-SQP one, and while a terminal cost is in force): ``d[i]`` in rad/s, the units of ``u``, [B, 6] float64 or [6] for
        the whole batch; a numpy array or a tensor on the controller's device.  The model becomes ``x+ = Ad x + Bd (u + d)`` over the
        whole horizon and the joint-acceleration cost row follows it; the input cost row and the bounds stay on ``u``
        (include/mpcbatch.h, mpcb_step_dist).  The values are copied into the controller's own device buffer (later edits of ``d``
        have no effect) and stay in force across steps and ``reset()`` until they are set again; ``None`` switches the disturbance
        off.  The next step linearises again first, as after a new reference; everything else carries.  A numpy array is validated
        before the device is touched (shape, dtype, finite); the values of a device tensor are the caller's to keep valid.
        ``robotic_mpc_amd.observer.DisturbanceObserver`` estimates ``d`` from the measured velocities."""
        import torch

        if d is None:
            if self._dist_on:
                self._dist_on, self._dist_changed = False, True
            return
        arr = self._check_disturbance(d)
        dev = torch.device("cuda", self.device)
        cur = torch.cuda.current_stream(self.device)
        if self._dist is None:
            self._dist = torch.empty((self.batch, 6), dtype=torch.float64, device=dev)
        if self._step_stream is not None and self._step_stream != cur:
            cur.wait_stream(self._step_stream)        # a step still reading the buffer on another stream finishes first
        src = torch.from_numpy(np.ascontiguousarray(arr)).to(dev) if isinstance(arr, np.ndarray) else arr
        self._dist.copy_(src.expand(self.batch, 6))
        self._dist_stream = cur
        self._dist_on, self._dist_changed = True, True

    def input_disturbance(self):
        """The input disturbance in force: ``None``, or a new [B, 6] float64 tensor on the controller's device."""
        import torch

        if not self._dist_on:
            return None
        cur = torch.cuda.current_stream(self.device)
        if self._dist_stream is not None and self._dist_stream != cur:
            cur.wait_stream(self._dist_stream)
        return self._dist.clone()

    def _check_surface(self, coeffs):
        """Validates a surface window ([B, N, 6] or [N, 6], float64, a numpy array or a tensor on the controller's device) without
        touching the device; returns it as a [B, N, 6] or [1, N, 6] array / tensor."""
        import torch

        B, N = self.batch, self.N
        if self.configs[0]["solver_type"] != packing.SOLVER_RTI:
            raise ValueError("set_surface needs an SQP_RTI controller: the scheduled surface is not offered with full SQP")
        if self._term_on and not self._combined:
            raise ValueError("a surface window is not offered while a terminal cost is in force (set_terminal_cost(None) "
                             "switches it off)")
        if self._dist_on and not self._combined:
            raise ValueError("a surface window is not offered while an input disturbance is in force (set_input_disturbance(None) "
                             "switches it off)")
        if isinstance(coeffs, np.ndarray):
            shape, dtype_ok = tuple(coeffs.shape), coeffs.dtype == np.float64
        elif isinstance(coeffs, torch.Tensor):
            shape, dtype_ok = tuple(coeffs.shape), coeffs.dtype == torch.float64
            if coeffs.device.type != "cuda" or coeffs.device.index != self.device:
                raise ValueError(f"the surface window must live on cuda:{self.device}, got {coeffs.device}")
        else:
            raise ValueError(f"the surface window must be a torch tensor, a numpy array or None, got {type(coeffs).__name__}")
        if shape not in ((B, N, 6), (N, 6)):
            raise ValueError(f"the surface window must have shape ({B}, {N}, 6) or ({N}, 6), got {shape}")
        if not dtype_ok:
            raise ValueError(f"the surface window must be float64, got {coeffs.dtype}")
        if isinstance(coeffs, np.ndarray) and not np.isfinite(coeffs).all():
            raise ValueError("the surface window has non-finite entries")
        return coeffs[None] if len(shape) == 2 else coeffs

    def set_surface(self, coeffs):
        """Puts a stage-varying surface under the following steps (SQP_RTI controllers; ``ValueError`` on a full-SQP one, and while
        a terminal cost or an input disturbance is in force): ``coeffs[i, k]`` = the six quadric coefficients a..f that stage ``k``
        of simulation ``i`` evaluates g1, g2 and their Jacobians on, [B, N, 6] float64 or [N, 6] for the whole batch (N the longest
        horizon; rows past ``horizons[i]`` are not read); a numpy array or a tensor on the controller's device
        (include/mpcbatch.h, mpcb_step_surf).  The values are copied into the controller's own device buffer and stay in force
        across steps and ``reset()`` until they are set again; ``None`` switches back to the packed ``surface_coeffs``.  The next
        step linearises again first, as after a new reference; everything else carries.  ``robotic_mpc_amd.surface`` builds such
        windows: rows ``[t, t + N)`` of ``surface.sample(cfg)`` are the window of closed-loop step ``t``."""
        import torch

        if coeffs is None:
            if self._surf_on:
                self._surf_on, self._surf_changed = False, True
            return
        arr = self._check_surface(coeffs)
        dev = torch.device("cuda", self.device)
        cur = torch.cuda.current_stream(self.device)
        if self._surf is None:
            self._surf = torch.empty((self.batch, self.N, 6), dtype=torch.float64, device=dev)
        if self._step_stream is not None and self._step_stream != cur:
            cur.wait_stream(self._step_stream)        # a step still reading the buffer on another stream finishes first
        src = torch.from_numpy(np.ascontiguousarray(arr)).to(dev) if isinstance(arr, np.ndarray) else arr
        self._surf.copy_(src.expand(self.batch, self.N, 6))
        self._surf_stream = cur
        self._surf_on, self._surf_changed = True, True

    def surface(self):
        """The surface window in force: ``None``, or a new [B, N, 6] float64 tensor on the controller's device."""
        import torch

        if not self._surf_on:
            return None
        cur = torch.cuda.current_stream(self.device)
        if self._surf_stream is not None and self._surf_stream != cur:
            cur.wait_stream(self._surf_stream)
        return self._surf.clone()

    def step(self, xhat, predict: bool = False, yref=None, shift=False, sens: bool = False, sens_w: bool = False, dist=None,
             surface=None) -> Dict:
        """One MPC step of every controller from the feedback states ``xhat`` ([B, 12] q; qdot, float64: a tensor on the
        controller's device, or a numpy array that is copied there).

        Returns device tensors: ``u0`` [B, 6] (the input to apply), ``status``, ``sqp_iter``, ``qp_iter`` [B] (int32),
        ``residuals`` [B, 4], ``cost``, ``solver_time`` [B]; with ``predict`` also the iterate's predicted trajectory
        ``x_pred`` [B, N+1, 12] and ``u_pred`` [B, N, 6] (N the longest horizon; rows past ``horizons[i]`` are NaN).  The launch is asynchronous on the current torch stream and nothing
        is synchronised.  The returned tensors are the controller's own buffers: the next ``step`` overwrites them, so clone
        what must outlive it.

        ``yref`` (optional) is ``set_reference(yref)`` before the step: the reference then stays in force for later steps.

        ``shift``: ``True`` starts every simulation that is not being reset from its previous solution moved one stage towards
        stage 0 (u_k <- u_{k+1} with the last input held, x_k <- x_{k+1} with x_N propagated by the model, multipliers and QP
        memory moved with their stages; include/mpcbatch.h, MPCB_WARM_SHIFT) and linearises there; a [B] bool mask (numpy, or a
        tensor on the controller's device) shifts those simulations only.  It applies to this step alone.  On the first step
        and after ``reset()`` there is nothing to shift: the step starts from the initial guess.

        ``sens=True`` (SQP_RTI only; ``ValueError`` on a full-SQP batch) adds ``du0_dx`` [B, 6, 12] = d u0 / d xhat,
        ``du0_dyref`` [B, N, 5, 6] with ``du0_dyref[i, k]`` = (d u0 / d yref_k)' and ``sens_valid`` [B] int32 (the controller's
        own buffers as well).  They are the exact Jacobians of this step's QP, the linearisation point held fixed, for every
        simulation whose QP an accepted bound-inactive fast-path attempt solved (``sens_valid`` 1): ``u0 + du0_dx (x - xhat)``
        is the local feedback law between two solves.  Row k = 0 of ``du0_dyref`` and, on a ragged batch, the rows past a
        simulation's own horizon are exactly zero.  Where the QP went through the interior-point loop (fast path off, attempt
        rejected or skipped during a back-off) or the status is not 0, ``sens_valid`` is 0 and every entry is NaN:
        sensitivities through active bounds are not provided, nor those of ``x_pred`` / ``u_pred``.  The step itself is
        unchanged by ``sens``.  The extra pass costs 12-20 % of the step rate at N = 100 (latency engine 13 / 15 / 20 % at batch 256 /
        1024 / 4096, throughput engine 12-14 %; ``profiles/controller_step_rate_sens.txt``); a step without ``sens`` costs what
        it did.

        ``sens_w=True`` implies ``sens`` and adds ``du0_dw`` [B, 7, 6] with ``du0_dw[i, p]`` = d u0 / d weight_p (the weights in
        the order of ``set_weights``; the controller's own buffer), NaN where ``sens_valid`` is 0.  It is the exact derivative of
        this step's QP, whose matrices are affine in the weights, with the linearisation point held fixed: the derivative of one
        real-time iteration.  Over several closed-loop steps the dependence of the carried iterate on the weights of earlier steps
        is not included.  A weight of 0 has its derivative; with a horizon of 1 the five task rows are exactly zero.
        Over a ``sens=True`` step it costs another 5-11 % of the step rate at N = 100 (latency engine 7 / 9 / 11 % at batch 256 / 1024 /
        4096, throughput engine 5-6 %; 18-28 % against a plain step; ``profiles/controller_step_rate_sensw.txt``); steps that do
        not ask cost what they did.

        While a terminal cost is in force (``set_terminal_cost``) the step's QP, ``cost`` and ``residuals`` include it,
        ``du0_dx`` / ``du0_dyref`` are the exact Jacobians of that QP, and ``sens=True`` adds ``du0_dxe`` [B, 6, 12] = d u0 / d x_ref
        of the terminal reference (NaN where ``sens_valid`` is 0; not zero with a horizon of 1).  ``sens_w=True`` then raises
        ``ValueError``: the weight sensitivity is not offered together with a terminal cost.

        ``dist`` (optional) is ``set_input_disturbance(dist)`` before the step: the disturbance then stays in force for later
        steps.  While one is in force the step's QP, ``cost`` and ``residuals`` are those of the model ``x+ = Ad x + Bd (u + d)``,
        ``x_pred`` is that model's prediction, and ``shift`` propagates the tail with it; ``sens=True`` and ``sens_w=True`` then
        raise ``ValueError``.  The step costs what a step with a new reference costs (``profiles/controller_step_rate_dist.txt``).

        ``surface`` (optional) is ``set_surface(surface)`` before the step: the window then stays in force for later steps.  While
        one is in force stage ``k`` works on the quadric of its row ``k``; ``cost`` and ``residuals`` are those of that problem;
        ``sens=True``, ``sens_w=True`` and ``dist`` then raise ``ValueError``."""
        import torch

        if self._combined:
            return self._step_combined(xhat, predict, yref, shift, sens, sens_w, dist, surface)
        if surface is not None:
            if dist is not None:
                raise ValueError("a surface window is not offered together with an input disturbance (dist)")
            self._check_surface(surface)
        if (sens or sens_w) and (self._surf_on or surface is not None):
            raise ValueError("step(sens=True) / step(sens_w=True) are not offered while a surface window is in force "
                             "(set_surface(None) switches it off)")
        if dist is not None and self._surf_on:
            raise ValueError("an input disturbance is not offered while a surface window is in force (set_surface(None) switches it off)")
        if dist is not None:
            self._check_disturbance(dist)
        if (sens or sens_w) and (self._dist_on or dist is not None):
            raise ValueError("step(sens=True) / step(sens_w=True) are not offered while an input disturbance is in force "
                             "(set_input_disturbance(None) switches it off)")
        if sens_w and self._term_on:
            raise ValueError("step(sens_w=True) is not offered while a terminal cost is in force (set_terminal_cost(None) switches it off)")
        sens = sens or sens_w
        if sens and self.configs[0]["solver_type"] != packing.SOLVER_RTI:
            raise ValueError("step(sens=True) needs an SQP_RTI controller: the sensitivities of u0 are those of one RTI step's QP")
        if yref is not None:
            self._check_reference(yref)
        shift_all = isinstance(shift, (bool, np.bool_))
        if not shift_all:
            self._check_mask(shift, "shift")
        x = self._xhat(xhat)
        io = dict(self._buffers(predict), xhat=x)
        if yref is not None:
            self.set_reference(yref)
        if dist is not None:
            self.set_input_disturbance(dist)
        if surface is not None:
            self.set_surface(surface)
        stream = torch.cuda.current_stream(self.device)
        warm = None
        if self._reset_mask is not None or not shift_all or bool(shift):
            warm = self._compose_warm(shift, shift_all, stream)
        if self._ref_on and self._ref_stream is not None and self._ref_stream != stream:
            stream.wait_stream(self._ref_stream)      # the copy of the reference lands before the step reads it
        if self._weights_stream is not None and self._weights_stream != stream:
            stream.wait_stream(self._weights_stream)  # the new weights are in the records before the step reads them
        if self._term_on and self._term_stream is not None and self._term_stream != stream:
            stream.wait_stream(self._term_stream)     # the copy of the terminal cost lands before the step reads it
        if self._dist_on and self._dist_stream is not None and self._dist_stream != stream:
            stream.wait_stream(self._dist_stream)     # the copy of the disturbance lands before the step reads it
        if self._surf_on and self._surf_stream is not None and self._surf_stream != stream:
            stream.wait_stream(self._surf_stream)     # the copy of the surface window lands before the step reads it
        # (a terminal cost, a disturbance or a surface window that was switched off leaves a stale linearisation behind, exactly as a
        # changed reference does)
        ref_changed = self._ref_changed or (self._term_changed and not self._term_on) or (self._dist_changed and not self._dist_on) \
            or (self._surf_changed and not self._surf_on)
        term = dict(term=self._term, term_changed=self._term_changed) if self._term_on else {}
        if sens:
            if self._sens is None:
                dev = torch.device("cuda", self.device)
                self._sens = dict(du0_dx=torch.zeros((self.batch, 6, 12), dtype=torch.float64, device=dev),
                                  du0_dyref=torch.zeros((self.batch, self.N, NREF, 6), dtype=torch.float64, device=dev),
                                  sens_valid=torch.zeros((self.batch,), dtype=torch.int32, device=dev))
            if self._step_stream is not None and self._step_stream != stream:
                stream.wait_stream(self._step_stream)     # a step still writing the buffers on another stream finishes first
            if sens_w and self._sensw is None:
                self._sensw = torch.zeros((self.batch, NWEIGHT, 6), dtype=torch.float64, device=torch.device("cuda", self.device))
            if self._term_on and self._sensxe is None:
                self._sensxe = torch.zeros((self.batch, 6, 12), dtype=torch.float64, device=torch.device("cuda", self.device))
            self.engine.step_sens(io, self._yref if self._ref_on else None, ref_changed=ref_changed, warm=warm,
                                  reset=self._reset, stream=stream.cuda_stream,
                                  sens=dict(du0_dx=self._sens["du0_dx"], du0_dyref=self._sens["du0_dyref"], valid=self._sens["sens_valid"]),
                                  **(dict(du0_dw=self._sensw) if sens_w else {}),
                                  **(dict(term, du0_dxe=self._sensxe) if self._term_on else {}))
        elif self._term_on:
            self.engine.step_sens(io, self._yref if self._ref_on else None, ref_changed=ref_changed, warm=warm, reset=self._reset,
                                  stream=stream.cuda_stream, **term)
        elif self._dist_on:
            self.engine.step_dist(io, self._yref if self._ref_on else None, ref_changed=ref_changed, warm=warm, reset=self._reset,
                                  dist=self._dist, dist_changed=self._dist_changed, stream=stream.cuda_stream)
        elif self._surf_on:
            self.engine.step_surf(io, self._yref if self._ref_on else None, ref_changed=ref_changed, warm=warm, reset=self._reset,
                                  surf=self._surf, surf_changed=self._surf_changed, stream=stream.cuda_stream)
        elif warm is not None:
            self.engine.step_warm(io, self._yref if self._ref_on else None, ref_changed=ref_changed, warm=warm,
                                  reset=self._reset, stream=stream.cuda_stream)
        elif self._ref_on or ref_changed:
            self.engine.step_ref(io, self._yref if self._ref_on else None, ref_changed=ref_changed, reset=self._reset,
                                 stream=stream.cuda_stream)
        else:
            self.engine.step(io, reset=self._reset, stream=stream.cuda_stream)
        self._step_stream = stream
        self._reset = False
        self._ref_changed = False
        self._term_changed = False
        self._dist_changed = False
        self._surf_changed = False
        self._reset_mask = None
        out = {k: v for k, v in io.items() if k != "xhat"}
        if sens:
            out.update(self._sens)
            if self._term_on:
                out["du0_dxe"] = self._sensxe
        if sens_w:
            out["du0_dw"] = self._sensw
        return out

    def _step_combined(self, xhat, predict, yref, shift, sens, sens_w, dist, surface) -> Dict:
        """step() of a controller built with combined=True: whatever of the terminal cost, the input disturbance and the surface
        window is in force goes into ONE launch of the combined step, with ``shift`` as its warm-start modes; what is switched off is
        handed over as None and the library fills its neutral table.  With ``shift`` the tail is propagated with this step's
        disturbance."""
        import torch

        if sens or sens_w:
            raise ValueError("step(sens=True) / step(sens_w=True) are not offered on a combined controller (BatchController(..., "
                             "combined=True)): the combined step forms no sensitivities")
        if surface is not None:
            self._check_surface(surface)
        if dist is not None:
            self._check_disturbance(dist)
        if yref is not None:
            self._check_reference(yref)
        shift_all = isinstance(shift, (bool, np.bool_))
        if not shift_all:
            self._check_mask(shift, "shift")
        x = self._xhat(xhat)
        io = dict(self._buffers(predict), xhat=x)
        if yref is not None:
            self.set_reference(yref)
        if dist is not None:
            self.set_input_disturbance(dist)
        if surface is not None:
            self.set_surface(surface)
        stream = torch.cuda.current_stream(self.device)
        warm = None
        if self._reset_mask is not None or not shift_all or bool(shift):
            warm = self._compose_warm(shift, shift_all, stream)
        for on, src in ((self._ref_on, self._ref_stream), (True, self._weights_stream), (self._term_on, self._term_stream),
                        (self._dist_on, self._dist_stream), (self._surf_on, self._surf_stream)):
            if on and src is not None and src != stream:
                stream.wait_stream(src)                   # the copies land before the step reads them
        # (whatever changed, or was switched off, leaves a stale linearisation behind exactly as a changed reference does)
        self.engine.step_combined(io, self._yref if self._ref_on else None, ref_changed=self._ref_changed, warm=warm, reset=self._reset,
                                  term=self._term if self._term_on else None, term_changed=self._term_changed,
                                  dist=self._dist if self._dist_on else None, dist_changed=self._dist_changed,
                                  surf=self._surf if self._surf_on else None, surf_changed=self._surf_changed,
                                  stream=stream.cuda_stream)
        self._step_stream = stream
        self._reset = False
        self._ref_changed = self._term_changed = self._dist_changed = self._surf_changed = False
        self._reset_mask = None
        return {k: v for k, v in io.items() if k != "xhat"}

    def _compose_warm(self, shift, shift_all, stream):
        """The int32 [B] modes of the next step in the controller's own buffer, written on the step's stream: reset where
        ``reset(mask)`` marked, shift where asked among the others, carry elsewhere."""
        import torch

        dev = torch.device("cuda", self.device)
        if self._warm is None:
            self._warm = torch.empty((self.batch,), dtype=torch.int32, device=dev)
        if self._step_stream is not None and self._step_stream != stream:
            stream.wait_stream(self._step_stream)         # a step still reading the buffer on another stream finishes first
        on_dev = lambda m: torch.from_numpy(np.ascontiguousarray(m)).to(dev) if isinstance(m, np.ndarray) else m
        if shift_all:
            self._warm.fill_(WARM_SHIFT if shift else 0)
        else:
            self._warm.copy_(on_dev(shift).to(torch.int32) * WARM_SHIFT)
        if self._reset_mask is not None:
            self._warm.masked_fill_(on_dev(self._reset_mask), WARM_RESET)
        return self._warm

    def reset(self, mask=None):
        """The next step starts from the initial guess (x_k = [q_0; qdot_0], u_k = 0, multipliers 0) again.  The task
        reference in force stays.

        ``mask`` (a [B] bool numpy array, or tensor on the controller's device) restarts the marked simulations only; the others
        keep their warm start.  Masks given before the next step accumulate."""
        if mask is None:
            self._reset = True
            return
        import torch

        mask = self._check_mask(mask, "mask")
        if self._reset_mask is None:
            self._reset_mask = mask.copy() if isinstance(mask, np.ndarray) else mask.clone()
        elif isinstance(self._reset_mask, np.ndarray) and isinstance(mask, np.ndarray):
            self._reset_mask |= mask
        else:
            dev = torch.device("cuda", self.device)
            as_t = lambda m: torch.from_numpy(m).to(dev) if isinstance(m, np.ndarray) else m
            self._reset_mask = as_t(self._reset_mask) | as_t(mask)

    def launch_info(self) -> Dict[str, int]:
        """Geometry of the step kernel: kernel family (0 latency, 1 throughput engine), wavefronts per simulation, LDS pool."""
        return self.engine.launch_info()

    def close(self):
        self.engine.close()
