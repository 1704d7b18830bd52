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
"""
from __future__ import annotations

from typing import Dict, Mapping, Optional, Sequence

import numpy as np

from . import config as cfgmod, packing
from .engine import CONTROLLER_ENGINES, STEP_FIELDS, MpcBatchEngine


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

    def __init__(self, configs: Sequence[Mapping], device: int = 0, engine: str = "latency"):
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

        chain = chain_for(cfgs[0])
        self.configs = cfgs
        self.horizons = horizons
        self.batch, self.N = len(cfgs), int(horizons.max())
        self.engine = MpcBatchEngine(device)
        self.device = self.engine.device
        self.engine.setup_controller(cfgs, chain, engine=engine)
        self._bufs: Optional[Dict] = None
        self._reset = True

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

    def step(self, xhat, predict: bool = False) -> Dict:
        """One MPC step of every controller from the feedback states ``xhat`` ([B, 12] q; qdot, float64: a tensor on the
        controller's device, or a numpy array that is copied there).

        Returns device tensors: ``u0`` [B, 6] (the input to apply), ``status``, ``sqp_iter``, ``qp_iter`` [B] (int32),
        ``residuals`` [B, 4], ``cost``, ``solver_time`` [B]; with ``predict`` also the iterate's predicted trajectory
        ``x_pred`` [B, N+1, 12] and ``u_pred`` [B, N, 6] (N the longest horizon; rows past ``horizons[i]`` are NaN).  The launch is asynchronous on the current torch stream and nothing
        is synchronised.  The returned tensors are the controller's own buffers: the next ``step`` overwrites them, so clone
        what must outlive it."""
        import torch

        x = self._xhat(xhat)
        io = dict(self._buffers(predict), xhat=x)
        stream = torch.cuda.current_stream(self.device)
        self.engine.step(io, reset=self._reset, stream=stream.cuda_stream)
        self._reset = False
        return {k: v for k, v in io.items() if k != "xhat"}

    def reset(self):
        """The next step starts from the initial guess (x_k = [q_0; qdot_0], u_k = 0, multipliers 0) again."""
        self._reset = True

    def launch_info(self) -> Dict[str, int]:
        """Geometry of the step kernel: kernel family (0 latency, 1 throughput engine), wavefronts per simulation, LDS pool."""
        return self.engine.launch_info()

    def close(self):
        self.engine.close()
