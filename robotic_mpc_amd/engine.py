"""ctypes binding of libmpcbatch.so (include/mpcbatch.h) -- the only compute path.

This is the layer that stands where ``acados_template.AcadosOcpSolver`` stands in the
reference (trajectory_optimizer.py:183-186; call sites simulator.py:210-221): a thin
ctypes wrapper around a native solver library.  PyTorch is used as plumbing only: it owns
the device result buffers and the HIP stream, so results can be gathered across GPUs with
``torch.distributed`` (RCCL) without a host round trip.

There is no CPU fallback: if the library or a GPU is missing, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import packing

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmpcbatch.so")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

RESULT_FIELDS = (
    # name, ctype, per-simulation shape as a function of (Nsim, T1)
    ("z", "f8", lambda S, T: (12, T)), ("u", "f8", lambda S, T: (6, T)), ("ee_pose", "f8", lambda S, T: (12, T)),
    ("ee_rpy", "f8", lambda S, T: (3, T)), ("ee_vel", "f8", lambda S, T: (6, T)),
    ("status", "i4", lambda S, T: (S,)), ("sqp_iter", "i4", lambda S, T: (S,)), ("qp_iter", "i4", lambda S, T: (S,)),
    ("residuals", "f8", lambda S, T: (S, 4)), ("cost", "f8", lambda S, T: (S,)), ("solver_time", "f8", lambda S, T: (S,)),
    ("errors", "f8", lambda S, T: (7, T)), ("plant_time", "f8", lambda S, T: (S,)),
)
ERROR_ROWS = ("e1", "e2", "e3", "e4", "e5", "p_task_z", "p_ee_y")   # rows of `errors` (simulator.py:337-344)
NSUMMARY = 24
# columns of the mpcb_summary record (include/mpcbatch.h)
SUMMARY_COLS = ("rmse_e1", "rmse_e2", "rmse_e3", "rmse_e4", "rmse_e5", "itse_e1", "itse_e2", "itse_e3", "itse_e4", "itse_e5",
                "weighted_rmse", "total_sqp_iterations", "avg_sqp_iterations", "num_failures", "max_kkt_residual",
                "total_solver_time", "avg_mpc_time", "avg_solver_time", "avg_integration_time", "total_computation_time",
                "total_qp_iterations")


class MpcbProblem(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("batch", "N", "Nsim", "solver_type", "max_iter", "qp_iter_max", "fixed_step",
                                       "precision")]


class MpcbResult(C.Structure):
    _fields_ = [("z", _dp), ("u", _dp), ("ee_pose", _dp), ("ee_rpy", _dp), ("ee_vel", _dp), ("status", _ip),
                ("sqp_iter", _ip), ("qp_iter", _ip), ("residuals", _dp), ("cost", _dp), ("solver_time", _dp),
                ("errors", _dp), ("plant_time", _dp)]


class MpcbStepIO(C.Structure):
    """mpcb_step_io: DEVICE pointers, batch-major; x_pred / u_pred may be NULL."""
    _fields_ = [("xhat", _dp), ("u0", _dp), ("status", _ip), ("sqp_iter", _ip), ("qp_iter", _ip), ("residuals", _dp),
                ("cost", _dp), ("solver_time", _dp), ("x_pred", _dp), ("u_pred", _dp)]


# name, ctype, per-simulation shape as a function of N (mpcb_step_io; x_pred / u_pred are optional)
STEP_FIELDS = (
    ("xhat", "f8", lambda N: (12,)), ("u0", "f8", lambda N: (6,)), ("status", "i4", lambda N: ()), ("sqp_iter", "i4", lambda N: ()),
    ("qp_iter", "i4", lambda N: ()), ("residuals", "f8", lambda N: (4,)), ("cost", "f8", lambda N: ()),
    ("solver_time", "f8", lambda N: ()), ("x_pred", "f8", lambda N: (N + 1, 12)), ("u_pred", "f8", lambda N: (N, 6)),
)


# BatchController / setup_controller engine names -> the MPCB_ENGINE_* values of include/mpcbatch.h
CONTROLLER_ENGINES = {"auto": -1, "latency": 0, "stream": 1}


# warm-start modes of step_warm (MPCB_WARM_*, include/mpcbatch.h)
WARM_CARRY, WARM_RESET, WARM_SHIFT = 0, 1, 2


def warm_modes(cfgs: Sequence[Dict]) -> Optional[np.ndarray]:
    """The warm-start modes of a bucket as mpcb_rollout_warm takes them, int32 [batch] of WARM_CARRY / WARM_SHIFT (config key
    warm_start), or None when every simulation carries."""
    modes = np.array([WARM_SHIFT if c.get("warm_start", "carry") == "shift" else WARM_CARRY for c in cfgs], dtype=np.int32)
    return modes if (modes == WARM_SHIFT).any() else None


def combined_arrays(cfgs: Sequence[Dict]) -> Dict:
    """The tables of a combined bucket as numpy arrays: "yref" [B, Nsim + N, 5], "pert" {"wcv" [B, 6], "u_dist" [B, Nsim, 6],
    "x_noise" [B, Nsim, 12]}, "term" {"blocks" [B, 18], "x_ref" [B, Nsim, 12]}, "gain" [B, 12], "surf" [B, Nsim + N, 6], "warm" [B]
    int32 (N the longest horizon).  A simulation that does not use a feature gets the neutral rows of include/mpcbatch.h: the packed
    reference row, the model's bandwidths and zero disturbance / noise, zero terminal blocks (and zero x_ref rows), zero observer
    gains, its own packed a..f on every row, WARM_CARRY."""
    from . import observer, plant, reference, surface, terminal

    B, Nsim = len(cfgs), int(cfgs[0]["Nsim"])
    rows = Nsim + max(int(c["N"]) for c in cfgs)

    def padded(y):
        out = np.empty((rows, y.shape[1]))
        out[:y.shape[0]], out[y.shape[0]:] = y, y[-1]
        return out

    a = {"yref": np.empty((B, rows, 5)), "pert": {"wcv": np.empty((B, 6)), "u_dist": np.zeros((B, Nsim, 6)), "x_noise": np.zeros((B, Nsim, 12))},
         "term": {"blocks": np.zeros((B, 18)), "x_ref": np.zeros((B, Nsim, 12))}, "gain": np.zeros((B, 12)),
         "surf": np.empty((B, rows, 6)), "warm": np.zeros(B, dtype=np.int32)}
    for i, c in enumerate(cfgs):
        a["yref"][i] = padded(reference.sample(c)) if c.get("reference_schedule") is not None else reference.packed_rows(c, rows)
        a["surf"][i] = padded(surface.sample(c)) if c.get("surface_schedule") is not None else surface.packed_rows(c, rows)
        if c.get("plant_perturbation") is not None:
            p = plant.sample(c)
            for k in ("wcv", "u_dist", "x_noise"):
                a["pert"][k][i] = p[k]
        else:
            a["pert"]["wcv"][i] = np.asarray(c["wcv"], dtype=np.float64)
        if c.get("terminal_cost") is not None:
            t = terminal.sample(c)
            a["term"]["blocks"][i], a["term"]["x_ref"][i] = t["blocks"].T.reshape(18), t["x_ref"]
        if c.get("disturbance_observer") is not None:
            a["gain"][i] = observer.stack([c])[0]
        if c.get("warm_start", "carry") == "shift":
            a["warm"][i] = WARM_SHIFT
    return a


class EngineError(RuntimeError):
    pass


class MpcbPlantPert(C.Structure):
    """mpcb_plant_pert (include/mpcbatch.h): device pointers, each may be NULL."""
    _fields_ = [("wcv", C.POINTER(C.c_double)), ("u_dist", C.POINTER(C.c_double)), ("x_noise", C.POINTER(C.c_double))]


class MpcbStepSensOut(C.Structure):
    """mpcb_step_sens_out (include/mpcbatch.h): device pointers."""
    _fields_ = [("du0_dx", C.POINTER(C.c_double)), ("du0_dyref", C.POINTER(C.c_double)), ("valid", C.POINTER(C.c_int))]


class MpcbTermTable(C.Structure):
    """mpcb_term_table (include/mpcbatch.h): device pointers."""
    _fields_ = [("blocks", C.POINTER(C.c_double)), ("x_ref", C.POINTER(C.c_double))]


class MpcbObserver(C.Structure):
    """mpcb_observer (include/mpcbatch.h): device pointers."""
    _fields_ = [("gain", C.POINTER(C.c_double)), ("d_hat", C.POINTER(C.c_double))]


_EXPORTS = ("mpcb_version", "mpcb_device_count", "mpcb_create", "mpcb_destroy", "mpcb_last_error",
            "mpcb_workspace_bytes", "mpcb_result_bytes_per_sim", "mpcb_setup", "mpcb_rollout", "mpcb_sync",
            "mpcb_last_kernel_ms", "mpcb_kernel_info", "mpcb_launch_info", "mpcb_engine", "mpcb_engine_for", "mpcb_summary",
            "mpcb_run", "mpcb_setup_controller", "mpcb_step", "mpcb_setup_controller_on", "mpcb_controller_engine_for",
            "mpcb_step_ref", "mpcb_step_warm", "mpcb_step_sens", "mpcb_set_weights", "mpcb_step_sens_w", "mpcb_step_term",
            "mpcb_step_dist",
            "mpcb_rollout_ref", "mpcb_queue_used", "mpcb_rollout_pert", "mpcb_rollout_term", "mpcb_rollout_obs",
            "mpcb_step_surf", "mpcb_rollout_surf", "mpcb_rollout_warm", "mpcb_step_combined", "mpcb_rollout_combined")


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen libmpcbatch.so and declare the signatures of include/mpcbatch.h."""
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise EngineError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          f"(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # torch bundles its own libamdhip64.so.7; import it first so that libmpcbatch.so binds to the
    # SAME HIP runtime instance (two runtimes in one process cannot share the device).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name in _EXPORTS:
        if not hasattr(lib, name):
            raise EngineError(f"{path} does not export {name}")
    lib.mpcb_version.restype = C.c_int
    lib.mpcb_device_count.restype = C.c_int
    lib.mpcb_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    lib.mpcb_destroy.argtypes = [C.c_void_p]
    lib.mpcb_destroy.restype = None
    lib.mpcb_last_error.argtypes = [C.c_void_p]
    lib.mpcb_last_error.restype = C.c_char_p
    lib.mpcb_engine_for.argtypes = [C.POINTER(MpcbProblem)]
    lib.mpcb_engine_for.restype = C.c_int
    lib.mpcb_workspace_bytes.argtypes = [C.POINTER(MpcbProblem)]
    lib.mpcb_workspace_bytes.restype = C.c_size_t
    lib.mpcb_result_bytes_per_sim.argtypes = [C.POINTER(MpcbProblem)]
    lib.mpcb_result_bytes_per_sim.restype = C.c_size_t
    lib.mpcb_setup.argtypes = [C.c_void_p, C.POINTER(MpcbProblem), _dp, _dp]
    lib.mpcb_rollout.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(MpcbResult), C.c_void_p]
    lib.mpcb_rollout_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(MpcbResult), _dp, C.c_void_p]
    lib.mpcb_rollout_pert.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(MpcbResult), _dp, C.POINTER(MpcbPlantPert), C.c_void_p]
    lib.mpcb_rollout_term.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(MpcbResult), _dp, C.POINTER(MpcbPlantPert), _dp, _dp,
                                      C.c_void_p]
    lib.mpcb_rollout_obs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(MpcbResult), _dp, C.POINTER(MpcbPlantPert), _dp, _dp,
                                     C.c_void_p]
    lib.mpcb_queue_used.argtypes = [C.c_void_p]
    lib.mpcb_sync.argtypes = [C.c_void_p]
    lib.mpcb_last_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    lib.mpcb_kernel_info.argtypes = [C.c_void_p] + [_ip] * 4
    lib.mpcb_run.argtypes = [C.c_void_p, C.POINTER(MpcbProblem), _dp, _dp, C.POINTER(MpcbResult)]
    lib.mpcb_summary.argtypes = [C.c_void_p, C.POINTER(MpcbResult), _dp, C.c_void_p]
    lib.mpcb_launch_info.argtypes = [C.c_void_p, _ip, _ip]
    lib.mpcb_engine.argtypes = [C.c_void_p]
    lib.mpcb_setup_controller.argtypes = [C.c_void_p, C.POINTER(MpcbProblem), _dp, _dp]
    lib.mpcb_step.argtypes = [C.c_void_p, C.POINTER(MpcbStepIO), C.c_int, C.c_void_p]
    lib.mpcb_setup_controller_on.argtypes = [C.c_void_p, C.POINTER(MpcbProblem), _dp, _dp, C.c_int]
    lib.mpcb_controller_engine_for.argtypes = [C.POINTER(MpcbProblem), C.c_int]
    lib.mpcb_step_ref.argtypes = [C.c_void_p, C.POINTER(MpcbStepIO), _dp, C.c_int, C.c_int, C.c_void_p]
    lib.mpcb_step_warm.argtypes = [C.c_void_p, C.POINTER(MpcbStepIO), _dp, C.c_int, _ip, C.c_int, C.c_void_p]
    lib.mpcb_step_sens.argtypes = [C.c_void_p, C.POINTER(MpcbStepIO), _dp, C.c_int, _ip, C.c_int, C.POINTER(MpcbStepSensOut), C.c_void_p]
    lib.mpcb_set_weights.argtypes = [C.c_void_p, _dp, C.c_void_p]
    lib.mpcb_step_sens_w.argtypes = [C.c_void_p, C.POINTER(MpcbStepIO), _dp, C.c_int, _ip, C.c_int, C.POINTER(MpcbStepSensOut), _dp,
                                     C.c_void_p]
    lib.mpcb_step_term.argtypes = [C.c_void_p, C.POINTER(MpcbStepIO), _dp, C.c_int, _ip, C.c_int, C.POINTER(MpcbStepSensOut), _dp, C.c_int,
                                   _dp, C.c_void_p]
    lib.mpcb_step_dist.argtypes = [C.c_void_p, C.POINTER(MpcbStepIO), _dp, C.c_int, _ip, C.c_int, _dp, C.c_int, C.c_void_p]
    lib.mpcb_step_surf.argtypes = [C.c_void_p, C.POINTER(MpcbStepIO), _dp, C.c_int, _ip, C.c_int, _dp, C.c_int, C.c_void_p]
    lib.mpcb_rollout_surf.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(MpcbResult), _dp, C.POINTER(MpcbPlantPert), _dp, C.c_void_p]
    lib.mpcb_rollout_warm.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(MpcbResult), _dp, C.POINTER(MpcbPlantPert), _dp, _ip,
                                      C.c_void_p]
    lib.mpcb_step_combined.argtypes = [C.c_void_p, C.POINTER(MpcbStepIO), _dp, C.c_int, _ip, C.c_int, _dp, C.c_int, _dp, C.c_int, _dp,
                                       C.c_int, C.c_void_p]
    lib.mpcb_rollout_combined.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(MpcbResult), _dp, C.POINTER(MpcbPlantPert),
                                          C.POINTER(MpcbTermTable), C.POINTER(MpcbObserver), _dp, _ip, C.c_void_p]
    lib.mpcb_controller_engine_for.restype = C.c_int
    if hasattr(lib, "mpcb_debug_task_lin"):
        lib.mpcb_debug_task_lin.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]
    return lib


def make_problem(cfgs: Sequence[Dict]) -> MpcbProblem:
    c0 = cfgs[0]
    ragged = any(c["N"] != c0["N"] for c in cfgs)
    if ragged and c0["solver_type"] != packing.SOLVER_RTI:
        raise ValueError("simulations of different horizons share a launch only with nlp_solver_type='SQP_RTI'")
    key0 = packing.bucket_key(c0, ragged)
    for c in cfgs[1:]:
        if packing.bucket_key(c, ragged) != key0:
            raise ValueError("all simulations of one launch must share Nsim, solver options and robot (and N, except SQP_RTI)")
    return MpcbProblem(len(cfgs), max(c["N"] for c in cfgs), c0["Nsim"], c0["solver_type"], c0["max_iter"], c0["qp_iter_max"],
                       int(c0["fixed_step"]), int(c0.get("precision", 0)))


def engine_for(batch: int, N: int, Nsim: int, solver: str = "SQP_RTI", precision: int = 0, lib: Optional[C.CDLL] = None) -> int:
    """Kernel family a uniform bucket of this shape is sent to (mpcb_engine_for; host logic, no GPU needed):
    0 latency engine, 1 throughput engine."""
    lib = lib or load_library()
    pb = MpcbProblem(batch, N, Nsim, 0 if solver == "SQP" else 1, 100, 50, 0, precision)
    return int(lib.mpcb_engine_for(C.byref(pb)))


def controller_engine_for(batch: int, N: int, solver: str = "SQP_RTI", ragged: bool = False, lib: Optional[C.CDLL] = None) -> int:
    """Kernel family ``BatchController(..., engine="auto")`` runs a batch of this shape on (mpcb_controller_engine_for; host logic,
    no GPU needed): 0 latency engine, 1 throughput engine."""
    lib = lib or load_library()
    pb = MpcbProblem(batch, N, 1, 0 if solver == "SQP" else 1, 100, 50, 0, 0)
    return int(lib.mpcb_controller_engine_for(C.byref(pb), int(bool(ragged))))


class MpcBatchEngine:
    """One handle on one GPU.  ``run`` = Simulator.__init__ + Simulator.run for a whole bucket."""

    def __init__(self, device: int = 0, lib_path: Optional[str] = None):
        self.lib = load_library(lib_path)
        self.device = int(device)
        n = self.lib.mpcb_device_count()
        if n <= 0:
            raise EngineError("no HIP device visible: the MPC engine runs on MI355X only (no CPU fallback)")
        h = C.c_void_p()
        rc = self.lib.mpcb_create(C.byref(h), self.device)
        if rc != 0:
            raise EngineError(f"mpcb_create(device={device}) failed with {rc} ({n} device(s) visible)")
        self._h = h
        self.last_kernel_ms: List[float] = []

    def close(self):
        if getattr(self, "_h", None):
            self.lib.mpcb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            msg = self.lib.mpcb_last_error(self._h)
            raise EngineError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def kernel_info(self) -> Dict[str, int]:
        v = [C.c_int(0) for _ in range(4)]
        self._check(self.lib.mpcb_kernel_info(self._h, *[C.byref(x) for x in v]), "mpcb_kernel_info")
        return dict(vgprs=v[0].value, sgprs=v[1].value, lds_bytes=v[2].value, scratch_bytes=v[3].value)

    def launch_info(self) -> Dict[str, int]:
        """Launch geometry chosen by setup(): kernel family (0 latency, 1 throughput engine), wavefronts per
        simulation, LDS chunk pool bytes."""
        w, pbytes = C.c_int(0), C.c_int(0)
        self._check(self.lib.mpcb_launch_info(self._h, C.byref(w), C.byref(pbytes)), "mpcb_launch_info")
        return dict(waves_per_sim=w.value, pool_bytes=pbytes.value, engine=int(self.lib.mpcb_engine(self._h)))

    # ------------------------------------------------------------------ device-resident path
    @staticmethod
    def prepare(cfgs: Sequence[Dict], chain):
        """Resolved configs -> what mpcb_setup takes: (problem, parameter records [batch, NPARAM], robot constants [105]).
        This is the construction-time half of Simulator.__init__ (dict -> numbers); nothing touches the device."""
        pb = make_problem(cfgs)
        params = packing.pack_batch(cfgs)
        robot = np.ascontiguousarray(chain.packed(cfgs[0]["t_ee"]), dtype=np.float64)
        assert params.shape == (len(cfgs), packing.NPARAM) and robot.shape == (105,)
        return pb, params, robot

    def setup_packed(self, pb: MpcbProblem, params: np.ndarray, robot: np.ndarray) -> MpcbProblem:
        """mpcb_setup: validate, derive the model constants, upload the records (H2D), size the workspace."""
        self._check(self.lib.mpcb_setup(self._h, C.byref(pb), params.ctypes.data_as(_dp), robot.ctypes.data_as(_dp)),
                    "mpcb_setup")
        self._pb = pb
        return pb

    def setup(self, cfgs: Sequence[Dict], chain) -> MpcbProblem:
        return self.setup_packed(*self.prepare(cfgs, chain))

    def alloc_results(self, pb: MpcbProblem):
        """Device result buffers as torch tensors (dict name -> tensor [batch, ...])."""
        import torch

        dev = torch.device("cuda", self.device)
        S, T = pb.Nsim, pb.Nsim + 1
        out = {}
        for name, ty, shp in RESULT_FIELDS:
            dt = torch.float64 if ty == "f8" else torch.int32
            out[name] = torch.zeros((pb.batch,) + shp(S, T), dtype=dt, device=dev)
        return out

    @staticmethod
    def _result_struct(bufs) -> MpcbResult:
        r = MpcbResult()
        for name, ty, _ in RESULT_FIELDS:
            ptr = bufs[name].data_ptr() if hasattr(bufs[name], "data_ptr") else bufs[name].ctypes.data
            setattr(r, name, C.cast(C.c_void_p(ptr), _dp if ty == "f8" else _ip))
        return r

    def rollout(self, bufs, step0: int, step1: int, yref=None, stream: Optional[int] = None, pert=None, term=None, obs=None,
                surf=None, warm=None, combined: bool = False):
        """Asynchronous launch of closed-loop steps [step0, step1) into device buffers.  `yref`: the task reference schedules of
        the batch, a contiguous float64 device tensor [batch, Nsim + N, 5] (N the longest horizon; schedule_tensor) -- the same one
        for every launch of a run -- or None for the packed references (mpcb_rollout).  `pert`: the plant perturbation of the
        batch (mpcb_rollout_pert; perturbation_tensors), a dict of contiguous float64 device tensors "wcv" [batch, 6], "u_dist"
        [batch, Nsim, 6], "x_noise" [batch, Nsim, 12], each may be missing or None -- the same ones for every launch of a run; it
        needs `yref` (schedule_tensor supplies the packed rows when the configurations carry no schedule).  `term`: the joint-wise
        terminal cost of the batch (mpcb_rollout_term; terminal_tensors), a dict of contiguous float64 device tensors "blocks"
        [batch, 18] (pqq 6 | pqv 6 | pvv 6) and "x_ref" [batch, Nsim, 12] (row t: the terminal reference of step t), both
        required -- the same ones for every launch of a run; it needs `yref` likewise, and takes `pert` or the nominal plant.
        `obs`: the on-device disturbance observer of the batch (mpcb_rollout_obs; observer_tensors), a dict of contiguous float64
        device tensors "gain" [batch, 12] (l1 6 | l2 6; read) and "d_hat" [batch, Nsim, 6] (written: row t = the estimate step t
        used) -- the same ones for every launch of a run; it needs `yref` likewise, takes `pert` or the nominal plant, and is not
        offered together with `term`.
        `surf`: the surface schedules of the batch (mpcb_rollout_surf; surface_tensor), a contiguous float64 device tensor
        [batch, Nsim + N, 6] (row r: a..f at time r dt) -- the same one for every launch of a run; it needs `yref` likewise, takes
        `pert` or the nominal plant, and is not offered together with `term` or `obs`.
        `warm`: the warm-start modes of the batch (mpcb_rollout_warm; warm_tensor), a contiguous int32 device tensor [batch] of
        WARM_CARRY / WARM_SHIFT, constant over the run -- the same one for every launch; a simulation whose mode is WARM_SHIFT moves
        its carried solver memory one stage towards stage 0 before every step but the run's first.  It needs `yref` likewise, takes
        `pert` or the nominal plant and `surf` or the packed surface, and is not offered together with `term` or `obs`.
        `combined`: route to mpcb_rollout_combined, the one rollout in which `term`, `obs`, `surf` and `warm` may all be given (any
        subset; each as described above, None = absent for the whole batch).  A simulation of the batch that does not use a feature
        brings neutral rows for it (combined_tensors).  It needs `yref`; SQP_RTI and fp64 only.  Without it every refusal above
        stands."""
        if combined:
            return self._rollout_pert(bufs, step0, step1, yref, pert, stream, term=term, obs=obs, surf=surf, warm=warm, combined=True)
        if warm is not None:
            if term is not None:
                raise ValueError("the shift warm start (warm) is not offered together with a terminal cost (term)")
            if obs is not None:
                raise ValueError("the shift warm start (warm) is not offered together with a disturbance observer (obs)")
            return self._rollout_pert(bufs, step0, step1, yref, pert, stream, surf=surf, warm=warm)
        if surf is not None:
            if term is not None:
                raise ValueError("a surface schedule (surf) is not offered together with a terminal cost (term)")
            if obs is not None:
                raise ValueError("a surface schedule (surf) is not offered together with a disturbance observer (obs)")
            return self._rollout_pert(bufs, step0, step1, yref, pert, stream, surf=surf)
        if obs is not None:
            if term is not None:
                raise ValueError("a disturbance observer (obs) is not offered together with a terminal cost (term)")
            return self._rollout_pert(bufs, step0, step1, yref, pert, stream, obs=obs)
        if term is not None:
            return self._rollout_pert(bufs, step0, step1, yref, pert, stream, term)
        if pert is not None:
            return self._rollout_pert(bufs, step0, step1, yref, pert, stream)
        if stream is None:
            import torch

            stream = torch.cuda.current_stream(self.device).cuda_stream
        r = self._result_struct(bufs)
        if yref is None:
            self._check(self.lib.mpcb_rollout(self._h, step0, step1, C.byref(r), C.c_void_p(stream)), "mpcb_rollout")
            return
        self._check_yref(yref)
        self._check(self.lib.mpcb_rollout_ref(self._h, step0, step1, C.byref(r), C.cast(C.c_void_p(yref.data_ptr()), _dp),
                                              C.c_void_p(stream)), "mpcb_rollout_ref")

    def _check_yref(self, yref):
        pb = self._pb
        if tuple(yref.shape) != (pb.batch, pb.Nsim + pb.N, 5) or not yref.is_contiguous() or str(yref.dtype) != "torch.float64":
            raise ValueError(f"yref must be a contiguous float64 tensor [{pb.batch}, {pb.Nsim + pb.N}, 5], got {tuple(yref.shape)} {yref.dtype}")

    def _rollout_pert(self, bufs, step0, step1, yref, pert, stream, term=None, obs=None, surf=None, warm=None, combined=False):
        """rollout(pert=, term=, obs=, surf=, warm=): every shape is checked before the library is called."""
        pb = self._pb
        tp = {}
        if combined:
            if yref is None:
                raise ValueError("a combined rollout needs yref: schedule_tensor(cfgs) supplies the packed rows when there is no schedule")
            pert = {} if pert is None else pert
        if warm is not None:
            if yref is None:
                raise ValueError("a rollout with the shift warm start needs yref: schedule_tensor(cfgs) supplies the packed rows when "
                                 "there is no schedule")
            if not hasattr(warm, "data_ptr") or tuple(warm.shape) != (pb.batch,) or not warm.is_contiguous() \
                    or str(warm.dtype) != "torch.int32" or not warm.is_cuda or warm.device.index != self.device:
                raise ValueError(f"warm must be a contiguous int32 tensor [{pb.batch}] on cuda:{self.device}, got "
                                 f"{tuple(getattr(warm, 'shape', ()))} {getattr(warm, 'dtype', type(warm).__name__)} "
                                 f"{getattr(warm, 'device', '')}".rstrip())
            pert = {} if pert is None else pert
        if surf is not None:
            if yref is None:
                raise ValueError("a rollout over a surface schedule needs yref: schedule_tensor(cfgs) supplies the packed rows when "
                                 "there is no schedule")
            shape = (pb.batch, pb.Nsim + pb.N, 6)
            if not hasattr(surf, "data_ptr") or tuple(surf.shape) != shape or not surf.is_contiguous() \
                    or str(surf.dtype) != "torch.float64" or not surf.is_cuda or surf.device.index != self.device:
                raise ValueError(f"surf must be a contiguous float64 tensor {list(shape)} on cuda:{self.device}, got "
                                 f"{tuple(getattr(surf, 'shape', ()))} {getattr(surf, 'dtype', type(surf).__name__)} "
                                 f"{getattr(surf, 'device', '')}".rstrip())
            pert = {} if pert is None else pert
        if obs is not None:
            oshapes = {"gain": (pb.batch, 12), "d_hat": (pb.batch, pb.Nsim, 6)}
            if not isinstance(obs, dict) or set(obs) != set(oshapes):
                raise ValueError(f"obs has the keys {tuple(oshapes)} (got {sorted(obs) if isinstance(obs, dict) else type(obs).__name__})")
            if yref is None:
                raise ValueError("a rollout with a disturbance observer needs yref: schedule_tensor(cfgs) supplies the packed rows when "
                                 "there is no schedule")
            for name, shape in oshapes.items():
                t = obs[name]
                if t is None or not hasattr(t, "data_ptr") or tuple(t.shape) != shape or not t.is_contiguous() \
                        or str(t.dtype) != "torch.float64" or not t.is_cuda or t.device.index != self.device:
                    raise ValueError(f"obs[{name!r}] must be a contiguous float64 tensor {list(shape)} on cuda:{self.device}, got "
                                     f"{tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t).__name__)} "
                                     f"{getattr(t, 'device', '')}".rstrip())
                tp[name] = C.cast(C.c_void_p(t.data_ptr()), _dp)
            pert = {} if pert is None else pert
        if term is not None:
            tshapes = {"blocks": (pb.batch, 18), "x_ref": (pb.batch, pb.Nsim, 12)}
            if not isinstance(term, dict) or set(term) != set(tshapes):
                raise ValueError(f"term has the keys {tuple(tshapes)} (got {sorted(term) if isinstance(term, dict) else type(term).__name__})")
            if yref is None:
                raise ValueError("a rollout with a terminal cost needs yref: schedule_tensor(cfgs) supplies the packed rows when there is "
                                 "no schedule")
            for name, shape in tshapes.items():
                t = term[name]
                if t is None or not hasattr(t, "data_ptr") or tuple(t.shape) != shape or not t.is_contiguous() \
                        or str(t.dtype) != "torch.float64" or not t.is_cuda or t.device.index != self.device:
                    raise ValueError(f"term[{name!r}] must be a contiguous float64 tensor {list(shape)} on cuda:{self.device}, got "
                                     f"{tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t).__name__)} "
                                     f"{getattr(t, 'device', '')}".rstrip())
                tp[name] = C.cast(C.c_void_p(t.data_ptr()), _dp)
            pert = {} if pert is None else pert
        shapes = {"wcv": (pb.batch, 6), "u_dist": (pb.batch, pb.Nsim, 6), "x_noise": (pb.batch, pb.Nsim, 12)}
        extra = set(pert) - set(shapes)
        if extra:
            raise ValueError(f"pert has the keys {tuple(shapes)} (got {sorted(pert)})")
        if yref is None:
            raise ValueError("a perturbed rollout needs yref: schedule_tensor(cfgs) supplies the packed rows when there is no schedule")
        self._check_yref(yref)
        p = MpcbPlantPert()
        for name, shape in shapes.items():
            t = pert.get(name)
            if t is None:
                continue
            if tuple(t.shape) != shape or not t.is_contiguous() or str(t.dtype) != "torch.float64" or not t.is_cuda:
                raise ValueError(f"pert[{name!r}] must be a contiguous float64 device tensor {list(shape)}, got {tuple(t.shape)} {t.dtype}")
            setattr(p, name, C.cast(C.c_void_p(t.data_ptr()), _dp))
        if stream is None:
            import torch

            stream = torch.cuda.current_stream(self.device).cuda_stream
        r = self._result_struct(bufs)
        if combined:
            tt = MpcbTermTable(tp["blocks"], tp["x_ref"]) if term is not None else None
            ob = MpcbObserver(tp["gain"], tp["d_hat"]) if obs is not None else None
            self._check(self.lib.mpcb_rollout_combined(
                self._h, step0, step1, C.byref(r), C.cast(C.c_void_p(yref.data_ptr()), _dp), C.byref(p),
                C.byref(tt) if tt is not None else None, C.byref(ob) if ob is not None else None,
                C.cast(C.c_void_p(surf.data_ptr()), _dp) if surf is not None else None,
                C.cast(C.c_void_p(warm.data_ptr()), _ip) if warm is not None else None, C.c_void_p(stream)), "mpcb_rollout_combined")
            return
        if warm is not None:
            sp = C.cast(C.c_void_p(surf.data_ptr()), _dp) if surf is not None else None
            self._check(self.lib.mpcb_rollout_warm(self._h, step0, step1, C.byref(r), C.cast(C.c_void_p(yref.data_ptr()), _dp), C.byref(p),
                                                   sp, C.cast(C.c_void_p(warm.data_ptr()), _ip), C.c_void_p(stream)), "mpcb_rollout_warm")
            return
        if surf is not None:
            self._check(self.lib.mpcb_rollout_surf(self._h, step0, step1, C.byref(r), C.cast(C.c_void_p(yref.data_ptr()), _dp), C.byref(p),
                                                   C.cast(C.c_void_p(surf.data_ptr()), _dp), C.c_void_p(stream)), "mpcb_rollout_surf")
            return
        if obs is not None:
            self._check(self.lib.mpcb_rollout_obs(self._h, step0, step1, C.byref(r), C.cast(C.c_void_p(yref.data_ptr()), _dp), C.byref(p),
                                                  tp["gain"], tp["d_hat"], C.c_void_p(stream)), "mpcb_rollout_obs")
            return
        if term is not None:
            self._check(self.lib.mpcb_rollout_term(self._h, step0, step1, C.byref(r), C.cast(C.c_void_p(yref.data_ptr()), _dp), C.byref(p),
                                                   tp["blocks"], tp["x_ref"], C.c_void_p(stream)), "mpcb_rollout_term")
            return
        self._check(self.lib.mpcb_rollout_pert(self._h, step0, step1, C.byref(r), C.cast(C.c_void_p(yref.data_ptr()), _dp), C.byref(p),
                                               C.c_void_p(stream)), "mpcb_rollout_pert")

    def terminal_tensors(self, cfgs: Sequence[Dict]):
        """The terminal costs of a bucket (terminal.stack) on this engine's device -- {"blocks", "x_ref"} -- or None when the
        configurations carry none (a bucket is all or nothing: packing.bucket_key)."""
        if not any(c.get("terminal_cost") is not None for c in cfgs):
            return None
        import torch

        from . import terminal

        dev = torch.device("cuda", self.device)
        blocks, x_ref = terminal.stack(cfgs)
        return {"blocks": torch.from_numpy(blocks).to(dev), "x_ref": torch.from_numpy(x_ref).to(dev)}

    def observer_tensors(self, cfgs: Sequence[Dict]):
        """The disturbance observers of a bucket on this engine's device -- {"gain": observer.stack(cfgs), "d_hat": zeros
        [batch, Nsim, 6], which the rollout fills} -- or None when the configurations carry none (a bucket is all or nothing:
        packing.bucket_key)."""
        if not any(c.get("disturbance_observer") is not None for c in cfgs):
            return None
        import torch

        from . import observer

        dev = torch.device("cuda", self.device)
        return {"gain": torch.from_numpy(observer.stack(cfgs)).to(dev),
                "d_hat": torch.zeros((len(cfgs), int(cfgs[0]["Nsim"]), 6), dtype=torch.float64, device=dev)}

    def surface_tensor(self, cfgs: Sequence[Dict]):
        """The surface schedules of a bucket (surface.stack) on this engine's device, [batch, Nsim + N, 6], or None when the
        configurations carry none (a bucket is all or nothing: packing.bucket_key)."""
        if not any(c.get("surface_schedule") is not None for c in cfgs):
            return None
        import torch

        from . import surface

        return torch.from_numpy(surface.stack(cfgs)).to(torch.device("cuda", self.device))

    def warm_tensor(self, cfgs: Sequence[Dict]):
        """The warm-start modes of a bucket (config key warm_start) on this engine's device, int32 [batch] of WARM_CARRY /
        WARM_SHIFT, or None when every simulation carries: that bucket takes the path it took without the key."""
        modes = warm_modes(cfgs)
        if modes is None:
            return None
        import torch

        return torch.from_numpy(modes).to(torch.device("cuda", self.device))

    def combined_tensors(self, cfgs: Sequence[Dict]):
        """What rollout(combined=True) takes for a bucket of configurations with combine_features, on this engine's device --
        {"yref", "pert", "term", "obs", "surf", "warm"}, every table present -- or None for any other bucket.  Each simulation
        brings its own rows for the features it uses and NEUTRAL rows for the others (combined_arrays), so one launch serves
        whatever subsets the bucket mixes; obs["d_hat"] [batch, Nsim, 6] is filled by the rollout (zeros where there is no observer)."""
        if not any(c.get("combine_features") for c in cfgs):
            return None
        import torch

        dev = torch.device("cuda", self.device)
        a = combined_arrays(cfgs)
        put = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)   # noqa: E731
        return {"yref": put(a["yref"]), "pert": {k: put(v) for k, v in a["pert"].items()},
                "term": {k: put(v) for k, v in a["term"].items()},
                "obs": {"gain": put(a["gain"]), "d_hat": torch.zeros((len(cfgs), int(cfgs[0]["Nsim"]), 6), dtype=torch.float64, device=dev)},
                "surf": put(a["surf"]), "warm": put(a["warm"])}

    def perturbation_tensors(self, cfgs: Sequence[Dict]):
        """The plant perturbations of a bucket (plant.stack) on this engine's device -- {"wcv", "u_dist", "x_noise"} -- or None when
        the configurations carry none (a bucket is all or nothing: packing.bucket_key)."""
        if not any(c.get("plant_perturbation") is not None for c in cfgs):
            return None
        import torch

        from . import plant

        dev = torch.device("cuda", self.device)
        return {k: torch.from_numpy(v).to(dev) for k, v in plant.stack(cfgs).items()}

    def queue_used(self) -> bool:
        """Whether the last rollout launch went through the throughput engine's work queue (mpcb_queue_used)."""
        rc = int(self.lib.mpcb_queue_used(self._h))
        if rc < 0:
            raise EngineError(f"mpcb_queue_used failed ({rc})")
        return rc == 1

    def schedule_tensor(self, cfgs: Sequence[Dict]):
        """The reference schedules of a bucket (reference.stack) on this engine's device, or None when the configurations carry
        none (a bucket is all or nothing: packing.bucket_key) -- unless they carry a plant perturbation, a terminal cost, a
        disturbance observer, a surface schedule or the shift warm start: those rollouts always track a schedule, the packed row [0, 1, 0, px_ref, vy_ref] on every row when there is no other."""
        from . import reference

        if not any(c.get("reference_schedule") is not None for c in cfgs):
            if not any(c.get("plant_perturbation") is not None or c.get("terminal_cost") is not None
                       or c.get("disturbance_observer") is not None or c.get("surface_schedule") is not None
                       or c.get("warm_start", "carry") == "shift" for c in cfgs):
                return None
            import torch

            rows = int(cfgs[0]["Nsim"]) + max(int(c["N"]) for c in cfgs)
            packed = np.stack([reference.packed_rows(c, rows) for c in cfgs])
            return torch.from_numpy(np.ascontiguousarray(packed)).to(torch.device("cuda", self.device))
        import torch

        return torch.from_numpy(reference.stack(cfgs)).to(torch.device("cuda", self.device))

    def sync(self):
        self._check(self.lib.mpcb_sync(self._h), "mpcb_sync")

    def summary(self, bufs, stream: Optional[int] = None):
        """Per-simulation summary record [batch, NSUMMARY] (device tensor) of a finished rollout --
        Simulator.metrics / solver_stats / timings / get_summary for the whole batch in one launch."""
        import torch

        if stream is None:
            stream = torch.cuda.current_stream(self.device).cuda_stream
        out = torch.empty((self._pb.batch, NSUMMARY), dtype=torch.float64, device=torch.device("cuda", self.device))
        r = self._result_struct(bufs)
        self._check(self.lib.mpcb_summary(self._h, C.byref(r), C.cast(C.c_void_p(out.data_ptr()), _dp), C.c_void_p(stream)),
                    "mpcb_summary")
        return out

    # ------------------------------------------------------------------ controller step
    def setup_controller(self, cfgs: Sequence[Dict], chain, engine: str = "latency") -> MpcbProblem:
        """mpcb_setup_controller_on: like setup(), for step(), fp64, on the kernel family `engine` ("latency": any batch size, one
        horizon; "stream": one wavefront per simulation, ragged SQP_RTI horizons too; "auto": mpcb_controller_engine_for decides)."""
        if engine not in CONTROLLER_ENGINES:
            raise ValueError(f"engine must be one of {sorted(CONTROLLER_ENGINES)}, got {engine!r}")
        pb, params, robot = self.prepare(cfgs, chain)
        self._check(self.lib.mpcb_setup_controller_on(self._h, C.byref(pb), params.ctypes.data_as(_dp), robot.ctypes.data_as(_dp),
                                                      CONTROLLER_ENGINES[engine]), "mpcb_setup_controller_on")
        self._pb = pb
        return pb

    @staticmethod
    def _step_struct(io) -> MpcbStepIO:
        r = MpcbStepIO()
        for name, ty, _ in STEP_FIELDS:
            t = io.get(name)
            if t is not None:
                setattr(r, name, C.cast(C.c_void_p(t.data_ptr()), _dp if ty == "f8" else _ip))
        return r

    def step(self, io, reset: bool = False, stream: Optional[int] = None):
        """mpcb_step: one MPC step of every simulation from the states io['xhat'] (device tensors named as the fields of
        mpcb_step_io; 'x_pred' / 'u_pred' optional).  Asynchronous on `stream` (default: the current torch stream)."""
        if stream is None:
            import torch

            stream = torch.cuda.current_stream(self.device).cuda_stream
        r = self._step_struct(io)
        self._check(self.lib.mpcb_step(self._h, C.byref(r), int(bool(reset)), C.c_void_p(stream)), "mpcb_step")

    def step_ref(self, io, yref=None, ref_changed: bool = False, reset: bool = False, stream: Optional[int] = None):
        """mpcb_step_ref: step() against the task reference `yref`, a contiguous float64 device tensor [batch, N, 5] (N the longest
        horizon) of the targets of g1..g5 per stage, or None for the packed references.  `ref_changed`: the reference differs from
        the previous step's (the step linearises again first)."""
        if stream is None:
            import torch

            stream = torch.cuda.current_stream(self.device).cuda_stream
        r = self._step_struct(io)
        yp = C.cast(C.c_void_p(yref.data_ptr()), _dp) if yref is not None else None
        self._check(self.lib.mpcb_step_ref(self._h, C.byref(r), yp, int(bool(ref_changed)), int(bool(reset)), C.c_void_p(stream)),
                    "mpcb_step_ref")

    def step_warm(self, io, yref=None, ref_changed: bool = False, warm=None, reset: bool = False, stream: Optional[int] = None):
        """mpcb_step_warm: step_ref() with one warm-start mode per simulation -- `warm` a contiguous int32 device tensor [batch] of
        WARM_CARRY / WARM_RESET / WARM_SHIFT, or None: every simulation carries, which is step_ref() exactly."""
        if stream is None:
            import torch

            stream = torch.cuda.current_stream(self.device).cuda_stream
        r = self._step_struct(io)
        yp = C.cast(C.c_void_p(yref.data_ptr()), _dp) if yref is not None else None
        wp = C.cast(C.c_void_p(warm.data_ptr()), _ip) if warm is not None else None
        self._check(self.lib.mpcb_step_warm(self._h, C.byref(r), yp, int(bool(ref_changed)), wp, int(bool(reset)), C.c_void_p(stream)),
                    "mpcb_step_warm")

    def set_weights(self, weights, stream: Optional[int] = None):
        """mpcb_set_weights: the seven cost weights of every simulation <- `weights`, a contiguous device tensor [batch, 7] float64
        (w_u, w_qddot, the task weights of g1..g5), read during the launch only; asynchronous on `stream` (default: the current
        torch stream).  The next step linearises again at its start."""
        if stream is None:
            import torch

            stream = torch.cuda.current_stream(self.device).cuda_stream
        self._check(self.lib.mpcb_set_weights(self._h, C.cast(C.c_void_p(weights.data_ptr()), _dp), C.c_void_p(stream)),
                    "mpcb_set_weights")

    def step_sens(self, io, yref=None, ref_changed: bool = False, warm=None, reset: bool = False, sens=None,
                  stream: Optional[int] = None, du0_dw=None, term=None, term_changed: bool = False, du0_dxe=None):
        """mpcb_step_sens: step_warm() that also writes the sensitivities of u0 -- `sens` a dict of contiguous device tensors
        du0_dx [batch, 6, 12] float64, valid [batch] int32 and optionally du0_dyref [batch, N, 5, 6] float64, or None: step_warm()
        exactly.  `du0_dw` (a contiguous device tensor [batch, 7, 6] float64; needs `sens`): mpcb_step_sens_w, which also writes
        the sensitivity of u0 to the cost weights there.  `term` (a contiguous device tensor [batch, 30] float64: pqq 6 | pqv 6 |
        pvv 6 | x_e 12 per simulation) or `term_changed`: mpcb_step_term, the step with that joint-wise terminal cost in force,
        which linearises again first when `term_changed`; `du0_dxe` (a contiguous device tensor [batch, 6, 12] float64; needs
        `sens` and `term`) takes d u0 / d x_e.  Not together with `du0_dw`."""
        if stream is None:
            import torch

            stream = torch.cuda.current_stream(self.device).cuda_stream
        r = self._step_struct(io)
        yp = C.cast(C.c_void_p(yref.data_ptr()), _dp) if yref is not None else None
        wp = C.cast(C.c_void_p(warm.data_ptr()), _ip) if warm is not None else None
        sp = None
        if sens is not None:
            dy = sens.get("du0_dyref")
            so = MpcbStepSensOut(C.cast(C.c_void_p(sens["du0_dx"].data_ptr()), _dp),
                                 C.cast(C.c_void_p(dy.data_ptr()), _dp) if dy is not None else None,
                                 C.cast(C.c_void_p(sens["valid"].data_ptr()), _ip))
            sp = C.byref(so)
        if term is not None or term_changed or du0_dxe is not None:
            if du0_dw is not None:
                raise EngineError("the weight sensitivity (du0_dw) is not offered together with a terminal cost")
            self._check(self.lib.mpcb_step_term(self._h, C.byref(r), yp, int(bool(ref_changed)), wp, int(bool(reset)), sp,
                                                C.cast(C.c_void_p(term.data_ptr()), _dp) if term is not None else None,
                                                int(bool(term_changed)),
                                                C.cast(C.c_void_p(du0_dxe.data_ptr()), _dp) if du0_dxe is not None else None,
                                                C.c_void_p(stream)), "mpcb_step_term")
            return
        if du0_dw is not None:
            self._check(self.lib.mpcb_step_sens_w(self._h, C.byref(r), yp, int(bool(ref_changed)), wp, int(bool(reset)), sp,
                                                  C.cast(C.c_void_p(du0_dw.data_ptr()), _dp), C.c_void_p(stream)), "mpcb_step_sens_w")
            return
        self._check(self.lib.mpcb_step_sens(self._h, C.byref(r), yp, int(bool(ref_changed)), wp, int(bool(reset)), sp,
                                            C.c_void_p(stream)), "mpcb_step_sens")

    def step_dist(self, io, yref=None, ref_changed: bool = False, warm=None, reset: bool = False, dist=None,
                  dist_changed: bool = False, stream: Optional[int] = None):
        """mpcb_step_dist: step_warm() whose prediction model carries the input disturbance `dist`, a contiguous float64 device
        tensor [batch, 6] in rad/s (x+ = Ad x + Bd (u + d)), or None: step_warm().  `dist_changed`: the disturbance differs from the
        previous step's, or was switched on or off (the step linearises again first)."""
        if stream is None:
            import torch

            stream = torch.cuda.current_stream(self.device).cuda_stream
        r = self._step_struct(io)
        yp = C.cast(C.c_void_p(yref.data_ptr()), _dp) if yref is not None else None
        wp = C.cast(C.c_void_p(warm.data_ptr()), _ip) if warm is not None else None
        dp = C.cast(C.c_void_p(dist.data_ptr()), _dp) if dist is not None else None
        self._check(self.lib.mpcb_step_dist(self._h, C.byref(r), yp, int(bool(ref_changed)), wp, int(bool(reset)), dp,
                                            int(bool(dist_changed)), C.c_void_p(stream)), "mpcb_step_dist")

    def step_surf(self, io, yref=None, ref_changed: bool = False, warm=None, reset: bool = False, surf=None,
                  surf_changed: bool = False, stream: Optional[int] = None):
        """mpcb_step_surf: step_warm() whose stage k evaluates the task functions on the quadric of row k of `surf`, a contiguous
        float64 device tensor [batch, N, 6] (a..f per stage; N the longest horizon), or None: step_warm().  `surf_changed`: the
        window differs from the previous step's, or was switched on or off (the step linearises again first)."""
        if surf is not None:
            pb = self._pb
            if not hasattr(surf, "data_ptr") or tuple(surf.shape) != (pb.batch, pb.N, 6) or not surf.is_contiguous() \
                    or str(surf.dtype) != "torch.float64" or not surf.is_cuda:
                raise ValueError(f"surf must be a contiguous float64 device tensor [{pb.batch}, {pb.N}, 6], got "
                                 f"{tuple(getattr(surf, 'shape', ()))} {getattr(surf, 'dtype', type(surf).__name__)}")
        if stream is None:
            import torch

            stream = torch.cuda.current_stream(self.device).cuda_stream
        r = self._step_struct(io)
        yp = C.cast(C.c_void_p(yref.data_ptr()), _dp) if yref is not None else None
        wp = C.cast(C.c_void_p(warm.data_ptr()), _ip) if warm is not None else None
        sp = C.cast(C.c_void_p(surf.data_ptr()), _dp) if surf is not None else None
        self._check(self.lib.mpcb_step_surf(self._h, C.byref(r), yp, int(bool(ref_changed)), wp, int(bool(reset)), sp,
                                            int(bool(surf_changed)), C.c_void_p(stream)), "mpcb_step_surf")

    def step_combined(self, io, yref=None, ref_changed: bool = False, warm=None, reset: bool = False, term=None,
                      term_changed: bool = False, dist=None, dist_changed: bool = False, surf=None, surf_changed: bool = False,
                      stream: Optional[int] = None):
        """mpcb_step_combined: the controller step in which the terminal cost `term` [batch, 30], the input disturbance `dist`
        [batch, 6], the surface window `surf` [batch, N, 6] and the warm-start modes `warm` [batch] are in force at once -- each a
        contiguous device tensor as in step_sens / step_dist / step_surf / step_warm, or None: absent for the whole batch (the
        library then fills neutral data: zero blocks, d = 0, the packed surface on every row).  A simulation that does not use a
        feature brings neutral rows itself.  `*_changed`: the step linearises again first.  SQP_RTI and fp64 only."""
        pb = self._pb
        for name, t, shape in (("term", term, (pb.batch, 30)), ("dist", dist, (pb.batch, 6)), ("surf", surf, (pb.batch, pb.N, 6))):
            if t is not None and (not hasattr(t, "data_ptr") or tuple(t.shape) != shape or not t.is_contiguous()
                                  or str(t.dtype) != "torch.float64" or not t.is_cuda):
                raise ValueError(f"{name} must be a contiguous float64 device tensor {list(shape)}, got "
                                 f"{tuple(getattr(t, 'shape', ()))} {getattr(t, 'dtype', type(t).__name__)}")
        if stream is None:
            import torch

            stream = torch.cuda.current_stream(self.device).cuda_stream
        r = self._step_struct(io)

        def ptr(t, ty=_dp):
            return C.cast(C.c_void_p(t.data_ptr()), ty) if t is not None else None

        self._check(self.lib.mpcb_step_combined(self._h, C.byref(r), ptr(yref), int(bool(ref_changed)), ptr(warm, _ip), int(bool(reset)),
                                                ptr(term), int(bool(term_changed)), ptr(dist), int(bool(dist_changed)), ptr(surf),
                                                int(bool(surf_changed)), C.c_void_p(stream)), "mpcb_step_combined")

    def debug_task_lin(self, cfgs: Sequence[Dict], chain, x: np.ndarray) -> np.ndarray:
        """Diagnostic: the device linearisation at points x[i] = [q; qdot] with the parameters of cfgs[i];
        returns [n, 60] records laid out like a G2 stage record (r 0..4, dg/dq 24..53, dg5/dqdot 54..59)."""
        n = len(cfgs)
        params = packing.pack_batch(cfgs)
        robot = np.ascontiguousarray(chain.packed(cfgs[0]["t_ee"]), dtype=np.float64)
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(n, 12)
        rec = np.zeros((n, 60))
        self._check(self.lib.mpcb_debug_task_lin(self._h, n, params.ctypes.data_as(_dp), robot.ctypes.data_as(_dp),
                                                 x.ctypes.data_as(_dp), rec.ctypes.data_as(_dp)), "mpcb_debug_task_lin")
        return rec

    def kernel_ms(self) -> float:
        ms = C.c_float(0)
        self._check(self.lib.mpcb_last_kernel_ms(self._h, C.byref(ms)), "mpcb_last_kernel_ms")
        return float(ms.value)

    def run_device(self, cfgs: Sequence[Dict], chain, step_chunk: int = 0):
        """setup + all steps; returns (problem, dict of device tensors). Synchronous."""
        pb = self.setup(cfgs, chain)
        bufs = self.alloc_results(pb)
        comb = self.combined_tensors(cfgs)     # a bucket with combine_features: every table, neutral rows where a feature is off
        if comb is not None:
            chunk = step_chunk if step_chunk and step_chunk > 0 else pb.Nsim
            self.last_kernel_ms = []
            for s0 in range(0, pb.Nsim, chunk):
                self.rollout(bufs, s0, min(pb.Nsim, s0 + chunk), combined=True, **comb)
                self.sync()
                self.last_kernel_ms.append(self.kernel_ms())
            bufs["d_hat"] = comb["obs"]["d_hat"]
            return pb, bufs
        yref = self.schedule_tensor(cfgs)      # sampled and stacked once; every chunk gets the same array
        pert = self.perturbation_tensors(cfgs)
        term = self.terminal_tensors(cfgs)
        obs = self.observer_tensors(cfgs)
        surf = self.surface_tensor(cfgs)
        warm = self.warm_tensor(cfgs)
        chunk = step_chunk if step_chunk and step_chunk > 0 else pb.Nsim
        self.last_kernel_ms = []
        for s0 in range(0, pb.Nsim, chunk):
            self.rollout(bufs, s0, min(pb.Nsim, s0 + chunk), yref=yref, pert=pert, term=term, obs=obs, surf=surf, warm=warm)
            self.sync()
            self.last_kernel_ms.append(self.kernel_ms())
        if obs is not None:
            bufs["d_hat"] = obs["d_hat"]       # [batch, Nsim, 6]: the estimate every step used, beside the result logs
        return pb, bufs

    def run(self, cfgs: Sequence[Dict], chain, step_chunk: int = 0) -> Dict[str, np.ndarray]:
        """Whole bucket, results as numpy arrays [batch, ...] (D2H copy included)."""
        _, bufs = self.run_device(cfgs, chain, step_chunk)
        return {k: v.cpu().numpy() for k, v in bufs.items()}

    # ------------------------------------------------------------------ host-buffer path
    def run_host_buffers(self, cfgs: Sequence[Dict], chain) -> Dict[str, np.ndarray]:
        """Same through mpcb_run (library-owned device buffers, numpy in/out, no torch).  mpcb_run takes no reference schedule:
        configurations that carry one are refused, and so are configurations with a plant perturbation, a terminal cost or a
        disturbance observer."""
        if any(c.get("combine_features") for c in cfgs):
            raise ValueError("mpcb_run takes no combined features: run configurations with combine_features through run() / run_device()")
        if any(c.get("reference_schedule") is not None for c in cfgs):
            raise ValueError("mpcb_run takes no reference schedule: run configurations with a reference_schedule through run() / run_device()")
        if any(c.get("plant_perturbation") is not None for c in cfgs):
            raise ValueError("mpcb_run takes no plant perturbation: run configurations with a plant_perturbation through run() / run_device()")
        if any(c.get("terminal_cost") is not None for c in cfgs):
            raise ValueError("mpcb_run takes no terminal cost: run configurations with a terminal_cost through run() / run_device()")
        if any(c.get("disturbance_observer") is not None for c in cfgs):
            raise ValueError("mpcb_run takes no disturbance observer: run configurations with a disturbance_observer through run() / "
                             "run_device()")
        if any(c.get("warm_start", "carry") == "shift" for c in cfgs):
            raise ValueError("mpcb_run takes no warm-start modes: run configurations with warm_start='shift' through run() / run_device()")
        if any(c.get("surface_schedule") is not None for c in cfgs):
            raise ValueError("mpcb_run takes no surface schedule: run configurations with a surface_schedule through run() / run_device()")
        pb = make_problem(cfgs)
        params = packing.pack_batch(cfgs)
        robot = np.ascontiguousarray(chain.packed(cfgs[0]["t_ee"]), dtype=np.float64)
        S, T = pb.Nsim, pb.Nsim + 1
        out = {name: np.zeros((pb.batch,) + shp(S, T), dtype=np.float64 if ty == "f8" else np.int32)
               for name, ty, shp in RESULT_FIELDS}
        r = self._result_struct(out)
        self._check(self.lib.mpcb_run(self._h, C.byref(pb), params.ctypes.data_as(_dp), robot.ctypes.data_as(_dp),
                                      C.byref(r)), "mpcb_run")
        return out
