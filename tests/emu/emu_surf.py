"""Loader for the TEST-ONLY host emulation of the controller step over a scheduled surface (see emu_surf_harness.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libmpc_emu_surf.so")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

CARRY, RESET, SHIFT = 0, 1, 2


def build(force=False):
    srcs = [os.path.join(_HERE, f) for f in ("emu_surf_harness.cpp", "emu_warm_harness.cpp", "emu_step_harness.cpp",
                                             "emu_harness.cpp")] + \
        [os.path.join(emu._CSRC, f) for f in os.listdir(emu._CSRC) if f.endswith(".h")]
    if force or not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-O2", "-fPIC", "-shared", "-ffp-contract=off",
                               "-o", _LIB, os.path.join(_HERE, "emu_surf_harness.cpp")])
    return _LIB


class Controller:
    """The engine's control_step for a batch of resolved configs (one bucket), workspaces kept between steps.
    set_surface(coeffs [B, N, 6] or [N, 6], or None) puts a surface window in force; the next step linearises again, as
    surf_changed of mpcb_step_surf sees to.  step(x, ..., surface=w) is set_surface(w) followed by the step."""

    _KEEP = object()

    def __init__(self, cfgs, chain, pool_doubles=0, waves=1):
        from robotic_mpc_amd import packing

        self.lib = C.CDLL(build())
        self.lib.emu_ctl_create.restype = C.c_void_p
        self.lib.emu_ctl_destroy.argtypes = [C.c_void_p]
        self.lib.emu_step_surf.argtypes = [C.c_void_p, _dp, _dp, C.c_int, _ip, C.c_int] + [_dp, _ip, _ip, _ip, _dp, _dp, _dp, _dp, _dp] + [_dp]
        c0 = cfgs[0]
        self.B, self.N = len(cfgs), c0["N"]
        pb = emu.Problem(self.B, self.N, c0["Nsim"], c0["solver_type"], c0["max_iter"], c0["qp_iter_max"], int(c0["fixed_step"]), 0)
        params = packing.pack_batch(cfgs)
        robot = np.ascontiguousarray(chain.packed(c0["t_ee"]))
        self.h = C.c_void_p(self.lib.emu_ctl_create(C.byref(pb), robot.ctypes.data_as(_dp), params.ctypes.data_as(_dp),
                                                     C.c_int(pool_doubles), C.c_int(waves)))
        self._reset = True
        self._surf = None
        self._stale = False

    def set_surface(self, w):
        self._surf = None if w is None else np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=np.float64), (self.B, self.N, 6))).copy()
        self._stale = True

    def step(self, xhat, yref=None, ref_changed=False, warm=None, reset=False, predict=True, surface=_KEEP):
        if surface is not Controller._KEEP:
            self.set_surface(surface)
        B, N = self.B, self.N
        x = np.ascontiguousarray(xhat, dtype=np.float64).reshape(B, 12)
        y = None if yref is None else np.ascontiguousarray(np.broadcast_to(yref, (B, N, 5)), dtype=np.float64)
        w = None if warm is None else np.ascontiguousarray(np.broadcast_to(warm, (B,)), dtype=np.int32)
        o = dict(u0=np.zeros((B, 6)), status=np.zeros(B, np.int32), sqp_iter=np.zeros(B, np.int32), qp_iter=np.zeros(B, np.int32),
                 residuals=np.full((B, 4), np.nan), cost=np.zeros(B), solver_time=np.full(B, np.nan))
        if predict:
            o["x_pred"], o["u_pred"] = np.zeros((B, N + 1, 12)), np.zeros((B, N, 6))
        ptr = lambda k: o[k].ctypes.data_as(_ip if o[k].dtype == np.int32 else _dp) if k in o else None
        rc = self.lib.emu_step_surf(self.h, x.ctypes.data_as(_dp), None if y is None else y.ctypes.data_as(_dp),
                                    C.c_int(int(bool(ref_changed or self._stale))), None if w is None else w.ctypes.data_as(_ip),
                                    C.c_int(int(reset or self._reset)),
                                    *[ptr(k) for k in ("u0", "status", "sqp_iter", "qp_iter", "residuals", "cost", "solver_time",
                                                       "x_pred", "u_pred")],
                                    None if self._surf is None else self._surf.ctypes.data_as(_dp))
        assert rc == 0, rc
        self._reset = False
        self._stale = False
        return o

    def __del__(self):
        try:
            self.lib.emu_ctl_destroy(self.h)
        except Exception:
            pass
