"""Loader for the TEST-ONLY host emulation of the combined controller step and rollout (see emu_combined_harness.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu
import emu_rollpert

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libmpc_emu_combined.so")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

CARRY, RESET, SHIFT = 0, 1, 2


def build(force=False):
    srcs = [os.path.join(_HERE, f) for f in ("emu_combined_harness.cpp", "emu_rollpert_harness.cpp", "emu_rollref_harness.cpp",
                                             "emu_ref_harness.cpp", "emu_step_harness.cpp", "emu_harness.cpp")] + \
        [os.path.join(emu._CSRC, f) for f in os.listdir(emu._CSRC) if f.endswith(".h")]
    if force or not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-O2", "-fPIC", "-shared", "-ffp-contract=off",
                               "-o", _LIB, os.path.join(_HERE, "emu_combined_harness.cpp")])
    return _LIB


def term_record(blocks, x_e):
    """[B, 30] = pqq 6 | pqv 6 | pvv 6 | x_e 12 from blocks [B, 6, 3] (or [6, 3]) and x_e [B, 12] (or [12])."""
    x_e = np.atleast_2d(np.asarray(x_e, dtype=np.float64))
    B = x_e.shape[0]
    b = np.broadcast_to(np.asarray(blocks, dtype=np.float64), (B, 6, 3))
    return np.ascontiguousarray(np.concatenate([b[:, :, 0], b[:, :, 1], b[:, :, 2], x_e], axis=1))


class Controller:
    """Engine<.., 1, 1, 1>::control_step<true> for a batch of resolved configs (one bucket), workspaces kept between steps.
    set_terminal(record [B, 30] or None), set_dist(d [B, 6] or None), set_surface(w [B, N, 6] or None) put a feature in force or
    switch it off; what is off is handed to the engine as its NEUTRAL table (zeros; the packed a..f on every row), as the library's
    host layer does.  Any change makes the next step linearise again."""

    _KEEP = object()

    def __init__(self, cfgs, chain, pool_doubles=0, waves=1):
        from robotic_mpc_amd import packing

        self.lib = C.CDLL(build())
        self.lib.emu_ctl_create.restype = C.c_void_p
        self.lib.emu_ctl_destroy.argtypes = [C.c_void_p]
        self.lib.emu_step_combined.argtypes = [C.c_void_p, _dp, _dp, C.c_int, _ip, C.c_int] + [_dp, _ip, _ip, _ip, _dp, _dp, _dp, _dp, _dp] + [_dp] * 3
        c0 = cfgs[0]
        self.B, self.N = len(cfgs), c0["N"]
        pb = emu.Problem(self.B, self.N, c0["Nsim"], c0["solver_type"], c0["max_iter"], c0["qp_iter_max"], int(c0["fixed_step"]), 0)
        params = packing.pack_batch(cfgs)
        robot = np.ascontiguousarray(chain.packed(c0["t_ee"]))
        self.h = C.c_void_p(self.lib.emu_ctl_create(C.byref(pb), robot.ctypes.data_as(_dp), params.ctypes.data_as(_dp),
                                                     C.c_int(pool_doubles), C.c_int(waves)))
        self._neutral_surf = np.ascontiguousarray(np.repeat(np.stack([np.asarray(c["coeffs"], dtype=np.float64) for c in cfgs])[:, None, :],
                                                            self.N, axis=1))
        self._reset = True
        self._term = self._dist = self._surf = None
        self._stale = False

    def set_terminal(self, rec):
        self._term = None if rec is None else np.ascontiguousarray(np.broadcast_to(np.asarray(rec, dtype=np.float64), (self.B, 30))).copy()
        self._stale = True

    def set_dist(self, d):
        self._dist = None if d is None else np.ascontiguousarray(np.broadcast_to(np.asarray(d, dtype=np.float64), (self.B, 6))).copy()
        self._stale = True

    def set_surface(self, w):
        self._surf = None if w is None else np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=np.float64), (self.B, self.N, 6))).copy()
        self._stale = True

    def step(self, xhat, yref=None, ref_changed=False, warm=None, reset=False, predict=True, term=_KEEP, dist=_KEEP, surface=_KEEP):
        if term is not Controller._KEEP:
            self.set_terminal(term)
        if dist is not Controller._KEEP:
            self.set_dist(dist)
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
        ptr = lambda k: o[k].ctypes.data_as(_ip if o[k].dtype == np.int32 else _dp) if k in o else None   # noqa: E731
        tm = self._term if self._term is not None else np.zeros((B, 30))
        di = self._dist if self._dist is not None else np.zeros((B, 6))
        su = self._surf if self._surf is not None else self._neutral_surf
        rc = self.lib.emu_step_combined(self.h, x.ctypes.data_as(_dp), None if y is None else y.ctypes.data_as(_dp),
                                        C.c_int(int(bool(ref_changed or self._stale))), None if w is None else w.ctypes.data_as(_ip),
                                        C.c_int(int(reset or self._reset)),
                                        *[ptr(k) for k in ("u0", "status", "sqp_iter", "qp_iter", "residuals", "cost", "solver_time",
                                                           "x_pred", "u_pred")],
                                        tm.ctypes.data_as(_dp), di.ctypes.data_as(_dp), su.ctypes.data_as(_dp))
        assert rc == 0, rc
        self._reset = False
        self._stale = False
        return o

    def __del__(self):
        try:
            self.lib.emu_ctl_destroy(self.h)
        except Exception:
            pass


def rollout(cfgs, chain, tabs, bounds=None, pool_doubles=0, waves=1):
    """Engine<.., TERM_TABLE, DIST_SHARED, 1>::rollout<true, true, true, true> for one bucket of resolved configs with the tables
    `tabs` of robotic_mpc_amd.engine.combined_arrays(cfgs) (every table present, neutral rows where a simulation does not use a
    feature), one launch per interval of `bounds` (default: one launch); dict of arrays [B, ...], "d_hat" [B, Nsim, 6] among them."""
    from robotic_mpc_amd import packing

    lib = C.CDLL(build())
    c0 = cfgs[0]
    B, N, Nsim = len(cfgs), c0["N"], c0["Nsim"]
    pb = emu.Problem(B, N, Nsim, c0["solver_type"], c0["max_iter"], c0["qp_iter_max"], int(c0["fixed_step"]), 0)
    params = packing.pack_batch(cfgs)
    robot = np.ascontiguousarray(chain.packed(c0["t_ee"]))
    bnd = np.ascontiguousarray([0, Nsim] if bounds is None else bounds, dtype=np.int32)
    assert bnd[0] == 0 and bnd[-1] == Nsim and (np.diff(bnd) > 0).all()
    f8 = lambda a, shape: np.ascontiguousarray(a, dtype=np.float64).reshape(shape)   # noqa: E731
    keep = [f8(tabs["yref"], (B, Nsim + N, 5)), f8(tabs["pert"]["wcv"], (B, 6)), f8(tabs["pert"]["u_dist"], (B, Nsim, 6)),
            f8(tabs["pert"]["x_noise"], (B, Nsim, 12)), f8(tabs["term"]["blocks"], (B, 18)), f8(tabs["term"]["x_ref"], (B, Nsim, 12)),
            f8(tabs["gain"], (B, 12))]
    surf = f8(tabs["surf"], (B, Nsim + N, 6))
    warm = np.ascontiguousarray(tabs["warm"], dtype=np.int32).reshape(B)
    T1 = Nsim + 1
    o = dict(z=np.zeros((B, 12, T1)), u=np.zeros((B, 6, T1)), ee_pose=np.zeros((B, 12, T1)), ee_rpy=np.zeros((B, 3, T1)),
             ee_vel=np.zeros((B, 6, T1)), status=np.zeros((B, Nsim), np.int32), sqp_iter=np.zeros((B, Nsim), np.int32),
             qp_iter=np.zeros((B, Nsim), np.int32), residuals=np.zeros((B, Nsim, 4)), cost=np.zeros((B, Nsim)),
             solver_time=np.zeros((B, Nsim)), errors=np.zeros((B, 7, T1)), plant_time=np.zeros((B, Nsim)),
             d_hat=np.full((B, Nsim, 6), np.nan))
    args = [C.byref(pb), robot.ctypes.data_as(_dp), params.ctypes.data_as(_dp)]
    args += [o[k].ctypes.data_as(_dp) for k in ("z", "u", "ee_pose", "ee_rpy", "ee_vel")]
    args += [o[k].ctypes.data_as(_ip) for k in ("status", "sqp_iter", "qp_iter")]
    args += [o[k].ctypes.data_as(_dp) for k in ("residuals", "cost", "solver_time", "errors", "plant_time")]
    args += [a.ctypes.data_as(_dp) for a in keep] + [o["d_hat"].ctypes.data_as(_dp), surf.ctypes.data_as(_dp), warm.ctypes.data_as(_ip)]
    args += [bnd.ctypes.data_as(_ip), C.c_int(len(bnd)), C.c_int(pool_doubles), C.c_int(waves)]
    assert lib.emu_rollout_combined(*args) == 0
    return o


plant_rk = emu_rollpert.plant_rk


def step_loop(cfgs, chain, tabs, pool=0, waves=1, off=()):
    """What DEFINES the combined rollout: Controller.step(z_t + noise_t, yref = window t, surface = window t, dist = d^_t,
    warm = mode if t >= 1) with the terminal record [blocks | x_ref[:, t]] set before every step and the torch DisturbanceObserver
    (gains of `tabs`) updated from the measurement and the commanded input, over plant_rk from the true state with the disturbed
    input.  `off`: features switched off for the guards ("term", "obs", "surf", "shift") -- their tables replaced by neutral ones."""
    import torch

    steps, N, B = cfgs[0]["Nsim"], cfgs[0]["N"], len(cfgs)
    ctl = Controller(cfgs, chain, pool_doubles=pool, waves=waves)
    pert, term = tabs["pert"], tabs["term"]
    gain = np.zeros((B, 12)) if "obs" in off else np.asarray(tabs["gain"], dtype=np.float64)
    blocks = np.zeros((B, 18)) if "term" in off else term["blocks"]
    surf = np.repeat(np.stack([c["coeffs"] for c in cfgs])[:, None, :], steps + N, axis=1) if "surf" in off else tabs["surf"]
    modes = np.zeros(B, np.int32) if "shift" in off else np.asarray(tabs["warm"], dtype=np.int32)
    a22 = np.stack([np.exp(-np.asarray(c["wcv"], dtype=np.float64) * c["dt"]) for c in cfgs])
    b2 = 1.0 - a22
    zt = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    o = dict(z=np.zeros((B, 12, steps + 1)), u=np.zeros((B, 6, steps + 1)), cost=np.zeros((B, steps)), residuals=np.zeros((B, steps, 4)),
             status=np.zeros((B, steps), np.int32), sqp_iter=np.zeros((B, steps), np.int32), qp_iter=np.zeros((B, steps), np.int32),
             d_hat=np.zeros((B, steps, 6)))
    o["z"][:, :, 0] = zt
    o["u"][:, :, 0] = np.stack([c["qdot0"] for c in cfgs])
    # DisturbanceObserver.update of observer.py with explicit gains (a simulation without an observer has l1 = l2 = 0), in torch
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))   # noqa: E731
    ta22, tb2, l1, l2 = T(a22), T(b2), T(gain[:, :6]), T(gain[:, 6:])
    v = d = y_prev = None
    u_prev = torch.zeros(B, 6, dtype=torch.float64)
    for t in range(steps):
        xhat = zt + pert["x_noise"][:, t]
        y = T(xhat[:, 6:]).clone()
        if v is None:
            v, d = y.clone(), torch.zeros_like(y)
        else:
            innov = y_prev - v
            v, d = ta22 * v + tb2 * (u_prev + d) + l1 * innov, d + l2 * innov
        y_prev = y
        o["d_hat"][:, t] = d.numpy()
        rec = np.concatenate([blocks, term["x_ref"][:, t]], axis=1)
        out = ctl.step(xhat, yref=tabs["yref"][:, t:t + N], ref_changed=True, predict=False, term=rec, dist=d.numpy(),
                       surface=surf[:, t:t + N], warm=modes if t >= 1 else np.zeros(B, np.int32))
        for k in ("cost", "residuals", "status", "sqp_iter", "qp_iter"):
            o[k][:, t] = out[k]
        zt = np.stack([plant_rk(c, pert["wcv"][i], zt[i], out["u0"][i] + pert["u_dist"][i, t]) for i, c in enumerate(cfgs)])
        o["z"][:, :, t + 1] = zt
        o["u"][:, :, t + 1] = out["u0"]
        u_prev = T(out["u0"]).clone()
    return o
