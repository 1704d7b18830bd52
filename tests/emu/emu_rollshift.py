"""Loader for the TEST-ONLY host emulation of the rollout with the shift warm start (see emu_rollshift_harness.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np

import emu
import emu_rollpert
import emu_surf
import emu_warm

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "libmpc_emu_rollshift.so")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)

CARRY, SHIFT = emu_warm.CARRY, emu_warm.SHIFT


def build(force=False):
    srcs = [os.path.join(_HERE, f) for f in ("emu_rollshift_harness.cpp", "emu_rollsurf_harness.cpp", "emu_rollpert_harness.cpp",
                                             "emu_rollref_harness.cpp", "emu_ref_harness.cpp", "emu_step_harness.cpp",
                                             "emu_harness.cpp")] + \
        [os.path.join(emu._CSRC, f) for f in os.listdir(emu._CSRC) if f.endswith(".h")]
    if force or not os.path.exists(_LIB) or os.path.getmtime(_LIB) < max(os.path.getmtime(s) for s in srcs):
        subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-O2", "-fPIC", "-shared", "-ffp-contract=off",
                               "-o", _LIB, os.path.join(_HERE, "emu_rollshift_harness.cpp")])
    return _LIB


def rollout(cfgs, chain, sched, warm, surf=None, wcv=None, u_dist=None, x_noise=None, step_chunk=0, pool_doubles=0, waves=1):
    """Engine<.., 0, 0, SURF>::rollout<true, true, false, true> for one bucket of resolved configs against sched [B, Nsim + N, 5]
    with the warm-start modes warm [B] (CARRY / SHIFT), on the surface table surf [B, Nsim + N, 6] or the packed surface (None),
    over the plant of emu_rollpert.rollout (each perturbation may be None); dict of arrays [B, ...].  warm None: emu_rollpert.rollout
    (emu_rollsurf.rollout with a table), as mpcb_rollout_warm hands a null `warm` on."""
    from robotic_mpc_amd import packing

    if warm is None:
        if surf is None:
            return emu_rollpert.rollout(cfgs, chain, sched, wcv=wcv, u_dist=u_dist, x_noise=x_noise, step_chunk=step_chunk,
                                        pool_doubles=pool_doubles, waves=waves)
        import emu_rollsurf

        return emu_rollsurf.rollout(cfgs, chain, sched, surf, wcv=wcv, u_dist=u_dist, x_noise=x_noise, step_chunk=step_chunk,
                                    pool_doubles=pool_doubles, waves=waves)
    lib = C.CDLL(build())
    c0 = cfgs[0]
    B, N, Nsim = len(cfgs), c0["N"], c0["Nsim"]
    pb = emu.Problem(B, N, Nsim, c0["solver_type"], c0["max_iter"], c0["qp_iter_max"], int(c0["fixed_step"]), 0)
    params = packing.pack_batch(cfgs)
    robot = np.ascontiguousarray(chain.packed(c0["t_ee"]))
    y = np.ascontiguousarray(sched, dtype=np.float64)
    assert y.shape == (B, Nsim + N, 5)
    w = np.ascontiguousarray(np.broadcast_to(warm, (B,)), dtype=np.int32)
    keep = [emu_rollpert._opt(wcv, (B, 6)), emu_rollpert._opt(u_dist, (B, Nsim, 6)), emu_rollpert._opt(x_noise, (B, Nsim, 12)),
            emu_rollpert._opt(surf, (B, Nsim + N, 6))]
    T1 = Nsim + 1
    o = dict(z=np.zeros((B, 12, T1)), u=np.zeros((B, 6, T1)), ee_pose=np.zeros((B, 12, T1)), ee_rpy=np.zeros((B, 3, T1)),
             ee_vel=np.zeros((B, 6, T1)), status=np.zeros((B, Nsim), np.int32), sqp_iter=np.zeros((B, Nsim), np.int32),
             qp_iter=np.zeros((B, Nsim), np.int32), residuals=np.zeros((B, Nsim, 4)), cost=np.zeros((B, Nsim)),
             solver_time=np.zeros((B, Nsim)), errors=np.zeros((B, 7, T1)), plant_time=np.zeros((B, Nsim)))
    args = [C.byref(pb), robot.ctypes.data_as(_dp), params.ctypes.data_as(_dp)]
    args += [o[k].ctypes.data_as(_dp) for k in ("z", "u", "ee_pose", "ee_rpy", "ee_vel")]
    args += [o[k].ctypes.data_as(_ip) for k in ("status", "sqp_iter", "qp_iter")]
    args += [o[k].ctypes.data_as(_dp) for k in ("residuals", "cost", "solver_time", "errors", "plant_time")]
    args += [y.ctypes.data_as(_dp)] + [p for _, p in keep] + [w.ctypes.data_as(_ip)]
    args += [C.c_int(step_chunk), C.c_int(pool_doubles), C.c_int(waves)]
    assert lib.emu_rollout_shift(*args) == 0
    return o


plant_rk = emu_rollpert.plant_rk
# the yardsticks: the emulated control_step with a warm-start mode per simulation (emu_warm_harness.cpp), and the one that takes a
# surface window as well (emu_surf_harness.cpp)
Controller = emu_warm.Controller
SurfController = emu_surf.Controller


def step_loop(cfgs, chain, sched, pert, modes, surf=None, pool=0, waves=1):
    """What defines the rollout: Controller.step(z_t + noise_t, yref = window t, ref_changed = True, warm = modes if t >= 1), with
    surface = window t of `surf` when there is a table, over plant_rk from the true state with the disturbed input.  `modes` [B] or
    a scalar; CARRY everywhere is the perturbed rollout's loop."""
    steps, N, B = cfgs[0]["Nsim"], cfgs[0]["N"], len(cfgs)
    ctl = (Controller if surf is None else SurfController)(cfgs, chain, pool_doubles=pool, waves=waves)
    modes = np.ascontiguousarray(np.broadcast_to(modes, (B,)), dtype=np.int32)
    zt = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    o = dict(z=np.zeros((B, 12, steps + 1)), u=np.zeros((B, 6, steps + 1)), cost=np.zeros((B, steps)), residuals=np.zeros((B, steps, 4)),
             status=np.zeros((B, steps), np.int32), sqp_iter=np.zeros((B, steps), np.int32), qp_iter=np.zeros((B, steps), np.int32))
    o["z"][:, :, 0] = zt
    o["u"][:, :, 0] = np.stack([c["qdot0"] for c in cfgs])                 # u[:, 0] = qdot_0
    for t in range(steps):
        kw = {} if surf is None else dict(surface=surf[:, t:t + N])
        out = ctl.step(zt + pert["x_noise"][:, t], yref=sched[:, t:t + N], ref_changed=True, predict=False,
                       warm=modes if t >= 1 else np.zeros(B, np.int32), **kw)
        for k in ("cost", "residuals", "status", "sqp_iter", "qp_iter"):
            o[k][:, t] = out[k]
        zt = np.stack([plant_rk(c, pert["wcv"][i], zt[i], out["u0"][i] + pert["u_dist"][i, t]) for i, c in enumerate(cfgs)])
        o["z"][:, :, t + 1] = zt
        o["u"][:, :, t + 1] = out["u0"]
    return o
