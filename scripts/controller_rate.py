#!/usr/bin/env python3
"""Closed-loop rate of the controller step (BatchController / mpcb_step) against the rollout (mpcb_rollout) on BASELINE
configs[1]'s shape: batch 256, N = 100, SQP_RTI, 600 closed-loop steps (bench.workload_configs).

The step path closes the loop over an RK4 plant written in torch on the device (the model's own dynamics, q' = qdot,
qdot' = wcv (u - qdot)), so no host round trip sits in the loop.  Both paths are timed with device events after a warm-up
run; the step path also reports the device time of the step launches alone (events around each launch).  Prints one JSON line
per (batch, engine) pair.

`--engine` takes one or more kernel families (BatchController's engine=, "latency" by default) and `--batch` one or more batch
sizes: every batch runs on each engine in turn, alternating, in one process.  The rollout is timed on the same family
(MPCB_ENGINE) unless --skip-rollout.  `--ref` takes one or more task-reference modes: none (the packed reference), once (a
per-stage tracking reference set before the loop) and every (a new one every step: the copy and one more linearisation per step).
`--warm` takes one or more warm starts: carry (step k starts from step k-1's iterate at the same stages) and shift (from that
iterate moved one stage, BatchController.step(shift=True): the shift pass and one more linearisation per step).  When it is given,
each line also reports the closed-loop effect on a schedule that slides one stage per step (row j of step k is stage k + j of one
ramp): the medians over steps 100.. of the stationarity residual and of max |u_pred - the previous step's u_pred|.
`--sens` asks every step for the sensitivities of u0 (BatchController.step(sens=True): the sensitivity pass in the step kernel) and
reports the fraction of steps that had them; `--sens-w` asks for the sensitivity to the cost weights as well
(BatchController.step(sens_w=True)).  `--terminal` puts a joint-wise LQR terminal cost in force before the loop
(BatchController.set_terminal_cost with robotic_mpc_amd.terminal.lqr_terminal's blocks around each simulation's start posture at
rest): the kernels of mpcb_step_term; with --sens every step also returns du0_dxe.  Not with --sens-w.  `--terminal zero` puts all-zero
blocks in force instead: the same kernels on exactly the plain step's trajectory and solver work (a zero terminal cost is none), which
isolates what the kernels themselves cost; the LQR cost changes the closed loop and with it the QP iterations per step (qp_iter_mean).
`--dist` gives every step an input disturbance for the prediction model (BatchController.step(dist=...): the kernels of mpcb_step_dist,
which linearise again at the start of every step as after a new reference): `--dist zero` all zeros, exactly the plain step's
trajectory, to be held against `--ref packed`, the packed reference rows given again every step (mpcb_step_ref with ref_changed = 1 on
the same trajectory); `--dist random` alternates two draws of +-0.1 rad/s.  Not with --sens, --sens-w or --terminal.

    python scripts/controller_rate.py [--batch 256 ...] [--engine latency|stream ...] [--N 100] [--steps 600] [--solver SQP_RTI]
                                      [--skip-rollout] [--ref none|once|every ...] [--warm carry|shift ...] [--sens] [--sens-w]
                                      [--terminal [lqr|zero]] [--dist [zero|random]]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def raw_configs(batch, N, steps, seed=0, solver="SQP_RTI"):
    """bench.workload_configs's draws as the (unresolved) dicts BatchController takes."""
    import numpy as np

    from robotic_mpc_amd import config

    rng = np.random.default_rng(seed)
    flat = dict(a=0.0, b=0.0, c=0.0, d=0.0, e=0.0, f=0.0)
    return [config.base_params(prediction_horizon=N, simulation_time=0.01 * steps, q_0=config.BASE_PARAMS["q_0"] + rng.uniform(-0.1, 0.1, 6),
                               surface_coeffs=flat, solver_options={"nlp_solver_type": solver}) for _ in range(batch)]


def rk4_plant(wcv, dt):
    """RK4 step of the joint model q' = qdot, qdot' = wcv (u - qdot) on [B, 12] device tensors."""
    import torch

    def f(x, u):
        return torch.cat([x[:, 6:], wcv * (u - x[:, 6:])], 1)

    def step(x, u):
        k1 = f(x, u)
        k2 = f(x + 0.5 * dt * k1, u)
        k3 = f(x + 0.5 * dt * k2, u)
        k4 = f(x + dt * k3, u)
        return x + (dt / 6) * (k1 + 2 * k2 + 2 * k3 + k4)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[256])
    ap.add_argument("--engine", nargs="+", choices=("latency", "stream"), default=["latency"])
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--solver", choices=("SQP_RTI", "SQP"), default="SQP_RTI")
    ap.add_argument("--skip-rollout", action="store_true")
    # task reference: none (the packed one), set once before the loop, or a new one every step (one more linearisation per step)
    ap.add_argument("--ref", nargs="+", choices=("none", "once", "every", "packed"), default=["none"])
    # warm start of every step: the previous iterate as it is, or moved one stage (the shift pass + one more linearisation per step)
    ap.add_argument("--warm", nargs="+", choices=("carry", "shift"), default=None)
    # every step also returns du0_dx / du0_dyref / sens_valid (the sensitivity pass)
    ap.add_argument("--sens", action="store_true")
    # ... and du0_dw (the weight sums inside the sensitivity pass); implies --sens
    ap.add_argument("--sens-w", action="store_true")
    # a joint-wise LQR terminal cost in force (the kernels of mpcb_step_term)
    ap.add_argument("--terminal", nargs="?", const="lqr", default=None, choices=("lqr", "zero"))
    # an input disturbance of the prediction model given every step (the kernels of mpcb_step_dist)
    ap.add_argument("--dist", nargs="?", const="random", default=None, choices=("zero", "random"))
    args = ap.parse_args()
    args.sens = args.sens or args.sens_w
    if args.dist and (args.sens or args.terminal):
        ap.error("--dist is not offered together with --sens, --sens-w or --terminal")
    if args.terminal and args.sens_w:
        ap.error("--sens-w is not offered together with --terminal")
    for B in args.batch:
        for eng in args.engine:
            for ref in args.ref:
                for warm in args.warm or ["carry"]:
                    measure(args, B, eng, ref, warm, sliding=args.warm is not None)


def sliding_medians(ctl, plant, x0, S, shift, lo=100):
    """The closed loop on a schedule that slides one stage per step: medians over steps lo.. (and over the batch) of the
    stationarity residual and of max |u_pred - previous u_pred|."""
    import torch

    base = ctl.default_reference()
    t = torch.arange(ctl.N + S, dtype=torch.float64, device=base.device)
    px = base[:, :1, 3] - 0.01 + 0.0002 * t[None, :]
    vy = base[:, :1, 4] + 0.01 * torch.sin(0.3 * t)[None, :]
    ctl.reset()
    x, prev, res, du = x0, None, [], []
    for k in range(S):
        y = base.clone()
        y[:, :, 3], y[:, :, 4] = px[:, k:k + ctl.N], vy[:, k:k + ctl.N]
        out = ctl.step(x, predict=True, yref=y, shift=shift)
        if k >= lo:
            res.append(out["residuals"][:, 0].clone())
            du.append((out["u_pred"] - prev).abs().amax(dim=(1, 2)))
        prev = out["u_pred"].clone()
        x = plant(x, out["u0"])
    return dict(steps=[lo, S], residual_stat_median=float(torch.stack(res).median()), du_pred_median=float(torch.stack(du).median()))


def measure(args, B, eng, ref="none", warm="carry", sliding=False):
    import numpy as np
    import torch

    import bench
    from robotic_mpc_amd import BatchController, engine
    from robotic_mpc_amd.simulator import chain_for

    S = args.steps
    raw = raw_configs(B, args.N, S, solver=args.solver)
    ctl = BatchController(raw, engine=eng)
    cfgs = ctl.configs
    dev = torch.device("cuda", 0)
    wcv = torch.tensor(np.stack([c["wcv"] for c in cfgs]), dtype=torch.float64, device=dev)
    plant = rk4_plant(wcv, cfgs[0]["dt"])
    x0 = torch.tensor(np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs]), dtype=torch.float64, device=dev)

    # a tracking schedule: a px_ref ramp along the horizon that moves 0.2 mm per step, and a vy_ref profile
    base = ctl.default_reference()
    ramp = torch.arange(ctl.N, dtype=torch.float64, device=dev)
    sched = [base.clone() for _ in range(2)]
    for j, y in enumerate(sched):
        y[:, :, 3] += 0.002 * ramp - 0.01 + 0.0002 * j
        y[:, :, 4] += 0.01 * torch.sin(0.3 * ramp + j)
    if ref == "once":
        ctl.set_reference(sched[0])
    if args.terminal:
        from robotic_mpc_amd import terminal

        x_e = x0.clone()
        x_e[:, 6:] = 0.0
        blocks = terminal.lqr_terminal(raw[0])["blocks"] if args.terminal == "lqr" else np.zeros((6, 3))
        ctl.set_terminal_cost(np.stack([blocks] * B), x_e)

    dsched = None
    if args.dist:
        rng = np.random.default_rng(1)
        dsched = [torch.tensor(rng.uniform(-0.1, 0.1, (B, 6)) if args.dist == "random" else np.zeros((B, 6)), dtype=torch.float64, device=dev)
                  for _ in range(2)]
    packed = base.clone()

    nvalid, nqp = [], []

    def closed_loop(events=None):
        ctl.reset()
        x = x0
        for k in range(S):
            if events is not None:
                events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                events[-1][0].record()
            kw = dict(sens_w=True) if args.sens_w else dict(sens=True) if args.sens else {}
            if warm == "shift":
                kw.update(shift=True)
            if dsched is not None:
                kw.update(dist=dsched[k % 2])
            o = ctl.step(x, yref=sched[k % 2] if ref == "every" else packed if ref == "packed" else None, **kw)
            u = o["u0"]
            if events is not None:
                events[-1][1].record()
                nqp.append(o["qp_iter"].sum())                  # (outside the timed span, like the count below)
                if args.sens:
                    nvalid.append(o["sens_valid"].sum())   # (outside the timed span; the timed loop above has no such launch)
            x = plant(x, u)
        return x

    closed_loop()                                   # warm-up (code objects, allocator)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    xf = closed_loop()
    t1.record()
    torch.cuda.synchronize()
    loop_ms = t0.elapsed_time(t1)
    ev = []
    closed_loop(ev)
    torch.cuda.synchronize()
    step_ms = [a.elapsed_time(b) for a, b in ev]
    out = dict(workload=f"batch {B}, N {args.N}, {args.solver}, {S} steps", engine=eng, reference=ref, warm=warm, sens=bool(args.sens), sens_w=bool(args.sens_w), terminal=args.terminal or False, dist=args.dist or False, step_loop_ms=round(loop_ms, 3),
               step_loop_steps_per_s=round(B * S / (loop_ms * 1e-3)), step_launch_ms_mean=round(float(np.mean(step_ms)), 4),
               step_launch_ms_median=round(float(np.median(step_ms)), 4), step_launch_ms_total=round(float(np.sum(step_ms)), 3),
               launch_info=ctl.launch_info(), kernel_info=ctl.engine.kernel_info(), final_state_finite=bool(torch.isfinite(xf).all()))
    out.update(qp_iter_mean=round(float(torch.stack(nqp).sum()) / (B * S), 4))
    if args.sens:
        out.update(sens_valid_fraction=round(float(torch.stack(nvalid).sum()) / (B * S), 5))
    if sliding and S > 110:
        out.update(sliding_schedule=sliding_medians(ctl, plant, x0, S, warm == "shift"))
    if not args.skip_rollout:
        bc = bench.workload_configs(B, args.N, 0.01 * S, seed=0, solver=args.solver)
        os.environ["MPCB_ENGINE"] = eng                 # the rollout on the same kernel family
        e = engine.MpcBatchEngine(0)
        chain = chain_for(bc[0])
        pb = e.setup(bc, chain)
        bufs = e.alloc_results(pb)
        e.rollout(bufs, 0, S)                       # warm-up
        e.sync()
        ms = []
        for _ in range(3):
            e.setup(bc, chain)
            e.rollout(bufs, 0, S)
            e.sync()
            ms.append(e.kernel_ms())
        out.update(rollout_ms=[round(m, 3) for m in ms], rollout_steps_per_s=round(B * S / (min(ms) * 1e-3)),
                   rollout_launch_info=e.launch_info(), step_over_rollout_kernel_time=round(float(np.sum(step_ms)) / min(ms), 3))
        e.close()
        del os.environ["MPCB_ENGINE"]
    ctl.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
