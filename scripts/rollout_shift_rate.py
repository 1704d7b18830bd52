#!/usr/bin/env python3
"""Device time of the rollout with the shift warm start (mpcb_rollout_warm), written to profiles/rollout_shift_rate.txt.

Workload and protocol of scripts/rollout_surf_rate.py: BASELINE configs[1]'s draws (controller_rate.raw_configs, seed 0), 600
closed-loop steps, the serpentine schedule of 6 lanes; medians of `runs` runs after one warm-up run, the variants of a measurement
alternating inside one process.  N = 100 and N = 20, batch 256 on the latency engine and batch 4096 on the throughput engine (work
queue), SQP_RTI.  The closed loop: the plant has 0.8 x the model's bandwidths and a step input disturbance of 0.05 rad/s from step 100
on (no measurement noise).

  (a) pert       mpcb_rollout_pert over that plant: the baseline, the parent commit's kernels, whose own run-to-run spread is recorded
      carry      mpcb_rollout_warm with MPCB_WARM_CARRY for every simulation: the SAME closed loop through the new kernels -- what the
                 new instantiation costs when it does nothing
  (b) shift      mpcb_rollout_warm with MPCB_WARM_SHIFT for every simulation, against carry: what the shift pass costs -- about one
                 read and write sweep over the G1 records per step -- on ANOTHER closed loop, whose mean QP iteration count is recorded
  (c) step loop  the BatchController loop the rollout replaces -- step(x, yref = window t, shift = t >= 1) at every step over a torch
                 RK4 plant with the same disturbance: the sum of the device times of the 600 step spans, against `shift`

    python scripts/rollout_shift_rate.py [--runs 6] [--steps 600] [--out profiles/rollout_shift_rate.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SCHEDULE = {"kind": "serpentine", "lanes": 6, "lane_pitch": 0.03, "lane_time": 0.6, "turn_time": 0.4}
WCV_SCALE, D_VALUE, D_START = 0.8, 0.05, 100
VARIANTS = ("pert", "carry", "shift")


def inputs(B, N, steps):
    """(raw configurations, resolved with the reference schedule and the perturbation)."""
    import controller_rate as cr
    from robotic_mpc_amd import config

    raw = cr.raw_configs(B, N, steps, solver="SQP_RTI")
    pert = {"wcv_scale": WCV_SCALE, "input_disturbance": {"kind": "step", "start_time": 0.01 * D_START, "value": D_VALUE}}
    cfgs = [config.resolve_config(dict(r, reference_schedule=SCHEDULE, plant_perturbation=pert)) for r in raw]
    return raw, cfgs


def modes(B, value):
    import torch

    return torch.full((B,), value, dtype=torch.int32, device=torch.device("cuda", 0))


def rollouts(B, eng, N, args):
    """Device ms of the three variants, `runs` each, alternating; each variant's launch facts and kernel_info."""
    import torch

    from robotic_mpc_amd import engine
    from robotic_mpc_amd.simulator import chain_for

    os.environ["MPCB_ENGINE"] = eng
    raw, cfgs = inputs(B, N, args.steps)
    chain = chain_for(cfgs[0])
    e = engine.MpcBatchEngine(0)
    pb = e.setup(cfgs, chain)
    bufs = e.alloc_results(pb)
    y = e.schedule_tensor(cfgs)
    pert = e.perturbation_tensors(cfgs)
    ms = {v: [] for v in VARIANTS}
    facts = {}
    for r in range(args.runs + 1):                      # (run 0: warm-up)
        for name, w in (("pert", None), ("carry", modes(B, engine.WARM_CARRY)), ("shift", modes(B, engine.WARM_SHIFT))):
            e.setup(cfgs, chain)
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pert, warm=w)
            e.sync()
            if r:
                ms[name].append(e.kernel_ms())
            facts[name] = dict(e.launch_info(), queue_used=e.queue_used(), failures=int((bufs["status"] != 0).sum()),
                               qp_iter_mean=round(float(bufs["qp_iter"].double().mean()), 4), finite=bool(torch.isfinite(bufs["z"]).all()),
                               kernel_info=e.kernel_info())
    e.close()
    del os.environ["MPCB_ENGINE"]
    return ms, facts, raw, cfgs


def step_loop(raw, cfgs, eng, N, args):
    """Sum of the device times of the step spans of the BatchController loop with shift from step 1 on, `runs` times."""
    import numpy as np
    import torch

    import controller_rate as cr
    from robotic_mpc_amd import BatchController, reference

    ctl = BatchController(raw, engine=eng)
    dev = torch.device("cuda", 0)
    y = torch.from_numpy(reference.stack(cfgs)).to(dev)
    wcv = torch.tensor(np.stack([c["wcv"] for c in cfgs]), dtype=torch.float64, device=dev)
    plant = cr.rk4_plant(WCV_SCALE * wcv, cfgs[0]["dt"])
    x0 = torch.tensor(np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs]), dtype=torch.float64, device=dev)
    sums = []
    for r in range(args.runs + 1):
        ctl.reset()
        x, ev = x0, []
        for k in range(args.steps):
            w = y[:, k:k + N].contiguous()             # (outside the timed span: the rollout reads its windows in place)
            ev.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            ev[-1][0].record()
            o = ctl.step(x, yref=w, shift=k >= 1)
            ev[-1][1].record()
            u_prev = o["u0"].clone()
            x = plant(x, u_prev + (D_VALUE if k >= D_START else 0.0))
        torch.cuda.synchronize()
        if r:
            sums.append(float(sum(a.elapsed_time(b) for a, b in ev)))
    ctl.close()
    return sums


def measure(args):
    import numpy as np

    med = lambda v: float(np.median(v))                 # noqa: E731
    fmt = lambda v: " ".join(f"{x:.1f}" for x in v)     # noqa: E731
    lines = ["Rollout with the shift warm start (mpcb_rollout_warm), one MI355X: device time against mpcb_rollout_pert and the step loop",
             "=" * 100, "",
             f"scripts/rollout_shift_rate.py --runs {args.runs} --steps {args.steps}: BASELINE configs[1]'s draws, {args.steps} closed-loop steps,",
             f"schedule {SCHEDULE}; plant: {WCV_SCALE} x the model's bandwidths, a step disturbance of {D_VALUE} rad/s from step {D_START} on.",
             f"Medians of {args.runs} runs after one warm-up run, variants alternating in one process; ms.",
             "pert: mpcb_rollout_pert (the parent commit's kernels); carry: mpcb_rollout_warm, every simulation MPCB_WARM_CARRY (the same closed",
             "loop through the new kernels); shift: mpcb_rollout_warm, every simulation MPCB_WARM_SHIFT.  kernel_info: mpcb_kernel_info after the launch.", ""]
    for N in (100, 20):
        for B, eng in ((256, "latency"), (4096, "stream")):
            ms, facts, raw, cfgs = rollouts(B, eng, N, args)
            loop = step_loop(raw, cfgs, eng, N, args)
            s, c, h = med(ms["pert"]), med(ms["carry"]), med(ms["shift"])
            spread = (max(ms["pert"]) - min(ms["pert"])) / s
            per = 1e3 / args.steps
            lines.append(f"N = {N}, batch {B}, {eng} engine, SQP_RTI")
            for v in VARIANTS:
                m = med(ms[v])
                lines += [f"  {v:5s} median {m:9.2f} ms  ({m * per:7.1f} us / step)   runs: {fmt(ms[v])}", f"            {facts[v]}"]
            lines.append(f"      pert's own spread (max - min) / median = {spread:.4f}")
            lines.append(f"  (a) carry / pert  = {c / s:.4f}   ({'inside' if abs(c / s - 1.0) <= spread else 'OUTSIDE'} the spread of 1)")
            lines.append(f"  (b) shift / carry = {h / c:.4f}   share of the shift pass in the shifted rollout (shift - carry) / shift = {(h - c) / h:.4f}"
                         f"   ({(h - c) * per:.2f} us / step; qp_iter mean {facts['carry']['qp_iter_mean']} -> {facts['shift']['qp_iter_mean']})")
            l = med(loop)
            lines += [f"  (c) step loop, step(yref = window, shift = t >= 1) every step: sum of the {args.steps} spans",
                      f"            median {l:9.2f} ms  ({l * per:7.1f} us / step)   runs: {fmt(loop)}",
                      f"      step loop / shift rollout = {l / h:.3f}", ""]
            print("\n".join(lines[-15:]), flush=True)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "w") as f:                  # (kept up to date: a later case that fails leaves the earlier ones)
                f.write("\n".join(lines) + "\n")


def geometries(args):
    """mpcb_kernel_info of the perturbed rollout's and this rollout's kernel at every geometry (one tiny launch each), appended."""
    import torch

    from robotic_mpc_amd import engine
    from robotic_mpc_amd.simulator import chain_for

    lines = ["", "mpcb_kernel_info at every geometry (4 simulations, N = 12, 4 steps): the perturbed rollout's kernel | this rollout's", ""]
    for name, env in (("latency <8,1>", dict(MPCB_ENGINE="latency", MPCB_WAVES_PER_SIM="8")), ("latency <4,1>", dict(MPCB_ENGINE="latency", MPCB_WAVES_PER_SIM="4")),
                      ("latency <4,2>", dict(MPCB_ENGINE="latency", MPCB_WAVES_PER_SIM="4", MPCB_WPE="2")),
                      ("latency <2,1>", dict(MPCB_ENGINE="latency", MPCB_WAVES_PER_SIM="2")), ("latency <1,1>", dict(MPCB_ENGINE="latency", MPCB_WAVES_PER_SIM="1")),
                      ("stream", dict(MPCB_ENGINE="stream"))):
        os.environ.update(env)
        raw, cfgs = inputs(4, 12, 4)
        chain = chain_for(cfgs[0])
        e = engine.MpcBatchEngine(0)
        pb = e.setup(cfgs, chain)
        bufs = e.alloc_results(pb)
        y, pert = e.schedule_tensor(cfgs), e.perturbation_tensors(cfgs)
        info = []
        for w in (None, modes(4, engine.WARM_SHIFT)):
            e.setup(cfgs, chain)
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=pert, warm=w)
            e.sync()
            info.append(e.kernel_info())
        lines.append(f"  {name:14s} {e.launch_info()}  {info[0]} | {info[1]}")
        e.close()
        for k in env:
            del os.environ[k]
        torch.cuda.synchronize()
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_shift_rate.txt"))
    ap.add_argument("--geometries", action="store_true", help="append mpcb_kernel_info at every geometry to the file instead of measuring")
    args = ap.parse_args()
    if args.geometries:
        geometries(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
