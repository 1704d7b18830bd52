#!/usr/bin/env python3
"""Device time of the rollout with the joint-wise terminal cost (mpcb_rollout_term), and the closed-loop study it exists for, written
to profiles/rollout_term_rate.txt.

Workload and protocol of scripts/rollout_pert_rate.py: BASELINE configs[1]'s draws (controller_rate.raw_configs, seed 0), 600
closed-loop steps, the serpentine schedule of 6 lanes; medians of six runs, the variants of a measurement alternating inside one
process.  N = 100 and N = 20, batch 256 on the latency engine and batch 4096 on the throughput engine (work queue), SQP_RTI:

  (a) pert       mpcb_rollout_pert with nominal perturbation arrays (the model's bandwidths, zero tables): the yardstick, whose own
                 run-to-run spread is recorded.  Its kernels are the parent commit's (the device assembly of mpc_rollout_pert.hip and
                 mpc_stream_rollout_pert.hip is unchanged; --resources prints the comparison).
      zero       mpcb_rollout_term with all-zero blocks over the same arrays: the SAME closed loop through the new kernels -- what the
                 kernels themselves cost
      lqr        mpcb_rollout_term with the lqr(10, 1, 1) blocks of each model and the table x_ref[t] = [q_0; 0] + [0.02 | 0.05]
                 sin(0.4 t): ANOTHER closed loop (its mean QP iteration count is recorded)
  (b) step loop  the BatchController loop that defines the rollout -- set_terminal_cost(blocks, x_ref[:, t]) and step(x, yref = window
                 t) at every step, over a torch RK4 plant: the sum of the device times of the 600 (set + step) launches, against `lqr`
  (c) study      tracking error of N = 20 with an LQR terminal cost around terminal.reference_from_run of the N = 100 run, against
                 plain N = 20 and plain N = 100, per simulation of a batch of 64, through Simulator-level configurations
                 (engine.run_device + mpcb_summary)

    python scripts/rollout_term_rate.py [--runs 6] [--steps 600] [--out profiles/rollout_term_rate.txt]

The resources of the kernels as compiled are appended from assembly files, no device needed:

    python scripts/rollout_term_rate.py --resources this=DIR parent=DIR [--out ...]      (DIR: the *.s files of the rollout units)
"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SCHEDULE = {"kind": "serpentine", "lanes": 6, "lane_pitch": 0.03, "lane_time": 0.6, "turn_time": 0.4}
LQR = {"kind": "lqr", "q_weight": 10.0, "qdot_weight": 1.0, "r_weight": 1.0}
VARIANTS = ("pert", "zero", "lqr")


def table(cfg):
    import numpy as np

    t = np.arange(cfg["Nsim"])[:, None]
    amp = np.array([0.02] * 6 + [0.05] * 6)
    return np.concatenate([cfg["q0"], np.zeros(6)])[None, :] + amp[None, :] * np.sin(0.4 * t)


def inputs(B, N, steps):
    """(raw configurations, resolved with the schedule, resolved with schedule and the lqr terminal cost, the table [B, steps, 12]).
    The configurations carry a constant reference and the table travels as an array: 4096 tables as JSON lists would only cost
    host time."""
    import numpy as np

    import controller_rate as cr
    from robotic_mpc_amd import config

    raw = cr.raw_configs(B, N, steps, solver="SQP_RTI")
    sched = [config.resolve_config(dict(r, reference_schedule=SCHEDULE)) for r in raw]
    term = [config.resolve_config(dict(r, reference_schedule=SCHEDULE,
                                       terminal_cost={"weight": LQR, "reference": {"kind": "constant", "value": table(c)[0].tolist()}}))
            for r, c in zip(raw, sched)]
    return raw, sched, term, np.ascontiguousarray(np.stack([table(c) for c in sched]))


def rollouts(B, eng, N, args):
    """Device ms of the three variants, `runs` each, alternating; each variant's launch facts and kernel_info."""
    import numpy as np
    import torch

    from robotic_mpc_amd import engine
    from robotic_mpc_amd.simulator import chain_for

    os.environ["MPCB_ENGINE"] = eng
    raw, sched, term, xtab = inputs(B, N, args.steps)
    chain = chain_for(sched[0])
    e = engine.MpcBatchEngine(0)
    pb = e.setup(sched, chain)
    bufs = e.alloc_results(pb)
    y = e.schedule_tensor(sched)
    lqr = {"blocks": e.terminal_tensors(term)["blocks"], "x_ref": torch.from_numpy(xtab).to(y.device)}
    zero = {"blocks": torch.zeros_like(lqr["blocks"]), "x_ref": lqr["x_ref"]}
    nominal = {"wcv": torch.from_numpy(np.stack([c["wcv"] for c in sched])).to(y.device),
               "u_dist": torch.zeros((B, pb.Nsim, 6), dtype=torch.float64, device=y.device),
               "x_noise": torch.zeros((B, pb.Nsim, 12), dtype=torch.float64, device=y.device)}
    ms = {v: [] for v in VARIANTS}
    facts = {}
    for r in range(args.runs + 1):                      # (run 0: warm-up)
        for name, t in (("pert", None), ("zero", zero), ("lqr", lqr)):
            e.setup(sched, chain)
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=nominal, term=t)
            e.sync()
            if r:
                ms[name].append(e.kernel_ms())
            facts[name] = dict(e.launch_info(), queue_used=e.queue_used(), failures=int((bufs["status"] != 0).sum()),
                               qp_iter_mean=round(float(bufs["qp_iter"].double().mean()), 4), finite=bool(torch.isfinite(bufs["z"]).all()),
                               kernel_info=e.kernel_info())
    e.close()
    del os.environ["MPCB_ENGINE"]
    return ms, facts, raw, term, xtab


def step_loop(raw, term, xtab, eng, N, args):
    """Sum of the device times of the (set_terminal_cost + step) launches of the BatchController loop, `runs` times."""
    import numpy as np
    import torch

    import controller_rate as cr
    from robotic_mpc_amd import BatchController, reference, terminal

    ctl = BatchController(raw, engine=eng)
    dev = torch.device("cuda", 0)
    y = torch.from_numpy(reference.stack(term)).to(dev)
    b18, _ = terminal.stack(term)
    blocks = torch.from_numpy(np.ascontiguousarray(b18.reshape(len(term), 3, 6).transpose(0, 2, 1))).to(dev)   # [B, 6, 3]
    xr = torch.from_numpy(xtab).to(dev)
    wcv = torch.tensor(np.stack([c["wcv"] for c in term]), dtype=torch.float64, device=dev)
    plant = cr.rk4_plant(wcv, term[0]["dt"])
    x0 = torch.tensor(np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in term]), dtype=torch.float64, device=dev)
    sums = []
    for r in range(args.runs + 1):
        ctl.reset()
        x, ev = x0, []
        for k in range(args.steps):
            w = y[:, k:k + N].contiguous()             # (outside the timed span: the rollout reads its windows and rows in place)
            xe = xr[:, k].contiguous()
            ev.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            ev[-1][0].record()
            ctl.set_terminal_cost(blocks, xe)
            o = ctl.step(x, yref=w)
            ev[-1][1].record()
            x = plant(x, o["u0"])
        torch.cuda.synchronize()
        if r:
            sums.append(float(sum(a.elapsed_time(b) for a, b in ev)))
    ctl.close()
    return sums


def study(args, B=64):
    """(c): weighted tracking RMSE (mpcb_summary) per simulation of plain N = 100, plain N = 20, and N = 20 closed by the LQR terminal
    cost around the N = 100 run's own trajectory."""
    import numpy as np

    import controller_rate as cr
    from robotic_mpc_amd import config, engine, terminal
    from robotic_mpc_amd.engine import SUMMARY_COLS
    from robotic_mpc_amd.simulator import chain_for

    os.environ["MPCB_ENGINE"] = "latency"
    col = SUMMARY_COLS.index("weighted_rmse")
    e = engine.MpcBatchEngine(0)

    def run(cfgs):
        pb, bufs = e.run_device(cfgs, chain_for(cfgs[0]))
        z = bufs["z"].cpu().numpy()
        return e.summary(bufs).cpu().numpy()[:, col], z, int((bufs["status"] != 0).sum()), e.kernel_ms()

    def cfgs(N, tabs=None):
        raw = cr.raw_configs(B, N, args.steps, solver="SQP_RTI")
        return [config.resolve_config(dict(r, reference_schedule=SCHEDULE, **({} if tabs is None else {
            "terminal_cost": {"weight": LQR, "reference": {"kind": "table", "rows": tabs[i].tolist()}}}))) for i, r in enumerate(raw)]

    long_rmse, z, f100, ms100 = run(cfgs(100))
    tabs = [terminal.reference_from_run({"q": z[i, :6], "qdot": z[i, 6:]}, 20) for i in range(B)]
    short_rmse, _, f20, ms20 = run(cfgs(20))
    term_rmse, _, f20t, ms20t = run(cfgs(20, tabs))
    e.close()
    del os.environ["MPCB_ENGINE"]
    q = lambda v: "median %.6f  mean %.6f  max %.6f" % (np.median(v), np.mean(v), np.max(v))   # noqa: E731
    return [f"(c) closed-loop study, {B} simulations, {args.steps} steps, latency engine: weighted tracking RMSE per simulation (mpcb_summary)",
            f"      N = 100 plain                                   {q(long_rmse)}   failures {f100}   {ms100:8.2f} ms",
            f"      N =  20 plain                                   {q(short_rmse)}   failures {f20}   {ms20:8.2f} ms",
            f"      N =  20 + lqr(10, 1, 1) around the N = 100 run  {q(term_rmse)}   failures {f20t}   {ms20t:8.2f} ms",
            f"      simulations where the terminal cost brings N = 20 closer to N = 100 than plain N = 20 is: "
            f"{int((np.abs(term_rmse - long_rmse) < np.abs(short_rmse - long_rmse)).sum())} of {B}",
            f"      median |rmse - rmse(N = 100)|: plain N = 20 {np.median(np.abs(short_rmse - long_rmse)):.6f}, with the terminal cost "
            f"{np.median(np.abs(term_rmse - long_rmse)):.6f}", ""]


def measure(args):
    import numpy as np

    med = lambda v: float(np.median(v))                 # noqa: E731
    fmt = lambda v: " ".join(f"{x:.1f}" for x in v)     # noqa: E731
    lines = ["Rollout with the joint-wise terminal cost (mpcb_rollout_term), one MI355X: device time against mpcb_rollout_pert and the step loop",
             "=" * 100, "",
             f"scripts/rollout_term_rate.py --runs {args.runs} --steps {args.steps}: BASELINE configs[1]'s draws, {args.steps} closed-loop steps,",
             f"schedule {SCHEDULE}.  Medians of {args.runs} runs, variants alternating in one process; ms.",
             "pert: mpcb_rollout_pert, nominal arrays (the parent commit's kernels); zero: mpcb_rollout_term, all-zero blocks (the same closed loop);",
             "lqr: mpcb_rollout_term, lqr(10, 1, 1) blocks and a moving table (another closed loop).  kernel_info: mpcb_kernel_info after the launch.", ""]
    for N in (100, 20):
        for B, eng in ((256, "latency"), (4096, "stream")):
            ms, facts, raw, term, xtab = rollouts(B, eng, N, args)
            loop = step_loop(raw, term, xtab, eng, N, args)
            s = med(ms["pert"])
            spread = (max(ms["pert"]) - min(ms["pert"])) / s
            per = 1e3 / args.steps
            lines.append(f"N = {N}, batch {B}, {eng} engine, SQP_RTI")
            for v in VARIANTS:
                m = med(ms[v])
                lines += [f"  (a) {v:5s} median {m:9.2f} ms  ({m * per:7.1f} us / step)   runs: {fmt(ms[v])}", f"            {facts[v]}"]
            lines.append(f"      pert's own spread (max - min) / median = {spread:.4f}")
            for v in VARIANTS[1:]:
                ratio = med(ms[v]) / s
                lines.append(f"      {v} / pert = {ratio:.4f}   ({'inside' if abs(ratio - 1.0) <= spread else 'OUTSIDE'} the spread of 1)")
            l = med(loop)
            lines += [f"  (b) step loop, set_terminal_cost + step every step: sum of the {args.steps} launch pairs",
                      f"            median {l:9.2f} ms  ({l * per:7.1f} us / step)   runs: {fmt(loop)}",
                      f"      step loop / lqr rollout = {l / med(ms['lqr']):.3f}", ""]
            print("\n".join(lines[-14:]), flush=True)
    lines += study(args)
    print("\n".join(lines[-7:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


def resources(args):
    import rollout_pert_rate as rp

    rp._KERNELS = re.compile(r"mpc_rollout_pert_kernel|mpc_stream_pert_kernel|mpc_rollout_term_kernel|mpc_stream_term_kernel|"
                             r"mpc_step_term_kernel|mpc_stream_step_term_kernel")
    sets = dict(a.split("=", 1) for a in args.resources)
    this, parent = rp.kernel_resources(sets["this"]), rp.kernel_resources(sets["parent"]) if "parent" in sets else {}
    lines = ["", "Kernels as compiled (hipcc -O3 --offload-arch=gfx950 -S --cuda-device-only, .amdhsa_kernel blocks): registers (VGPR + AGPR),",
             "accum offset (= VGPRs), static LDS bytes, scratch bytes per lane -- this commit | the parent commit", ""]
    for name in sorted(this):
        p = parent.get(name)
        same = "" if p is None else ("   same" if p == this[name] else "   DIFFERENT")
        lines.append(f"  {name[:64]:64s} {this[name]} | {p if p is not None else 'new'}{same}")
    lines.append("")
    with open(args.out, "a") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_term_rate.txt"))
    ap.add_argument("--resources", nargs="+", metavar="NAME=DIR", help="append the compiled kernels' resources from assembly files")
    args = ap.parse_args()
    if args.resources:
        resources(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
