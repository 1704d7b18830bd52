#!/usr/bin/env python3
"""Device time of the combined rollout (mpcb_rollout_combined), written to profiles/rollout_combined_rate.txt.

Workload and protocol of scripts/rollout_shift_rate.py: BASELINE configs[1]'s draws (controller_rate.raw_configs, seed 0), 600
closed-loop steps, the serpentine schedule of 6 lanes; medians of `runs` runs after one warm-up run, the variants of a measurement
alternating inside one process.  N = 100 and N = 20, batch 256 on the latency engine and batch 4096 on the throughput engine (work
queue), SQP_RTI.  The closed loop: the plant has 0.8 x the model's bandwidths and a step input disturbance of 0.05 rad/s from step 100
on (no measurement noise).  The features: an LQR terminal cost (q 10, qdot 1, r 1) around [q_0; 0], an observer with pole 0.2, a
surface moving at 0.05 m/s along x, the shift warm start.

  (a) pert / neutral      mpcb_rollout_pert against mpcb_rollout_combined with all four neutral: the SAME closed loop through the new
                          kernels -- what the all-on instantiation costs when it does nothing
  (b) F / combined F      each feature's own kernel (mpcb_rollout_term, _obs, _surf, _warm) against the combined kernel with that ONE
                          feature live and the other three neutral: the same closed loop again
  (c) all / step loop     all four live, against the BatchController(combined=True) loop it replaces -- set_terminal_cost, the torch
                          observer and step(x, yref, surface, dist, shift = t >= 1) at every step over a torch RK4 plant with the same
                          disturbance: the sum of the device times of the 600 step spans

The comparison kernels are the ones the parent commit has: their translation units compile to the same device code here.

    python scripts/rollout_combined_rate.py [--runs 4] [--steps 600] [--out profiles/rollout_combined_rate.txt]
    python scripts/rollout_combined_rate.py --geometries      (appends mpcb_kernel_info at every geometry to the file)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SCHEDULE = {"kind": "serpentine", "lanes": 6, "lane_pitch": 0.03, "lane_time": 0.6, "turn_time": 0.4}
WCV_SCALE, D_VALUE, D_START, POLE, VEL = 0.8, 0.05, 100, 0.2, [0.05, 0.0, 0.0]
FEATURES = ("term", "obs", "surf", "shift")


def inputs(B, N, steps, live=FEATURES):
    """(raw configurations, resolved with the schedule, the perturbation and the features of `live`, combine_features on)."""
    import controller_rate as cr
    from robotic_mpc_amd import config

    raw = cr.raw_configs(B, N, steps, solver="SQP_RTI")
    pert = {"wcv_scale": WCV_SCALE, "input_disturbance": {"kind": "step", "start_time": 0.01 * D_START, "value": D_VALUE}}
    cfgs = []
    for r in raw:
        kw = dict(reference_schedule=SCHEDULE, plant_perturbation=pert, combine_features=True)
        if "term" in live:
            kw["terminal_cost"] = {"weight": {"kind": "lqr", "q_weight": 10.0, "qdot_weight": 1.0, "r_weight": 1.0},
                                   "reference": {"kind": "constant", "value": list(r["q_0"]) + [0.0] * 6}}
        if "obs" in live:
            kw["disturbance_observer"] = {"pole": POLE}
        if "surf" in live:
            kw["surface_schedule"] = {"kind": "moving", "velocity": VEL}
        if "shift" in live:
            kw["warm_start"] = "shift"
        cfgs.append(config.resolve_config(dict(r, **kw)))
    return raw, cfgs


def variants(e, B, N, steps):
    """name -> keyword arguments of MpcBatchEngine.rollout.  `F`: feature F's own kernels; `cF`: the combined kernels with F alone
    live; `pert` / `neutral`; `all`.  Two sets of tables are sampled -- all four live, all four neutral (engine.combined_arrays) -- and
    the one-feature sets take that feature's tables from the first and the rest from the second; the device tensors are shared."""
    import numpy as np
    import torch

    from robotic_mpc_amd import engine

    dev = torch.device("cuda", e.device)
    put = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)   # noqa: E731
    live, off = engine.combined_arrays(inputs(B, N, steps)[1]), engine.combined_arrays(inputs(B, N, steps, live=())[1])
    d_hat = torch.zeros((B, steps, 6), dtype=torch.float64, device=dev)

    def dev_set(a):
        return {"yref": put(a["yref"]), "pert": {k: put(v) for k, v in a["pert"].items()}, "term": {k: put(v) for k, v in a["term"].items()},
                "obs": {"gain": put(a["gain"]), "d_hat": d_hat}, "surf": put(a["surf"]), "warm": put(a["warm"])}

    t_live, t_off = dev_set(live), dev_set(off)
    key = {"term": "term", "obs": "obs", "surf": "surf", "shift": "warm"}
    out = {"pert": dict(yref=t_off["yref"], pert=t_off["pert"]), "neutral": dict(combined=True, **t_off)}
    for f in FEATURES:
        out[f] = dict(yref=t_off["yref"], pert=t_off["pert"], **{key[f]: t_live[key[f]]})
        out["c" + f] = dict(combined=True, **{**t_off, key[f]: t_live[key[f]]})
    out["all"] = dict(combined=True, **t_live)
    return out


def rollouts(B, eng, N, args):
    """Device ms of every variant, `runs` each, alternating; each variant's launch facts and kernel_info."""
    import torch

    from robotic_mpc_amd import engine
    from robotic_mpc_amd.simulator import chain_for

    os.environ["MPCB_ENGINE"] = eng
    raw, cfgs = inputs(B, N, args.steps)
    chain = chain_for(cfgs[0])
    e = engine.MpcBatchEngine(0)
    pb = e.setup(cfgs, chain)
    bufs = e.alloc_results(pb)
    var = variants(e, B, N, args.steps)
    ms = {v: [] for v in var}
    facts = {}
    for r in range(args.runs + 1):                      # (run 0: warm-up)
        for name, kw in var.items():
            e.setup(cfgs, chain)
            e.rollout(bufs, 0, pb.Nsim, **kw)
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
    """Sum of the device times of the step spans of the BatchController(combined=True) loop with all four live, `runs` times."""
    import numpy as np
    import torch

    import controller_rate as cr
    from robotic_mpc_amd import BatchController, engine
    from robotic_mpc_amd.observer import DisturbanceObserver

    ctl = BatchController(raw, engine=eng, combined=True)
    dev = torch.device("cuda", 0)
    a = engine.combined_arrays(cfgs)
    put = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)   # noqa: E731
    y, surf, xref = put(a["yref"]), put(a["surf"]), put(a["term"]["x_ref"])
    blocks = put(a["term"]["blocks"].reshape(len(cfgs), 3, 6).transpose(0, 2, 1))
    wcv = torch.tensor(np.stack([c["wcv"] for c in cfgs]), dtype=torch.float64, device=dev)
    plant = cr.rk4_plant(WCV_SCALE * wcv, cfgs[0]["dt"])
    x0 = torch.tensor(np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs]), dtype=torch.float64, device=dev)
    sums = []
    for r in range(args.runs + 1):
        ctl.reset()
        obs = DisturbanceObserver(wcv, cfgs[0]["dt"], pole=POLE)
        x, ev = x0, []
        u_prev = torch.zeros((len(cfgs), 6), dtype=torch.float64, device=dev)
        for k in range(args.steps):
            w, sw = y[:, k:k + N].contiguous(), surf[:, k:k + N].contiguous()   # (outside the timed span: the rollout reads in place)
            d = obs.update(x, u_prev)
            ctl.set_terminal_cost(blocks, xref[:, k].contiguous())
            ev.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
            ev[-1][0].record()
            o = ctl.step(x, yref=w, surface=sw, dist=d, shift=k >= 1)
            ev[-1][1].record()
            u_prev = o["u0"].clone()
            x = plant(x, u_prev + (D_VALUE if k >= D_START else 0.0))
        torch.cuda.synchronize()
        if r:
            sums.append(float(sum(p.elapsed_time(q) for p, q in ev)))
    ctl.close()
    return sums


def measure(args):
    import numpy as np

    med = lambda v: float(np.median(v))                 # noqa: E731
    fmt = lambda v: " ".join(f"{x:.1f}" for x in v)     # noqa: E731
    lines = ["Combined rollout (mpcb_rollout_combined), one MI355X: device time against the single-feature rollouts and the step loop",
             "=" * 100, "",
             f"scripts/rollout_combined_rate.py --runs {args.runs} --steps {args.steps}: BASELINE configs[1]'s draws, {args.steps} closed-loop steps,",
             f"schedule {SCHEDULE}; plant: {WCV_SCALE} x the model's bandwidths, a step disturbance of {D_VALUE} rad/s from step {D_START} on.",
             f"Features: LQR terminal cost (q 10, qdot 1, r 1) around [q_0; 0]; observer pole {POLE}; surface moving at {VEL} m/s; shift.",
             f"Medians of {args.runs} runs after one warm-up run, variants alternating in one process; ms.",
             "pert: mpcb_rollout_pert; neutral: mpcb_rollout_combined, all four neutral; term / obs / surf / shift: mpcb_rollout_term / _obs /",
             "_surf / _warm; cterm / cobs / csurf / cshift: mpcb_rollout_combined with that one feature live; all: all four live.",
             "kernel_info: mpcb_kernel_info after the launch.", ""]
    for N in (100, 20):
        for B, eng in ((256, "latency"), (4096, "stream")):
            ms, facts, raw, cfgs = rollouts(B, eng, N, args)
            loop = step_loop(raw, cfgs, eng, N, args)
            per = 1e3 / args.steps
            m = {v: med(ms[v]) for v in ms}
            spread = (max(ms["pert"]) - min(ms["pert"])) / m["pert"]
            lines.append(f"N = {N}, batch {B}, {eng} engine, SQP_RTI")
            for v in ms:
                lines += [f"  {v:7s} median {m[v]:9.2f} ms  ({m[v] * per:7.1f} us / step)   runs: {fmt(ms[v])}", f"            {facts[v]}"]
            lines.append(f"      pert's own spread (max - min) / median = {spread:.4f}")
            lines.append(f"  (a) neutral / pert = {m['neutral'] / m['pert']:.4f}")
            lines.append("  (b) " + "   ".join(f"c{f} / {f} = {m['c' + f] / m[f]:.4f}" for f in FEATURES))
            l = med(loop)
            lines += [f"  (c) step loop, set_terminal_cost + observer + step(yref, surface, dist, shift = t >= 1) every step: sum of the {args.steps} spans",
                      f"            median {l:9.2f} ms  ({l * per:7.1f} us / step)   runs: {fmt(loop)}",
                      f"      all / pert = {m['all'] / m['pert']:.4f}   step loop / all = {l / m['all']:.3f}", ""]
            print("\n".join(lines[-(2 * len(ms) + 9):]), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:                  # (kept up to date: a later case that fails leaves the earlier ones)
                f.write("\n".join(lines) + "\n")


def geometries(args):
    """mpcb_kernel_info of the four single-feature rollouts' kernels and of this rollout's at every geometry (one tiny launch each)."""
    import torch

    from robotic_mpc_amd import engine
    from robotic_mpc_amd.simulator import chain_for

    lines = ["", "mpcb_kernel_info at every geometry (4 simulations, N = 12, 4 steps): vgprs / lds_bytes / scratch_bytes of the kernels of",
             "mpcb_rollout_term | _obs | _surf | _warm | _combined", ""]
    for name, env in (("latency <8,1>", dict(MPCB_ENGINE="latency", MPCB_WAVES_PER_SIM="8")), ("latency <4,1>", dict(MPCB_ENGINE="latency", MPCB_WAVES_PER_SIM="4")),
                      ("latency <4,2>", dict(MPCB_ENGINE="latency", MPCB_WAVES_PER_SIM="4", MPCB_WPE="2")),
                      ("latency <2,1>", dict(MPCB_ENGINE="latency", MPCB_WAVES_PER_SIM="2")), ("latency <1,1>", dict(MPCB_ENGINE="latency", MPCB_WAVES_PER_SIM="1")),
                      ("stream", dict(MPCB_ENGINE="stream"))):
        os.environ.update(env)
        _, cfgs = inputs(4, 12, 4)
        chain = chain_for(cfgs[0])
        e = engine.MpcBatchEngine(0)
        pb = e.setup(cfgs, chain)
        bufs = e.alloc_results(pb)
        var = variants(e, 4, 12, 4)
        info = []
        for v in FEATURES + ("all",):
            e.setup(cfgs, chain)
            e.rollout(bufs, 0, pb.Nsim, **var[v])
            e.sync()
            k = e.kernel_info()
            info.append(f"{k['vgprs']} / {k['lds_bytes']} / {k['scratch_bytes']}")
        lines.append(f"  {name:14s} {e.launch_info()}  " + " | ".join(info))
        e.close()
        for k in env:
            del os.environ[k]
        torch.cuda.synchronize()
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_combined_rate.txt"))
    ap.add_argument("--geometries", action="store_true", help="append mpcb_kernel_info at every geometry to the file instead of measuring")
    args = ap.parse_args()
    if args.geometries:
        geometries(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
