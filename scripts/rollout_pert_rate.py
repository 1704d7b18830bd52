#!/usr/bin/env python3
"""Device time of the rollout over a perturbed plant (mpcb_rollout_pert), written to profiles/rollout_pert_rate.txt.

Workload and protocol of scripts/rollout_ref_rate.py: BASELINE configs[1]'s draws (controller_rate.raw_configs, seed 0), N = 100, 600
closed-loop steps, the serpentine schedule of 6 lanes; medians of six runs, the variants of a measurement alternating inside one
process.  Batch 256 on the latency engine and batch 4096 on the throughput engine (work queue), SQP_RTI, three variants each:

  scheduled   mpcb_rollout_ref: the yardstick, whose own run-to-run spread is recorded
  nominal     mpcb_rollout_pert with all three arrays given and perturbing nothing (the model's bandwidths, zero tables): the SAME
              closed loop through the new kernels -- the cost of the 30 loads and 18 additions per step, and of the plant step that
              follows the solve instead of running inside its last pass
  perturbed   mpcb_rollout_pert with bandwidths scaled by [0.7, 1.2], Gaussian noise (sigma_q 1e-3, sigma_qdot 1e-2) and a step
              disturbance of 0.05 rad/s from one third of the run on: ANOTHER closed loop (its mean QP iteration count is recorded)

    python scripts/rollout_pert_rate.py [--runs 6] [--steps 600] [--N 100] [--out profiles/rollout_pert_rate.txt]

The resources of the kernels as compiled (VGPRs, AGPRs, LDS, scratch from the .amdhsa_kernel blocks of `hipcc -S --cuda-device-only`
output) are appended from assembly files, no device needed -- of this tree and, for comparison, of the parent commit's:

    python scripts/rollout_pert_rate.py --resources this=DIR parent=DIR [--out ...]      (DIR: the *.s files of the rollout units)
"""
import argparse
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

SCHEDULE = {"kind": "serpentine", "lanes": 6, "lane_pitch": 0.03, "lane_time": 0.6, "turn_time": 0.4}
VARIANTS = ("scheduled", "nominal", "perturbed")


def perturbation(i, steps, dt=0.01):
    import numpy as np

    scale = np.random.default_rng([0, 77, i]).uniform(0.7, 1.2, 6)
    return {"wcv_scale": scale.tolist(), "input_disturbance": {"kind": "step", "start_time": dt * (steps // 3), "value": 0.05},
            "measurement_noise": {"kind": "gaussian", "sigma_q": 1e-3, "sigma_qdot": 1e-2, "seed": i}}


def rollouts(B, eng, args):
    """Device ms of the three variants, `runs` each, alternating; each variant's launch facts and kernel_info."""
    import numpy as np
    import torch

    import controller_rate as cr
    from robotic_mpc_amd import config, engine
    from robotic_mpc_amd.simulator import chain_for

    os.environ["MPCB_ENGINE"] = eng
    raw = cr.raw_configs(B, args.N, args.steps, solver="SQP_RTI")
    sched = [config.resolve_config(dict(r, reference_schedule=SCHEDULE)) for r in raw]
    pert = [config.resolve_config(dict(r, reference_schedule=SCHEDULE, plant_perturbation=perturbation(i, args.steps))) for i, r in enumerate(raw)]
    chain = chain_for(sched[0])
    e = engine.MpcBatchEngine(0)
    pb = e.setup(sched, chain)
    bufs = e.alloc_results(pb)
    y = e.schedule_tensor(sched)
    real = e.perturbation_tensors(pert)
    dev = y.device
    nominal = {"wcv": torch.from_numpy(np.stack([c["wcv"] for c in sched])).to(dev), "u_dist": torch.zeros_like(real["u_dist"]),
               "x_noise": torch.zeros_like(real["x_noise"])}
    ms = {v: [] for v in VARIANTS}
    facts = {}
    for r in range(args.runs + 1):                      # (run 0: warm-up)
        for name, p in (("scheduled", None), ("nominal", nominal), ("perturbed", real)):
            e.setup(sched, chain)
            e.rollout(bufs, 0, pb.Nsim, yref=y, pert=p)
            e.sync()
            if r:
                ms[name].append(e.kernel_ms())
            facts[name] = dict(e.launch_info(), queue_used=e.queue_used(), failures=int((bufs["status"] != 0).sum()),
                               qp_iter_mean=round(float(bufs["qp_iter"].double().mean()), 4), finite=bool(torch.isfinite(bufs["z"]).all()),
                               kernel_info=e.kernel_info())
    e.close()
    del os.environ["MPCB_ENGINE"]
    return ms, facts


def measure(args):
    import numpy as np

    med = lambda v: float(np.median(v))                 # noqa: E731
    fmt = lambda v: " ".join(f"{x:.1f}" for x in v)     # noqa: E731
    lines = ["Rollout over a perturbed plant (mpcb_rollout_pert), one MI355X: device time against mpcb_rollout_ref",
             "=" * 100, "",
             f"scripts/rollout_pert_rate.py --runs {args.runs} --steps {args.steps} --N {args.N}: BASELINE configs[1]'s draws, N = {args.N}, "
             f"{args.steps} closed-loop steps,", f"schedule {SCHEDULE}.  Medians of {args.runs} runs, variants alternating in one process; ms.",
             "nominal: all three arrays given, perturbing nothing (the same closed loop); perturbed: bandwidths x [0.7, 1.2], noise 1e-3 / 1e-2,",
             "a step disturbance of 0.05 rad/s from one third of the run on (another closed loop).  kernel_info: mpcb_kernel_info after the launch",
             "(the plain rollout's kernel after a scheduled launch, the perturbed rollout's after a perturbed one).", ""]
    for B, eng in ((256, "latency"), (4096, "stream")):
        ms, facts = rollouts(B, eng, args)
        s = med(ms["scheduled"])
        spread = (max(ms["scheduled"]) - min(ms["scheduled"])) / s
        per = 1e3 / args.steps
        lines.append(f"batch {B}, {eng} engine, SQP_RTI")
        for v in VARIANTS:
            m = med(ms[v])
            lines += [f"  {v:10s} median {m:9.2f} ms  ({m * per:7.1f} us / step)   runs: {fmt(ms[v])}", f"             {facts[v]}"]
        lines.append(f"  scheduled rollout's own spread (max - min) / median = {spread:.4f}")
        for v in VARIANTS[1:]:
            ratio = med(ms[v]) / s
            lines.append(f"  {v} / scheduled = {ratio:.4f}   ({'inside' if abs(ratio - 1.0) <= spread else 'OUTSIDE'} the spread of 1)")
        lines.append("")
        print("\n".join(lines[-12:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


_KERNELS = re.compile(r"mpc_rollout_kernel|mpc_stream_kernel|mpc_rollout_ref_kernel|mpc_stream_ref_kernel|mpc_rollout_pert_kernel|mpc_stream_pert_kernel")


def kernel_resources(directory):
    """{kernel symbol: (vgprs incl. AGPRs, accum offset, LDS bytes, scratch bytes per lane)} of the rollout kernels in DIR/*.s."""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        text = open(path).read()
        for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, flags=re.S):
            name, body = m.group(1), m.group(2)
            if not _KERNELS.search(name):
                continue
            get = lambda key: int(re.search(rf"\.amdhsa_{key} (\d+)", body).group(1))   # noqa: E731
            out[name] = (get("next_free_vgpr"), get("accum_offset"), get("group_segment_fixed_size"), get("private_segment_fixed_size"))
    return out


def resources(args):
    sets = dict(a.split("=", 1) for a in args.resources)
    this, parent = kernel_resources(sets["this"]), kernel_resources(sets["parent"]) if "parent" in sets else {}
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
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_pert_rate.txt"))
    ap.add_argument("--resources", nargs="+", metavar="NAME=DIR", help="append the compiled kernels' resources from assembly files")
    args = ap.parse_args()
    if args.resources:
        resources(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
