#!/usr/bin/env python3
"""What the shift warm start does to the closed loop, in emulation (no GPU), written to profiles/rollout_shift_closed_loop.txt.

Part 1: the loop that defines the rollout -- the emulated latency-engine step with a warm-start mode (tests/emu/emu_warm.Controller)
over the perturbed plant, tests/emu/emu_rollshift.step_loop -- on the configurations of tests/test_emulation_rollout_pert.py::_cfgs
(serpentine reference, perturbed plant, two simulations, SQP_RTI), once with CARRY everywhere and once with SHIFT from step 1 on.
Part 2: the emulated rollouts themselves (emu_rollshift.rollout, the code behind mpcb_rollout_warm), carry against shift: the weighted
RMSE of the five task errors of the logged columns, on the serpentine schedule and on a moving surface, at N = 12 and N = 20.

    python scripts/rollout_shift_closed_loop.py [--out profiles/rollout_shift_closed_loop.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))

CARRY, SHIFT = 0, 2
VELOCITY = [0.05, -0.05, 0.02]          # of the moving surface, m/s
STEPS2 = 40                             # steps of the rollouts of part 2


def part1(chain):
    import emu_rollshift
    import test_emulation_rollout_pert as tp
    from robotic_mpc_amd import plant, reference

    rows = []
    for N, steps in ((12, 14), (20, 7), (2, 10), (1, 10)):
        cfgs = tp._cfgs(N, steps, "SQP_RTI", True)
        sched, pert = reference.stack(cfgs), plant.stack(cfgs)
        a = emu_rollshift.step_loop(cfgs, chain, sched, pert, CARRY, waves=4)
        b = emu_rollshift.step_loop(cfgs, chain, sched, pert, SHIFT, waves=4)
        assert (a["status"] == 0).all() and (b["status"] == 0).all()
        dz = [float(np.abs(a["z"][i] - b["z"][i]).max()) for i in range(2)]
        ra, rb = float(a["residuals"][:, 1:, 0].mean()), float(b["residuals"][:, 1:, 0].mean())
        rows.append(f"    {N:4d} {steps:6d}    {dz[0]:.1e} / {dz[1]:.1e}    {ra:.5f} -> {rb:.5f}"
                    f"    max |d residuals| {float(np.abs(a['residuals'] - b['residuals']).max()):.1e}")
        print(rows[-1], flush=True)
    return rows


def weighted_rmse(errors, dt=0.01):
    """analysis.compute_metrics' weighted RMSE of one simulation's [7, T1] error log (rows e1 .. e5)."""
    from robotic_mpc_amd import analysis

    return analysis.compute_metrics({k: errors[j] for j, k in enumerate(analysis.ERROR_ROWS)}, dt)["weighted_rmse"]


def part2(chain):
    import emu_rollshift
    import test_emulation_rollout_pert as tp
    from robotic_mpc_amd import config, plant, reference, surface

    rows = []
    for N in (12, 20):
        for name, extra in (("serpentine schedule", {}), ("serpentine schedule, moving surface", {"surface_schedule": {"kind": "moving", "velocity": VELOCITY}})):
            q0 = np.asarray(config.BASE_PARAMS["q_0"]) + np.array([0.05, -0.04, 0.03, 0.02, -0.03, 0.04])
            pa, pb = tp._pert(STEPS2)
            kw = dict(prediction_horizon=N, simulation_time=0.01 * STEPS2 + 1e-9, solver_options={"nlp_solver_type": "SQP_RTI"},
                      reference_schedule=tp.SERPENTINE, **extra)
            cfgs = [config.resolve_config(config.base_params(**kw, q_0=q0, plant_perturbation=pa)),
                    config.resolve_config(config.base_params(**kw, q_0=q0, w_u=0.002, px_ref=0.38, plant_perturbation=pb))]
            sched, pert = reference.stack(cfgs), plant.stack(cfgs)
            surf = surface.stack(cfgs) if extra else None
            a = emu_rollshift.rollout(cfgs, chain, sched, CARRY, surf=surf, **pert, waves=4)
            b = emu_rollshift.rollout(cfgs, chain, sched, SHIFT, surf=surf, **pert, waves=4)
            assert (a["status"] == 0).all() and (b["status"] == 0).all()
            wa, wb = [weighted_rmse(a["errors"][i]) for i in range(2)], [weighted_rmse(b["errors"][i]) for i in range(2)]
            rows.append(f"    N = {N:3d}, {STEPS2} steps, {name:38s} carry {wa[0]:.6f} / {wa[1]:.6f}   shift {wb[0]:.6f} / {wb[1]:.6f}"
                        f"   shift / carry {wb[0] / wa[0]:.4f} / {wb[1] / wa[1]:.4f}")
            print(rows[-1], flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_shift_closed_loop.txt"))
    args = ap.parse_args()
    from robotic_mpc_amd import robots

    chain = robots.builtin_chain("ur10")
    lines = ["Closed loop of the rollout with the shift warm start (mpcb_rollout_warm), in emulation", "=" * 100, "",
             "scripts/rollout_shift_closed_loop.py (host emulation of the latency engine at 4 wavefronts; no GPU).", "",
             "1. The loop that defines the rollout: emu_warm.Controller.step(z_t + noise_t, yref = window t, ref_changed, warm) over the perturbed",
             "   plant, configurations of tests/test_emulation_rollout_pert.py::_cfgs (serpentine reference, perturbed plant, two simulations,",
             "   SQP_RTI), warm = CARRY everywhere against SHIFT from step 1 on.  Every step of every loop has status 0.", "",
             "       N  steps    max |dz| between the loops    mean stationarity residual after the step, steps >= 1 (carry -> shift)"]
    lines += part1(chain)
    lines += ["", "2. The emulated rollouts (the code behind mpcb_rollout_warm), every simulation CARRY against every simulation SHIFT: weighted RMSE",
              "   of the five task errors over the logged columns (analysis.compute_metrics), simulation 0 / simulation 1; the plant of part 1",
              f"   with its disturbance from step {STEPS2 // 3} on; the moving surface translates at {VELOCITY} m/s.  Every step has status 0.", ""]
    lines += part2(chain)
    lines += ["", "The shifted iterate is linearised where the previous step left the solution of the same table rows, so the step's stationarity",
              "residual falls (part 1); the closed-loop tracking error, which the plant mismatch, the disturbance and the noise dominate, moves",
              "by what part 2 shows.  With N = 1 the shift moves nothing that reaches u0 and the loops coincide."]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
