"""Build libmpcbatch.so (HIP, gfx950 only) in-tree with hipcc."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libmpcbatch.so")
LIB_PROF = os.path.join(HERE, "libmpcbatch_prof.so")
ARCH = "gfx950"
# translation units of the library: the rollout kernels + C ABI, the controller step kernels of each engine (modules of their own), and
# their variants with a per-simulation warm start (mpcb_step_warm) and with the sensitivities of u0 (mpcb_step_sens; modules of
# their own again), with the sensitivity of u0 to the cost weights on top of those (mpcb_step_sens_w; again modules of their own), and
# the steps with a joint-wise terminal cost, without and with the sensitivity pass (mpcb_step_term; modules of their own as well),
# and the rollout kernels of each engine that track a task reference schedule (mpcb_rollout_ref; modules of their own too), and those
# of the rollout over a perturbed plant (mpcb_rollout_pert; likewise) and of the rollout with a terminal cost (mpcb_rollout_term),
# and the steps with an input disturbance in the prediction model (mpcb_step_dist), and the rollout kernels whose steps take that
# disturbance from an on-device observer (mpcb_rollout_obs), the steps and rollouts over a scheduled surface (mpcb_step_surf,
# mpcb_rollout_surf), and the rollout kernels with the per-simulation shift warm start (mpcb_rollout_warm), and the step and rollout
# kernels in which terminal cost, disturbance / observer, scheduled surface and shift are live at once (mpcb_step_combined,
# mpcb_rollout_combined)
SOURCES = ("mpc_kernel.hip", "mpc_step.hip", "mpc_stream_step.hip", "mpc_step_warm.hip", "mpc_stream_step_warm.hip",
           "mpc_step_sens.hip", "mpc_stream_step_sens.hip", "mpc_step_sensw.hip", "mpc_stream_step_sensw.hip",
           "mpc_step_term.hip", "mpc_stream_step_term.hip", "mpc_step_term_sens.hip", "mpc_stream_step_term_sens.hip",
           "mpc_rollout_ref.hip", "mpc_stream_rollout_ref.hip", "mpc_rollout_pert.hip", "mpc_stream_rollout_pert.hip",
           "mpc_rollout_term.hip", "mpc_stream_rollout_term.hip", "mpc_step_dist.hip", "mpc_stream_step_dist.hip",
           "mpc_rollout_obs.hip", "mpc_stream_rollout_obs.hip", "mpc_step_surf.hip", "mpc_stream_step_surf.hip",
           "mpc_rollout_surf.hip", "mpc_stream_rollout_surf.hip", "mpc_rollout_shift.hip", "mpc_stream_rollout_shift.hip",
           "mpc_step_combined.hip", "mpc_stream_step_combined.hip", "mpc_rollout_combined.hip", "mpc_stream_rollout_combined.hip")


def _stale(target: str) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    srcs = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(os.path.dirname(HERE), "include", "mpcbatch.h")]
    return any(os.path.getmtime(s) > t for s in srcs)


def _compile(target: str, flags, verbose: bool = False) -> None:
    """One hipcc per translation unit, side by side (the units are independent modules and the largest takes most of the time a
    single command spends on all of them one after the other), then one link.  Objects live in a temporary directory."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    common = [hipcc, f"--offload-arch={ARCH}", "-O3", "-fPIC", "-std=c++17", *flags]
    jobs = max(1, min(len(SOURCES), int(os.environ.get("MAX_JOBS", 0)) or len(os.sched_getaffinity(0))))
    with tempfile.TemporaryDirectory(prefix="mpcb_build_") as d:
        cmds = [common + ["-c", os.path.join(CSRC, f), "-o", os.path.join(d, f + ".o")] for f in SOURCES]
        if verbose:
            print("\n".join(" ".join(c) for c in cmds), file=sys.stderr)
        with ThreadPoolExecutor(jobs) as pool:
            list(pool.map(subprocess.check_call, cmds))
        subprocess.check_call([hipcc, f"--offload-arch={ARCH}", "-fPIC", "-shared", "-o", target + ".tmp", *[c[-1] for c in cmds]])
        os.replace(target + ".tmp", target)


def build(force: bool = False, profile: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 -> robotic_mpc_amd/libmpcbatch.so (cross-compiles without a GPU)."""
    target = LIB_PROF if profile else LIB
    if not force and not _stale(target):
        return target
    flags = (["-DMPCB_PROFILE"] if profile else []) + (["-Rpass-analysis=kernel-resource-usage"] if verbose else [])
    _compile(target, flags, verbose)
    return target


def build_variant(name: str, defines) -> str:
    """Diagnostic builds (scripts/): robotic_mpc_amd/libmpcbatch_<name>.so with extra -D switches, rebuilt when stale."""
    target = os.path.join(HERE, f"libmpcbatch_{name}.so")
    if _stale(target):
        _compile(target, [f"-D{d}" for d in defines])
    return target


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, profile="--profile" in sys.argv, verbose=True))
