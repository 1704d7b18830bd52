"""Scan the gfx950 assembly of the engine's kernels (rollout module mpc_kernel.hip, controller step modules mpc_step.hip and
mpc_stream_step.hip) for a known hipcc 7.2 miscompile and for register spills beyond their recorded budgets.

A lane-divergent loop (`s_andn2_b64 exec ... s_cbranch_execnz`) falls through with an EMPTY exec
mask; hipcc 7.2 sometimes places VGPR<-AGPR spill reloads (`v_accvgpr_read`) in that fall-through
block, before exec is restored, so the reload silently does nothing.  All loop bounds in the
engine are made wave-uniform (Ex::uni) so that such loops do not exist; this script verifies it.

usage: python scripts/check_asm.py            (exit code 1 when the pattern is found)
"""
import os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_kernel.hip")
# the controller step kernels (their own module): scanned like the rollout module, under the same budgets
STEP_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_step.hip")
# the throughput engine's controller step kernel (a module of its own as well): its passes are the rollout's, under HOT_STREAM
STREAM_STEP_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_stream_step.hip")
# the kernels of the rollout against a reference schedule (mpcb_rollout_ref; modules of their own): the rollout kernels with the
# REF passes, under budgets of their own below
ROLLOUT_REF_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_rollout_ref.hip")
STREAM_ROLLOUT_REF_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_stream_rollout_ref.hip")
# the kernels of the rollout over a perturbed plant (mpcb_rollout_pert; modules of their own): the scheduled rollout's with the PERT
# plant step, under budgets of their own below
ROLLOUT_PERT_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_rollout_pert.hip")
STREAM_ROLLOUT_PERT_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_stream_rollout_pert.hip")
# the kernels of the rollout with a terminal cost (mpcb_rollout_term; modules of their own): the perturbed rollout's on the engine
# built with its TERM flag, under budgets of their own below
ROLLOUT_TERM_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_rollout_term.hip")
STREAM_ROLLOUT_TERM_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_stream_rollout_term.hip")
# the kernels of the rollout with an on-device disturbance observer (mpcb_rollout_obs; modules of their own): the perturbed rollout's
# on the engine built with its DIST flag (the estimate in the shared block), under budgets of their own below
ROLLOUT_OBS_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_rollout_obs.hip")
STREAM_ROLLOUT_OBS_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_stream_rollout_obs.hip")
# the kernels of the rollout over a scheduled, stage-varying surface (mpcb_rollout_surf; modules of their own): the perturbed rollout's
# on the engine built with its SURF flag (the stage's coefficients loaded by the lane that linearises it), under budgets of their own
ROLLOUT_SURF_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_rollout_surf.hip")
STREAM_ROLLOUT_SURF_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_stream_rollout_surf.hip")
# the kernels of the rollout with the shift warm start (mpcb_rollout_warm; modules of their own): the perturbed rollout's and the scheduled
# surface's with Engine::shift_pass / se::shift_pass at the top of a step, under budgets of their own below
ROLLOUT_SHIFT_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_rollout_shift.hip")
STREAM_ROLLOUT_SHIFT_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_stream_rollout_shift.hip")
# the kernels of the combined rollout (mpcb_rollout_combined; modules of their own): the perturbed rollout's on the engine built with
# its TERM_TABLE, DIST_SHARED and SURF flags at once, with shift_pass after the observer's publication, under budgets of their own
ROLLOUT_COMBINED_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_rollout_combined.hip")
STREAM_ROLLOUT_COMBINED_SRC = os.path.join(ROOT, "robotic_mpc_amd", "csrc", "mpc_stream_rollout_combined.hip")
SOURCES = (SRC, STEP_SRC, STREAM_STEP_SRC, ROLLOUT_REF_SRC, STREAM_ROLLOUT_REF_SRC, ROLLOUT_PERT_SRC, STREAM_ROLLOUT_PERT_SRC,
           ROLLOUT_TERM_SRC, STREAM_ROLLOUT_TERM_SRC, ROLLOUT_OBS_SRC, STREAM_ROLLOUT_OBS_SRC, ROLLOUT_SURF_SRC,
           STREAM_ROLLOUT_SURF_SRC, ROLLOUT_SHIFT_SRC, STREAM_ROLLOUT_SHIFT_SRC, ROLLOUT_COMBINED_SRC, STREAM_ROLLOUT_COMBINED_SRC)


def scan(asm_text):
    lines = asm_text.split("\n")
    func, hits = None, []
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            func = m.group(1)
        if "s_cbranch_execnz" not in l:
            continue
        for j in range(i + 1, min(i + 80, len(lines))):
            t = lines[j].strip()
            if (t.startswith(".LBB") or t.startswith("s_or_b64 exec") or t.startswith("s_mov_b64 exec")
                    or t.startswith("s_or_saveexec") or "s_branch" in t or "s_cbranch" in t or "s_setpc" in t):
                break
            if t.startswith("v_") and not t.startswith(("v_readlane", "v_readfirstlane", "v_cmp")):
                hits.append((func, i + 1, j + 1, t))
                break
    return hits


# Second check (round 3, widened in round 4): the item-parallel passes keep up to ~100 operands per lane in flight; a build whose
# register budget they exceed (the 8-wavefront and the two-per-CU geometries have 256) spills them to scratch memory, and every
# scratch reload waits with vmcnt(0) for ALL prefetches in flight -- measured: the final forward sweep with 38 scratch operations
# cost 12 us per MPC step (-4 %).  Guarded: the hot passes of EVERY shipped latency kernel (<8,1>, <4,1>, <4,2>; <2,1> and <1,1> are
# test geometries) and the sweeps of the throughput engine, which must hold nothing in scratch beyond a pass's entry / exit
# (MAX_SCRATCH_OPS); and a recorded BUDGET for the functions that do live with scratch -- the once-per-step NLP pass (task_lin holds
# ~130 doubles), the plant log, the SQP merit pass, the kernel bodies (the inlined solver driver: engine object, residual arrays) --
# so that growth there is a decision, not an accident.  Who owns the kernels' scratch bytes (BENCH roofline.scratch_bytes): these.
HOT = ("fwd_resident", "corr_resident", "residual_direct", "fact_pass_t", "fast_rhs", "fast_commit", "forward_step_pass", "corrector_bwd_pass")
HOT_GEOM = ("DevExecILi8ELi1E", "DevExecILi4ELi1E", "DevExecILi4ELi2E")
HOT_STREAM = ("se9fact_pass", "se12forward_pass", "se14corrector_pass", "se13residual_pass", "se14residual_items", "se11fast_commit", "se9rti_items")
MAX_SCRATCH_OPS = 8      # (callee-saved registers at a pass's entry / exit)
# function-name fragment -> scratch operations allowed (the count at the commit that recorded it, + ~10 %)
BUDGET = {
    # (round 4, end: the joint-angle sincos of mpc_kin.h replaced the library's, whose large-argument path was what these functions spilled
    # around: nlp_direct 121 / 147 -> 41 / 54, log_state 43 -> 2, merit_pass 394 -> 186, the throughput engine's lin_pass 56 -> 0 and
    # log_state 33 -> 0 -- those two are held to the hot passes' limit now)
    "DevExecILi8ELi1EEE10nlp_direct": 46, "DevExecILi4ELi2EEE10nlp_direct": 60, "DevExecILi4ELi1EEE10nlp_direct": 8,
    "DevExecILi8ELi1EEE9log_state": 8, "DevExecILi4ELi2EEE9log_state": 8, "DevExecILi4ELi1EEE9log_state": 8,
    "10merit_pass": 210, "se8lin_pass": 8, "se9log_state": 8,
    "18mpc_rollout_kernelILi8ELi1E": 340, "18mpc_rollout_kernelILi4ELi2E": 330, "18mpc_rollout_kernelILi4ELi1E": 258,
    "17mpc_stream_kernelId": 160, "17mpc_stream_kernelIf": 160,
    # the scheduled rollout (recorded: 224 / 293 / 61 for the kernel bodies, 127 for the throughput engine's; its NLP pass against the
    # window, with the plant lane's reference row, 37 / 38 / 2; lin_pass<true> 3)
    "22mpc_rollout_ref_kernelILi8ELi1E": 246, "22mpc_rollout_ref_kernelILi4ELi2E": 322, "22mpc_rollout_ref_kernelILi4ELi1E": 68,
    "21mpc_stream_ref_kernelId": 140,
    "DevExecILi8ELi1EELi0EE10nlp_directILb1ELb1E": 41, "DevExecILi4ELi2EELi0EE10nlp_directILb1ELb1E": 42,
    "DevExecILi4ELi1EELi0EE10nlp_directILb1ELb1E": 8,
    # the perturbed rollout (recorded: 232 / 300 / 61 for the kernel bodies, 140 for the throughput engine's; its NLP pass is the
    # scheduled rollout's, 33 / 36 / 2 here without the plant lane's work)
    "23mpc_rollout_pert_kernelILi8ELi1E": 255, "23mpc_rollout_pert_kernelILi4ELi2E": 330, "23mpc_rollout_pert_kernelILi4ELi1E": 68,
    "22mpc_stream_pert_kernelId": 154,
    # the rollout with a terminal cost (recorded: 228 / 301 / 65 for the kernel bodies, 143 for the throughput engine's; its NLP pass
    # with the stage-N terms of the terminal cost 50 / 49 / 2)
    "23mpc_rollout_term_kernelILi8ELi1E": 251, "23mpc_rollout_term_kernelILi4ELi2E": 331, "23mpc_rollout_term_kernelILi4ELi1E": 72,
    "22mpc_stream_term_kernelId": 157,
    "DevExecILi8ELi1EELi2EE10nlp_directILb1ELb1E": 55, "DevExecILi4ELi2EELi2EE10nlp_directILb1ELb1E": 54,
    "DevExecILi4ELi1EELi2EE10nlp_directILb1ELb1E": 8,
    # the rollout with a disturbance observer (recorded: 265 / 328 / 61 for the kernel bodies -- the observer's gains and estimate
    # live across the step in the six plant lanes -- 164 for the throughput engine's; its NLP pass with the effective input 35 / 36 / 2)
    "22mpc_rollout_obs_kernelILi8ELi1E": 292, "22mpc_rollout_obs_kernelILi4ELi2E": 361, "22mpc_rollout_obs_kernelILi4ELi1E": 68,
    "21mpc_stream_obs_kernelId": 180,
    "DevExecILi8ELi1EELi0ELi2EE10nlp_directILb1ELb1E": 39, "DevExecILi4ELi2EELi0ELi2EE10nlp_directILb1ELb1E": 40,
    "DevExecILi4ELi1EELi0ELi2EE10nlp_directILb1ELb1E": 8,
    # the rollout over a scheduled surface (recorded: 229 / 301 / 63 for the kernel bodies, 144 for the throughput engine's; its NLP
    # pass, with the row's coefficients live across the Jacobian loop, 41 / 40 / 4 against the perturbed rollout's 33 / 36 / 2)
    "23mpc_rollout_surf_kernelILi8ELi1E": 252, "23mpc_rollout_surf_kernelILi4ELi2E": 331, "23mpc_rollout_surf_kernelILi4ELi1E": 70,
    "22mpc_stream_surf_kernelId": 158,
    "DevExecILi8ELi1EELi0ELi0ELi1EE10nlp_directILb1ELb1E": 45, "DevExecILi4ELi2EELi0ELi0ELi1EE10nlp_directILb1ELb1E": 44,
    "DevExecILi4ELi1EELi0ELi0ELi1EE10nlp_directILb1ELb1E": 8,
    # the rollout with the shift warm start (recorded: 235 / 303 / 61 for the kernel bodies without a surface table against the perturbed
    # rollout's 232 / 300 / 61, 232 / 304 / 63 with one against the scheduled surface's 229 / 301 / 63; 149 and 142 for the throughput
    # engine's; the NLP passes are those two rollouts' own)
    "24mpc_rollout_shift_kernelILi8ELi1E": 258, "24mpc_rollout_shift_kernelILi4ELi2E": 333, "24mpc_rollout_shift_kernelILi4ELi1E": 68,
    "29mpc_rollout_shift_surf_kernelILi8ELi1E": 255, "29mpc_rollout_shift_surf_kernelILi4ELi2E": 334, "29mpc_rollout_shift_surf_kernelILi4ELi1E": 70,
    "23mpc_stream_shift_kernelId": 164, "28mpc_stream_shift_surf_kernelId": 158,
    # the combined rollout (recorded: 279 / 347 / 66 for the kernel bodies against the observer rollout's 265 / 328 / 61 -- the terminal
    # pointers, the surface pointer and the observer's registers are live across the step together -- 168 for the throughput engine's
    # against 164; its NLP pass with the terminal terms, the effective input and the row's coefficients 54 / 50 / 2)
    "27mpc_rollout_combined_kernelILi8ELi1E": 307, "27mpc_rollout_combined_kernelILi4ELi2E": 382, "27mpc_rollout_combined_kernelILi4ELi1E": 73,
    "26mpc_stream_combined_kernelId": 185,
    "DevExecILi8ELi1EELi2ELi2ELi1EE10nlp_directILb1ELb1E": 60, "DevExecILi4ELi2EELi2ELi2ELi1EE10nlp_directILb1ELb1E": 55,
    "DevExecILi4ELi1EELi2ELi2ELi1EE10nlp_directILb1ELb1E": 8,
}


# A step kernel is the rollout kernel of its geometry without the plant and the logs: it is held to that kernel's budget.
KERNEL_ALIASES = (("15mpc_step_kernel", "18mpc_rollout_kernel"), ("22mpc_stream_step_kernel", "17mpc_stream_kernelId"))


def scratch_by_function(asm_text):
    out, func = {}, None
    for l in asm_text.split("\n"):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            func = m.group(1)
            out.setdefault(func, 0)
        elif l.startswith(".Lfunc_end"):
            func = None
        elif func and "scratch_" in l:
            out[func] += 1
    return out


def scratch_ops(asm_text):
    """Functions over their limit: {name: (count, limit)}."""
    bad = {}
    for func, n in scratch_by_function(asm_text).items():
        limit = None
        name = func
        for alias, budgeted in KERNEL_ALIASES:
            name = name.replace(alias, budgeted)
        for frag, b in BUDGET.items():
            if frag in name:
                limit = b
        if limit is None:
            hot = (any(h in func for h in HOT) and any(g in func for g in HOT_GEOM)) or any(h in func for h in HOT_STREAM)
            limit = MAX_SCRATCH_OPS if hot else None
        if limit is not None and n > limit:
            bad[func] = (n, limit)
    return bad


def compile_asm(src, d, extra):
    out = os.path.join(d, os.path.basename(src) + ".s")
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--offload-device-only",
                           "-o", out, src] + extra, cwd=d, stderr=subprocess.DEVNULL)
    return open(out).read()


def main():
    hits, spills = [], {}
    from concurrent.futures import ThreadPoolExecutor

    with tempfile.TemporaryDirectory() as d:
        # (the modules are independent: one hipcc each, side by side)
        with ThreadPoolExecutor(max(1, min(len(SOURCES), len(os.sched_getaffinity(0))))) as pool:
            texts = list(pool.map(lambda src: compile_asm(src, d, sys.argv[1:]), SOURCES))
        for text in texts:
            hits += scan(text)
            for f, (n, limit) in scratch_ops(text).items():     # (a pass compiled in several modules: its worst count)
                if f not in spills or n > spills[f][0]:
                    spills[f] = (n, limit)
    for h in hits:
        print("vector op under empty exec after divergent loop: %s line %d -> %d: %s" % h)
    for f, (n, limit) in spills.items():
        print("scratch operations over the limit: %s: %d (limit %d)" % (f, n, limit))
    print("check_asm: %d suspicious site(s), %d function(s) over their scratch limit" % (len(hits), len(spills)))
    return 1 if hits or spills else 0


if __name__ == "__main__":
    sys.exit(main())
