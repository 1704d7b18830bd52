// mpc_launch.h -- host side of the kernel variants.  Every variant of the controller step and of the rollout is a translation unit of
// its own (mpc_step.hip says why) that defines its kernel and ONE getter, declared here; mpc_kernel.hip launches whatever the getter
// returns.  The getter's return type is the kernel's signature, so a unit whose kernel takes other arguments does not compile.
#pragma once
#include <hip/hip_runtime.h>

#include "mpc_layout.h"

namespace mpcb {

// latency engine (mpc_core.h): (pb, rb, params, ws_base, ws_stride, <the call's own arguments>, pool_doubles, <the variant's tables>)
using StepFn = void (*)(Problem, Robot, const InstParams *, double *, size_t, StepIO, int, int);
using RolloutFn = void (*)(Problem, Robot, const InstParams *, double *, size_t, Outputs, int, int, int);
using RolloutRefFn = void (*)(Problem, Robot, const InstParams *, double *, size_t, Outputs, int, int, int, const double *);
using RolloutPertFn = void (*)(Problem, Robot, const InstParams *, double *, size_t, Outputs, int, int, int, const double *, PlantPert);
using RolloutTermFn = void (*)(Problem, Robot, const InstParams *, double *, size_t, Outputs, int, int, int, const double *, PlantPert,
                               TermTab);
using RolloutObsFn = void (*)(Problem, Robot, const InstParams *, double *, size_t, Outputs, int, int, int, const double *, PlantPert,
                              ObsArg);
using RolloutSurfFn = void (*)(Problem, Robot, const InstParams *, double *, size_t, Outputs, int, int, int, const double *, PlantPert,
                               const double *);
using RolloutShiftFn = void (*)(Problem, Robot, const InstParams *, double *, size_t, Outputs, int, int, int, const double *, PlantPert,
                                const double *, const int *);
using RolloutCombinedFn = void (*)(Problem, Robot, const InstParams *, double *, size_t, Outputs, int, int, int, const double *, PlantPert,
                                   TermTab, ObsArg, const double *, const int *);
// throughput engine (mpc_stream.h): the robot record in device memory, no pool; rollouts take (queue, chunk_steps, timeout_ticks)
using StreamStepFn = void (*)(Problem, const Robot *, const InstParams *, double *, size_t, StepIO, int);
using StreamRolloutFn = void (*)(Problem, const Robot *, const InstParams *, double *, size_t, Outputs, int, int, int *, int, long long);
using StreamRolloutRefFn = void (*)(Problem, const Robot *, const InstParams *, double *, size_t, Outputs, int, int, int *, int, long long,
                                    const double *);
using StreamRolloutPertFn = void (*)(Problem, const Robot *, const InstParams *, double *, size_t, Outputs, int, int, int *, int, long long,
                                     const double *, PlantPert);
using StreamRolloutTermFn = void (*)(Problem, const Robot *, const InstParams *, double *, size_t, Outputs, int, int, int *, int, long long,
                                     const double *, PlantPert, TermTab);
using StreamRolloutObsFn = void (*)(Problem, const Robot *, const InstParams *, double *, size_t, Outputs, int, int, int *, int, long long,
                                    const double *, PlantPert, ObsArg);
using StreamRolloutSurfFn = void (*)(Problem, const Robot *, const InstParams *, double *, size_t, Outputs, int, int, int *, int, long long,
                                     const double *, PlantPert, const double *);
using StreamRolloutShiftFn = void (*)(Problem, const Robot *, const InstParams *, double *, size_t, Outputs, int, int, int *, int, long long,
                                      const double *, PlantPert, const double *, const int *);
using StreamRolloutCombinedFn = void (*)(Problem, const Robot *, const InstParams *, double *, size_t, Outputs, int, int, int *, int, long long,
                                         const double *, PlantPert, TermTab, ObsArg, const double *, const int *);

// The kernel of the latency engine's template K<NWV, WPE = 1> for a launch geometry (mpcb_setup picks it; <2> and <1> are reached
// through MPCB_WAVES_PER_SIM), as a pointer of type Fn.  The module holds its kernels in the order they are instantiated in, which is
// the order of the arms (each cast names its kernel where it stands; uncast, the innermost conditional would come first): keep it.
#define MPCB_GEOMETRY_KERNEL(Fn, K, waves_per_sim, wpe)                                                                     \
    ((waves_per_sim) == 8   ? static_cast<Fn>(K<8>)                                                                         \
     : (waves_per_sim) == 4 ? ((wpe) == 2 ? static_cast<Fn>(K<4, 2>) : static_cast<Fn>(K<4>))                               \
     : (waves_per_sim) == 2 ? static_cast<Fn>(K<2>)                                                                         \
                            : static_cast<Fn>(K<1>))

// mpc_step*.hip / mpc_stream_step*.hip: mpcb_step, _warm, _sens, _sens_w, _term without and with the sensitivity pass, _dist, _surf
StepFn step_kernel(int waves_per_sim, int wpe);
StepFn step_warm_kernel(int waves_per_sim, int wpe);
StepFn step_sens_kernel(int waves_per_sim, int wpe);
StepFn step_sensw_kernel(int waves_per_sim, int wpe);
StepFn step_term_kernel(int waves_per_sim, int wpe);
StepFn step_term_sens_kernel(int waves_per_sim, int wpe);
StepFn step_dist_kernel(int waves_per_sim, int wpe);
StepFn step_surf_kernel(int waves_per_sim, int wpe);
StreamStepFn stream_step_kernel();
StreamStepFn stream_step_warm_kernel();
StreamStepFn stream_step_sens_kernel();
StreamStepFn stream_step_sensw_kernel();
StreamStepFn stream_step_term_kernel();
StreamStepFn stream_step_term_sens_kernel();
StreamStepFn stream_step_dist_kernel();
StreamStepFn stream_step_surf_kernel();
// mpc_rollout_*.hip / mpc_stream_rollout_*.hip: mpcb_rollout_ref, _pert, _term, _obs, _surf (the kernels of mpcb_rollout are mpc_kernel.hip's own)
RolloutRefFn rollout_ref_kernel(int waves_per_sim, int wpe);
RolloutPertFn rollout_pert_kernel(int waves_per_sim, int wpe);
RolloutTermFn rollout_term_kernel(int waves_per_sim, int wpe);
RolloutObsFn rollout_obs_kernel(int waves_per_sim, int wpe);
RolloutSurfFn rollout_surf_kernel(int waves_per_sim, int wpe);
StreamRolloutRefFn stream_rollout_ref_kernel();
StreamRolloutPertFn stream_rollout_pert_kernel();
StreamRolloutTermFn stream_rollout_term_kernel();
StreamRolloutObsFn stream_rollout_obs_kernel();
StreamRolloutSurfFn stream_rollout_surf_kernel();
// mpc_rollout_shift.hip / mpc_stream_rollout_shift.hip: mpcb_rollout_warm, without (`surf` false) and with a surface table
RolloutShiftFn rollout_shift_kernel(int waves_per_sim, int wpe, bool surf);
StreamRolloutShiftFn stream_rollout_shift_kernel(bool surf);
// mpc_step_combined.hip / mpc_stream_step_combined.hip, mpc_rollout_combined.hip / mpc_stream_rollout_combined.hip: mpcb_step_combined
// and mpcb_rollout_combined, all four features in one instantiation; neutral_surf_fill (mpc_rollout_combined.hip) writes the neutral
// surface table [batch][rows][NSURF], every row of simulation i = InstParams::coeffs of i, on stream s
StepFn step_combined_kernel(int waves_per_sim, int wpe);
StreamStepFn stream_step_combined_kernel();
RolloutCombinedFn rollout_combined_kernel(int waves_per_sim, int wpe);
StreamRolloutCombinedFn stream_rollout_combined_kernel();
void neutral_surf_fill(int batch, size_t rows, const InstParams *params, double *out, hipStream_t s);

}  // namespace mpcb
