// mpc_stream_rollout_shift.hip -- gfx950 kernels of the rollout with the shift warm start (mpcb_rollout_warm, include/mpcbatch.h) on
// the THROUGHPUT engine: se::rollout<double, true, true, false, false, SURF, true> (mpc_stream.h), the perturbed rollout's closed loop
// in which a simulation whose mode is MPCB_WARM_SHIFT moves its carried solver memory one stage towards stage 0 of its own horizon
// (se::shift_pass<false>) at the top of every step t >= 1, as mpcb_step_warm does.  Two kernels: without a surface table, and over a
// scheduled surface (the step of mpc_stream_rollout_surf.hip).
//
// A translation unit of its own for the reason given in mpc_step.hip.  The two launch shapes of mpc_stream_kernel (mpc_kernel.hip):
// one wavefront per simulation, or the work queue over (simulation, chunk of steps) items, through the loop they all share
// (mpc_stream_queue.h).  t is the absolute step number, so a work item that starts at step t >= 1 shifts first, whichever wavefront
// ran the item before; it hands on what the perturbed rollout's does and nothing more.  The mode is one uniform load per item.
// Ragged horizons: each simulation shifts over its own horizon and propagates the tail at its own end.  fp64 only.
//
// disable_tail_calls, as in mpc_stream_step.hip.
#include <hip/hip_runtime.h>

#ifndef MPCB_STREAM_WPE
#define MPCB_STREAM_WPE 2
#endif
#include "mpc_launch.h"
#include "mpc_stream.h"
#include "mpc_stream_queue.h"

using namespace mpcb;

// yref_sched: [batch][Nsim + N][NTASK], N = pb.N (the longest horizon of the batch); pert: the three [batch][...] arrays of
// mpcb_plant_pert (each may be null); surf_sched: not read; warm: [batch] of MPCB_WARM_*, not null
template <class FT>
__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_shift_kernel(
    Problem pb, const Robot *__restrict__ rbd, const InstParams *__restrict__ params, double *ws_base, size_t ws_stride, Outputs out, int step0,
    int step1, int *queue, int chunk_steps, long long timeout_ticks, const double *__restrict__ yref_sched, PlantPert pert,
    const double *__restrict__ surf_sched, const int *__restrict__ warm)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t rows = (size_t)pb.Nsim + pb.N;
    MPCB_STREAM_QUEUE_LOOP(se::rollout<FT, true, true, false, false, false, true>(pb, params, rbd, ws_base, ws_stride, out, inst, s0, s1,
                                                                                  yref_sched + (size_t)inst * rows * NTASK,
                                                                                  plant_pert_of(pert, inst, pb.Nsim), {}, {}, {},
                                                                                  se::uni(warm[inst])))
#endif
}

// surf_sched: [batch][Nsim + N][NSURF], not null
template <class FT>
__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_shift_surf_kernel(
    Problem pb, const Robot *__restrict__ rbd, const InstParams *__restrict__ params, double *ws_base, size_t ws_stride, Outputs out, int step0,
    int step1, int *queue, int chunk_steps, long long timeout_ticks, const double *__restrict__ yref_sched, PlantPert pert,
    const double *__restrict__ surf_sched, const int *__restrict__ warm)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t rows = (size_t)pb.Nsim + pb.N;
    MPCB_STREAM_QUEUE_LOOP(se::rollout<FT, true, true, false, false, true, true>(pb, params, rbd, ws_base, ws_stride, out, inst, s0, s1,
                                                                                 yref_sched + (size_t)inst * rows * NTASK,
                                                                                 plant_pert_of(pert, inst, pb.Nsim), {}, {},
                                                                                 surf_sched + (size_t)inst * rows * NSURF,
                                                                                 se::uni(warm[inst])))
#endif
}

namespace mpcb {
StreamRolloutShiftFn stream_rollout_shift_kernel(bool surf)
{
    return surf ? mpc_stream_shift_surf_kernel<double> : mpc_stream_shift_kernel<double>;
}
}  // namespace mpcb
