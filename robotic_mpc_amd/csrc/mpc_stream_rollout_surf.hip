// mpc_stream_rollout_surf.hip -- gfx950 kernel of the rollout over a scheduled, stage-varying surface (mpcb_rollout_surf,
// include/mpcbatch.h) on the THROUGHPUT engine: se::rollout<double, true, true, false, false, true> (mpc_stream.h), the perturbed
// rollout's closed loop with the SURF flag on the passes that evaluate the task functions -- stage k of closed-loop step t reads row
// t + k of the simulation's surface table, log column t row t.
//
// A translation unit of its own for the reason given in mpc_step.hip.  The two launch shapes of mpc_stream_kernel (mpc_kernel.hip):
// one wavefront per simulation, or the work queue over (simulation, chunk of steps) items, through the loop they all share
// (mpc_stream_queue.h).  A work item hands on what the perturbed rollout's does and nothing more: the row index is the absolute step
// number, so an item finds its rows whichever wavefront ran the one before.  Ragged horizons: tables are strided by the longest
// horizon of the batch, a simulation of horizon N_i reads rows [t, t + N_i).  fp64 only.
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
// mpcb_plant_pert (each may be null); surf_sched: [batch][Nsim + N][NSURF], not null
template <class FT>
__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_surf_kernel(
    Problem pb, const Robot *__restrict__ rbd, const InstParams *__restrict__ params, double *ws_base, size_t ws_stride, Outputs out, int step0,
    int step1, int *queue, int chunk_steps, long long timeout_ticks, const double *__restrict__ yref_sched, PlantPert pert,
    const double *__restrict__ surf_sched)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t rows = (size_t)pb.Nsim + pb.N;
    MPCB_STREAM_QUEUE_LOOP(se::rollout<FT, true, true, false, false, true>(pb, params, rbd, ws_base, ws_stride, out, inst, s0, s1,
                                                                           yref_sched + (size_t)inst * rows * NTASK,
                                                                           plant_pert_of(pert, inst, pb.Nsim), {}, {},
                                                                           surf_sched + (size_t)inst * rows * NSURF))
#endif
}

namespace mpcb {
StreamRolloutSurfFn stream_rollout_surf_kernel() { return mpc_stream_surf_kernel<double>; }
}  // namespace mpcb
