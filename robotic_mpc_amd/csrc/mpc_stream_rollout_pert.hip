// mpc_stream_rollout_pert.hip -- gfx950 kernel of the rollout over a perturbed plant (mpcb_rollout_pert, include/mpcbatch.h) on the
// THROUGHPUT engine: se::rollout<double, true, true> (mpc_stream.h), the scheduled rollout's closed loop whose built-in plant has
// bandwidths of its own, an additive input disturbance and measurement noise on the feedback state.
//
// A translation unit of its own for the reason given in mpc_step.hip.  The two launch shapes of mpc_stream_kernel (mpc_kernel.hip):
// one wavefront per simulation, or the work queue over (simulation, chunk of steps) items, through the loop they all share
// (mpc_stream_queue.h, where the protocol is described).  What a work item hands to the next is the TRUE plant state
// (w.state[ST_Z]); the next item forms its own feedback state from it.  fp64 only.
//
// disable_tail_calls, as in mpc_stream_step.hip: the first pass of a step is called before anything local has escaped here as well.
#include <hip/hip_runtime.h>

#ifndef MPCB_STREAM_WPE
#define MPCB_STREAM_WPE 2
#endif
#include "mpc_launch.h"
#include "mpc_stream.h"
#include "mpc_stream_queue.h"

using namespace mpcb;

// yref_sched: [batch][Nsim + N][NTASK], N = pb.N (the longest horizon of the batch); pert: the three [batch][...] arrays of
// mpcb_plant_pert (each may be null)
template <class FT>
__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_pert_kernel(
    Problem pb, const Robot *__restrict__ rbd, const InstParams *__restrict__ params, double *ws_base, size_t ws_stride, Outputs out, int step0,
    int step1, int *queue, int chunk_steps, long long timeout_ticks, const double *__restrict__ yref_sched, PlantPert pert)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t rows = (size_t)pb.Nsim + pb.N;
    MPCB_STREAM_QUEUE_LOOP(se::rollout<FT, true, true>(pb, params, rbd, ws_base, ws_stride, out, inst, s0, s1,
                                                       yref_sched + (size_t)inst * rows * NTASK, plant_pert_of(pert, inst, pb.Nsim)))
#endif
}

namespace mpcb {
StreamRolloutPertFn stream_rollout_pert_kernel() { return mpc_stream_pert_kernel<double>; }
}  // namespace mpcb
