// mpc_stream_rollout_obs.hip -- gfx950 kernel of the rollout with an on-device disturbance observer (mpcb_rollout_obs,
// include/mpcbatch.h) on the THROUGHPUT engine: se::rollout<double, true, true, false, true> (mpc_stream.h), the perturbed rollout's
// closed loop with the DIST flag threaded through the step as DIST_SHARED -- x+ = Ad x + Bd (u + d^_t) in every step's prediction model,
// d^_t the estimate the rollout's own observer formed at the end of step t - 1 (mpc_nlp.h observer_next), kept in g_ssm (free slots of
// logv, lv_dhat) where eff_u reads it; the [batch][Nsim][6] log is only written.  On a ragged batch every simulation runs its own horizon, as in the
// perturbed rollout.  A `pert` whose three members are null is the nominal plant.
//
// A translation unit of its own for the reason given in mpc_step.hip.  The two launch shapes of mpc_stream_kernel (mpc_kernel.hip):
// one wavefront per simulation, or the work queue over (simulation, chunk of steps) items, through the loop they all share
// (mpc_stream_queue.h).  What a work item hands to the next is what the perturbed rollout's hands on, plus the twelve doubles of the
// observer in w.state[ST_OBS], stored before the release and loaded after the acquire with ST_Z.  fp64 only.
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
// mpcb_plant_pert (each may be null); obs: gain [batch][12] = l1 6 | l2 6 (read) and d_hat [batch][Nsim][6] (written), neither null
template <class FT>
__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_obs_kernel(
    Problem pb, const Robot *__restrict__ rbd, const InstParams *__restrict__ params, double *ws_base, size_t ws_stride, Outputs out, int step0,
    int step1, int *queue, int chunk_steps, long long timeout_ticks, const double *__restrict__ yref_sched, PlantPert pert,
    ObsArg obs)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t rows = (size_t)pb.Nsim + pb.N;
    MPCB_STREAM_QUEUE_LOOP(se::rollout<FT, true, true, false, true>(pb, params, rbd, ws_base, ws_stride, out, inst, s0, s1,
                                                                    yref_sched + (size_t)inst * rows * NTASK,
                                                                    plant_pert_of(pert, inst, pb.Nsim), {},
                                                                    obs_arg_of(obs, inst, pb.Nsim)))
#endif
}

namespace mpcb {
StreamRolloutObsFn stream_rollout_obs_kernel() { return mpc_stream_obs_kernel<double>; }
}  // namespace mpcb
