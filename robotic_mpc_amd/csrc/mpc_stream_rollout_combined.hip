// mpc_stream_rollout_combined.hip -- gfx950 kernel of the rollout in which the terminal cost, the disturbance observer, the scheduled
// surface and the shift warm start are live at once (mpcb_rollout_combined, include/mpcbatch.h) on the THROUGHPUT engine:
// se::rollout<double, true, true, true, true, true, true> (mpc_stream.h).  Every step is ONE mpc_step carrying TermArg<TERM_TABLE>,
// DistArg<DIST_SHARED> and lin_pass<true, 1> / line_search<true, 1>; before it the observer publishes d^_t (g_ssm, lv_dhat, and row t
// of the d_hat log) and then a simulation whose mode is MPCB_WARM_SHIFT shifts (t >= 1, shift_pass<false, DIST_SHARED>: the tail takes
// u_{N-1} + d^_t).  x_e is row t of the terminal table and the surface window starts at row t of the surface table, t the absolute
// step number: the first step of a later launch and of a later work item read the rows the single launch reads.
//
// Ragged horizons: the terminal cost sits on each simulation's own last stage, its shift ends at its own horizon, and its tables have
// Nsim + NMAX rows (NMAX = pb.N, the longest horizon of the batch).  One kernel, not one per subset: a simulation that does not use a
// feature runs with neutral data for it, which the host fills (mpc_rollout_combined.hip says which).
//
// A translation unit of its own for the reason given in mpc_step.hip.  The two launch shapes of mpc_stream_kernel (mpc_kernel.hip):
// one wavefront per simulation, or the work queue over (simulation, chunk of steps) items, through the loop they all share
// (mpc_stream_queue.h).  A work item hands on what the observer rollout's hands on (ST_OBS with ST_Z) and nothing more.  fp64 only.
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
// mpcb_plant_pert (each may be null); term: blocks [batch][18] and x_ref [batch][Nsim][12]; obs: gain [batch][12] (read) and d_hat
// [batch][Nsim][6] (written); surf_sched: [batch][Nsim + N][NSURF]; warm: [batch] of MPCB_WARM_* -- none of them null
template <class FT>
__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_combined_kernel(
    Problem pb, const Robot *__restrict__ rbd, const InstParams *__restrict__ params, double *ws_base, size_t ws_stride, Outputs out, int step0,
    int step1, int *queue, int chunk_steps, long long timeout_ticks, const double *__restrict__ yref_sched, PlantPert pert, TermTab term,
    ObsArg obs, const double *__restrict__ surf_sched, const int *__restrict__ warm)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t rows = (size_t)pb.Nsim + pb.N;
    MPCB_STREAM_QUEUE_LOOP(se::rollout<FT, true, true, true, true, true, true>(pb, params, rbd, ws_base, ws_stride, out, inst, s0, s1,
                                                                               yref_sched + (size_t)inst * rows * NTASK,
                                                                               plant_pert_of(pert, inst, pb.Nsim),
                                                                               term_tab_of(term, inst, pb.Nsim),
                                                                               obs_arg_of(obs, inst, pb.Nsim),
                                                                               surf_sched + (size_t)inst * rows * NSURF,
                                                                               se::uni(warm[inst])))
#endif
}

namespace mpcb {
StreamRolloutCombinedFn stream_rollout_combined_kernel() { return mpc_stream_combined_kernel<double>; }
}  // namespace mpcb
