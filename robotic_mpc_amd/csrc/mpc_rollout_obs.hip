// mpc_rollout_obs.hip -- gfx950 kernels of the rollout with an on-device disturbance observer (mpcb_rollout_obs, include/mpcbatch.h) on
// the latency engine: Engine<DevExec, 0, DIST_SHARED>::rollout<true, true, true>, the perturbed rollout's closed loop on the engine built
// with its DIST flag -- x+ = Ad x + Bd (u + d^_t) in every step's prediction model -- whose d^_t is the estimate the rollout's own
// observer formed at the end of step t - 1 (mpc_nlp.h observer_next: DisturbanceObserver of observer.py, re-associated in time).
//
// Where eff_u finds d^: in Smem, in six slots of logv that no log row uses (lv_dhat, mpc_layout.h), which the plant lanes write before
// the solve and every lane reads after the phase barrier.  Not in the [batch][Nsim][6] log, which the kernel only writes: a uniform
// load of a location the same kernel stored to may be served from a scalar-cache line fetched before the store (rows of 48 bytes
// share lines with the previous step's row).  Smem, the pool and the workspace are those of every other kernel.
//
// A translation unit of its own for the reason given in mpc_step.hip.  Same geometries as mpc_rollout_kernel.  A `pert` whose three
// members are null is the nominal plant.
#include <hip/hip_runtime.h>

#include "mpc_core.h"
#include "mpc_devexec.h"
#include "mpc_launch.h"

// yref_sched: [batch][Nsim + N][NTASK], N = pb.N; pert: the three [batch][...] arrays of mpcb_plant_pert (each may be null);
// obs: gain [batch][12] = l1 6 | l2 6 (read) and d_hat [batch][Nsim][6] (written), neither null
template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) void mpc_rollout_obs_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                               double *ws_base, size_t ws_stride, Outputs out, int step0,
                                                               int step1, int pool_doubles, const double *__restrict__ yref_sched,
                                                               PlantPert pert, ObsArg obs)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>, 0, DIST_SHARED> eng(ex, c);
    eng.template rollout<true, true, true>(out, inst, step0, step1, yref_sched + (size_t)inst * ((size_t)pb.Nsim + pb.N) * NTASK,
                                           plant_pert_of(pert, inst, pb.Nsim), {}, obs_arg_of(obs, inst, pb.Nsim));
}

namespace mpcb {
RolloutObsFn rollout_obs_kernel(int waves_per_sim, int wpe) { return MPCB_GEOMETRY_KERNEL(RolloutObsFn, mpc_rollout_obs_kernel, waves_per_sim, wpe); }
}  // namespace mpcb
