// mpc_rollout_pert.hip -- gfx950 kernels of the rollout over a perturbed plant (mpcb_rollout_pert, include/mpcbatch.h) on the latency
// engine: Engine::rollout<true, true>, the scheduled rollout's closed loop whose built-in plant has bandwidths of its own, an additive
// input disturbance and measurement noise on the feedback state.  The logs record the true plant state; the solve sees the noisy one.
//
// A translation unit of its own for the reason given in mpc_step.hip: instantiated next to the rollout kernels of mpc_kernel.hip or
// mpc_rollout_ref.hip, these kernels would change the code of those.  Same geometries (DevExec<NWV, WPE>), dynamic-LDS pool and
// workspace as mpc_rollout_kernel; the perturbation arrays are read from global memory by the lanes that use them.
#include <hip/hip_runtime.h>

#include "mpc_core.h"
#include "mpc_devexec.h"
#include "mpc_launch.h"

// yref_sched: [batch][Nsim + N][NTASK], N = pb.N; pert: the three [batch][...] arrays of mpcb_plant_pert (each may be null)
template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) void mpc_rollout_pert_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                                double *ws_base, size_t ws_stride, Outputs out, int step0,
                                                                int step1, int pool_doubles, const double *__restrict__ yref_sched,
                                                                PlantPert pert)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>> eng(ex, c);
    eng.template rollout<true, true>(out, inst, step0, step1, yref_sched + (size_t)inst * ((size_t)pb.Nsim + pb.N) * NTASK,
                                     plant_pert_of(pert, inst, pb.Nsim));
}

namespace mpcb {
RolloutPertFn rollout_pert_kernel(int waves_per_sim, int wpe) { return MPCB_GEOMETRY_KERNEL(RolloutPertFn, mpc_rollout_pert_kernel, waves_per_sim, wpe); }
}  // namespace mpcb
