// mpc_rollout_surf.hip -- gfx950 kernels of the rollout over a scheduled, stage-varying surface (mpcb_rollout_surf, include/mpcbatch.h)
// on the latency engine: Engine<DevExec, 0, 0, 1>::rollout<true, true>, the perturbed rollout's closed loop on the engine built with its
// SURF flag -- stage k of closed-loop step t evaluates the task functions on the quadric of row t + k of the simulation's surface
// table, and log column t measures the task errors against row t.
//
// The table is read-only during a launch: the lanes that linearise load their stage's row from global memory, and the error log reads
// its row with uniform loads.  Nothing new carries between steps or launches; Smem, the pool and the workspace are those of every
// other kernel.
//
// A translation unit of its own for the reason given in mpc_step.hip.  Same geometries as mpc_rollout_pert_kernel.  A `pert` whose
// three members are null is the nominal plant.
#include <hip/hip_runtime.h>

#include "mpc_core.h"
#include "mpc_devexec.h"
#include "mpc_launch.h"

// yref_sched: [batch][Nsim + N][NTASK], N = pb.N; pert: the three [batch][...] arrays of mpcb_plant_pert (each may be null);
// surf_sched: [batch][Nsim + N][NSURF], not null
template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) void mpc_rollout_surf_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                                double *ws_base, size_t ws_stride, Outputs out, int step0,
                                                                int step1, int pool_doubles, const double *__restrict__ yref_sched,
                                                                PlantPert pert, const double *__restrict__ surf_sched)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>, 0, 0, 1> eng(ex, c);
    const size_t rows = (size_t)pb.Nsim + pb.N;
    eng.template rollout<true, true>(out, inst, step0, step1, yref_sched + (size_t)inst * rows * NTASK, plant_pert_of(pert, inst, pb.Nsim), {}, {},
                                     surf_sched + (size_t)inst * rows * NSURF);
}

namespace mpcb {
RolloutSurfFn rollout_surf_kernel(int waves_per_sim, int wpe) { return MPCB_GEOMETRY_KERNEL(RolloutSurfFn, mpc_rollout_surf_kernel, waves_per_sim, wpe); }
}  // namespace mpcb
