// mpc_rollout_shift.hip -- gfx950 kernels of the rollout with the shift warm start (mpcb_rollout_warm, include/mpcbatch.h) on the
// latency engine: Engine<DevExec, 0, 0, SURF>::rollout<true, true, false, true>, the perturbed rollout's closed loop in which a
// simulation whose mode is MPCB_WARM_SHIFT moves its carried solver memory one stage towards stage 0 (Engine::shift_pass) at the top
// of every step t >= 1 -- t the absolute step number -- as mpcb_step_warm does.  Two kernel families: without a surface table
// (SURF = 0) and over a scheduled surface (SURF = 1, the step of mpc_rollout_surf.hip).
//
// The mode is one uniform load per simulation.  shift_pass stages blocks of stage records through the chunk pool, of which nothing is
// live between two steps of a scheduled rollout (Engine::rollout says why).  Nothing new carries between steps or launches; Smem,
// the pool and the workspace are those of every other kernel.
//
// A translation unit of its own for the reason given in mpc_step.hip.  Same geometries as mpc_rollout_pert_kernel.  A `pert` whose
// three members are null is the nominal plant.
#include <hip/hip_runtime.h>

#include "mpc_core.h"
#include "mpc_devexec.h"
#include "mpc_launch.h"

template <int NWV, int WPE, int SURF>
__device__ __forceinline__ void rollout_shift_body(const Problem &pb, const Robot &rb, const InstParams *__restrict__ params, double *ws_base,
                                                   size_t ws_stride, const Outputs &out, int step0, int step1, int pool_doubles,
                                                   const double *__restrict__ yref_sched, const PlantPert &pert,
                                                   const double *__restrict__ surf_sched, const int *__restrict__ warm)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>, 0, 0, SURF> eng(ex, c);
    const size_t rows = (size_t)pb.Nsim + pb.N;
    const int mode = ex.uni(warm[inst]);
    if constexpr (SURF != 0)
        eng.template rollout<true, true, false, true>(out, inst, step0, step1, yref_sched + (size_t)inst * rows * NTASK,
                                                      plant_pert_of(pert, inst, pb.Nsim), {}, {}, surf_sched + (size_t)inst * rows * NSURF, mode);
    else
        eng.template rollout<true, true, false, true>(out, inst, step0, step1, yref_sched + (size_t)inst * rows * NTASK,
                                                      plant_pert_of(pert, inst, pb.Nsim), {}, {}, {}, mode);
}

// yref_sched: [batch][Nsim + N][NTASK], N = pb.N; pert: the three [batch][...] arrays of mpcb_plant_pert (each may be null);
// surf_sched: not read; warm: [batch] of MPCB_WARM_*, not null
template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) void mpc_rollout_shift_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                                 double *ws_base, size_t ws_stride, Outputs out, int step0,
                                                                 int step1, int pool_doubles, const double *__restrict__ yref_sched,
                                                                 PlantPert pert, const double *__restrict__ surf_sched,
                                                                 const int *__restrict__ warm)
{
    rollout_shift_body<NWV, WPE, 0>(pb, rb, params, ws_base, ws_stride, out, step0, step1, pool_doubles, yref_sched, pert, surf_sched, warm);
}

// surf_sched: [batch][Nsim + N][NSURF], not null
template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) void mpc_rollout_shift_surf_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                                      double *ws_base, size_t ws_stride, Outputs out, int step0,
                                                                      int step1, int pool_doubles, const double *__restrict__ yref_sched,
                                                                      PlantPert pert, const double *__restrict__ surf_sched,
                                                                      const int *__restrict__ warm)
{
    rollout_shift_body<NWV, WPE, 1>(pb, rb, params, ws_base, ws_stride, out, step0, step1, pool_doubles, yref_sched, pert, surf_sched, warm);
}

namespace mpcb {
RolloutShiftFn rollout_shift_kernel(int waves_per_sim, int wpe, bool surf)
{
    if (surf) return MPCB_GEOMETRY_KERNEL(RolloutShiftFn, mpc_rollout_shift_surf_kernel, waves_per_sim, wpe);
    return MPCB_GEOMETRY_KERNEL(RolloutShiftFn, mpc_rollout_shift_kernel, waves_per_sim, wpe);
}
}  // namespace mpcb
