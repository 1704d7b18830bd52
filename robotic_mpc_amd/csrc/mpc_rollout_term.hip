// mpc_rollout_term.hip -- gfx950 kernels of the rollout with the joint-wise terminal cost (mpcb_rollout_term, include/mpcbatch.h) on the
// latency engine: Engine<DevExec, TERM_TABLE>::rollout<true, true>, the perturbed rollout's closed loop on the engine built with its
// TERM flag (the value that reads the record from two arrays) -- every step's Riccati recursion starts from P_N = lm I + P, and its stage-N gradient, cost and stationarity rows take the
// terminal term (mpc_nlp.h term_*) against row t of the simulation's reference table.
//
// A translation unit of its own for the reason given in mpc_step.hip: instantiated next to any other rollout kernel, these kernels
// would change the code of those.  Same geometries (DevExec<NWV, WPE>), dynamic-LDS pool and workspace as mpc_rollout_kernel; the
// blocks, the reference rows and the perturbation arrays are read from global memory where they are used.  A `pert` whose three
// members are null is the nominal plant: one kernel family serves both.
#include <hip/hip_runtime.h>

#include "mpc_core.h"
#include "mpc_devexec.h"
#include "mpc_launch.h"

// yref_sched: [batch][Nsim + N][NTASK], N = pb.N; pert: the three [batch][...] arrays of mpcb_plant_pert (each may be null);
// term: blocks [batch][18] and x_ref [batch][Nsim][12] (neither null)
template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) void mpc_rollout_term_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                                double *ws_base, size_t ws_stride, Outputs out, int step0,
                                                                int step1, int pool_doubles, const double *__restrict__ yref_sched,
                                                                PlantPert pert, TermTab term)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>, TERM_TABLE> eng(ex, c);
    eng.template rollout<true, true>(out, inst, step0, step1, yref_sched + (size_t)inst * ((size_t)pb.Nsim + pb.N) * NTASK,
                                     plant_pert_of(pert, inst, pb.Nsim), term_tab_of(term, inst, pb.Nsim));
}

namespace mpcb {
RolloutTermFn rollout_term_kernel(int waves_per_sim, int wpe) { return MPCB_GEOMETRY_KERNEL(RolloutTermFn, mpc_rollout_term_kernel, waves_per_sim, wpe); }
}  // namespace mpcb
