// mpc_rollout_ref.hip -- gfx950 kernels of the rollout against a task reference schedule (mpcb_rollout_ref, include/mpcbatch.h) on
// the latency engine: Engine::rollout<true>, the closed loop whose step t tracks the window [t, t + N) of each simulation's schedule
// and whose error log measures column t against schedule row t.
//
// A translation unit of its own for the reason given in mpc_step.hip: instantiated next to the rollout kernels of mpc_kernel.hip,
// these kernels would change the code of those.  Same geometries (DevExec<NWV, WPE>), dynamic-LDS pool and workspace as
// mpc_rollout_kernel.
#include <hip/hip_runtime.h>

#include "mpc_core.h"
#include "mpc_devexec.h"
#include "mpc_launch.h"

// yref_sched: [batch][Nsim + N][NTASK], N = pb.N
template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) void mpc_rollout_ref_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                               double *ws_base, size_t ws_stride, Outputs out, int step0,
                                                               int step1, int pool_doubles, const double *__restrict__ yref_sched)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>> eng(ex, c);
    eng.template rollout<true>(out, inst, step0, step1, yref_sched + (size_t)inst * ((size_t)pb.Nsim + pb.N) * NTASK);
}

namespace mpcb {
RolloutRefFn rollout_ref_kernel(int waves_per_sim, int wpe) { return MPCB_GEOMETRY_KERNEL(RolloutRefFn, mpc_rollout_ref_kernel, waves_per_sim, wpe); }
}  // namespace mpcb
