// mpc_step_combined.hip -- gfx950 kernels of the controller step in which the terminal cost, the input disturbance, the surface window
// and the per-simulation warm start are in force at once (mpcb_step_combined, include/mpcbatch.h) on the latency engine:
// Engine<DevExec, 1, 1, 1>::control_step<true>.  One real-time iteration of the NLP whose stage k evaluates its task outputs on row k
// of io.surf, whose model is x+ = Ad x + Bd (u + d) with d = io.dist, and whose stage N adds 1/2 (x_N - x_e)' P (x_N - x_e) from
// io.term; with MPCB_WARM_SHIFT the carried memory moves one stage first and the tail takes u_{N-1} + d, this step's disturbance.
//
// ONE instantiation per geometry: a simulation that does not use a feature brings neutral data for it (zero blocks, d = 0, a window
// whose rows equal its own a..f, MPCB_WARM_CARRY), which the host fills -- the kernel takes no branch on a null pointer
// (mpc_rollout_combined.hip).  No sensitivities.
//
// A translation unit of its own for the reason given in mpc_step.hip.  Same geometries, dynamic-LDS pool, workspace and
// disable_tail_calls as mpc_step_kernel.
#include <hip/hip_runtime.h>

#include "mpc_core.h"
#include "mpc_devexec.h"
#include "mpc_launch.h"

// io.term [batch][NTERM], io.dist [batch][6], io.surf [batch][N][NSURF]: not null; io.warm: [batch] or null (carry)
template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) __attribute__((disable_tail_calls)) void mpc_step_combined_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                        double *ws_base, size_t ws_stride, StepIO io, int reset, int pool_doubles)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>, 1, 1, 1> eng(ex, c);
    eng.template control_step<true>(io, inst, reset != 0);
}

namespace mpcb {
StepFn step_combined_kernel(int waves_per_sim, int wpe) { return MPCB_GEOMETRY_KERNEL(StepFn, mpc_step_combined_kernel, waves_per_sim, wpe); }
}  // namespace mpcb
