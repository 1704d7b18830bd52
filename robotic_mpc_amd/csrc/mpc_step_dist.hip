// mpc_step_dist.hip -- gfx950 kernels of the controller step with an input disturbance in the prediction model (mpcb_step_dist,
// include/mpcbatch.h) on the latency engine: Engine<DevExec, 0, true>::control_step<true>, the warm-start step of the engine built
// with its DIST flag -- x+ = Ad x + Bd (u + d): the dynamics defect, the qddot residual with its gradient rows and the shift's tail
// read the effective input u + d (Engine::eff_u); the input cost row, the bounds and the stage Hessians are the ones they were.
//
// A translation unit of its own for the reason given in mpc_step.hip: the kernels of mpcb_step ... mpcb_step_term stay the code they
// are, whatever is compiled next to them.  Same geometries, dynamic-LDS pool, workspace and disable_tail_calls as mpc_step_kernel;
// mpcb_step_dist launches these only when it is given a disturbance.
#include <hip/hip_runtime.h>

#include "mpc_core.h"
#include "mpc_devexec.h"
#include "mpc_launch.h"

template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) __attribute__((disable_tail_calls)) void mpc_step_dist_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                        double *ws_base, size_t ws_stride, StepIO io, int reset, int pool_doubles)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>, 0, true> eng(ex, c);
    eng.template control_step<true>(io, inst, reset != 0);
}

namespace mpcb {
StepFn step_dist_kernel(int waves_per_sim, int wpe) { return MPCB_GEOMETRY_KERNEL(StepFn, mpc_step_dist_kernel, waves_per_sim, wpe); }
}  // namespace mpcb
