// mpc_step_sensw.hip -- gfx950 kernels of the controller step that returns, with the feedback gain and the reference sensitivity of
// u0, its sensitivity to the seven cost weights (mpcb_step_sens_w, include/mpcbatch.h) on the latency engine:
// Engine::control_step<true, true, true>, the warm-start step with Engine::sens_pass<true> between the QP solve and the closing
// linearisation.
//
// A translation unit of its own for the reason given in mpc_step.hip: the kernels of mpcb_step ... mpcb_step_sens stay the code they
// are, whatever is compiled next to them.  Same geometries, dynamic-LDS pool, workspace and disable_tail_calls as mpc_step_kernel;
// mpcb_step_sens_w launches these only when it is given somewhere to write du0_dw.
#include <hip/hip_runtime.h>

#include "mpc_core.h"
#include "mpc_devexec.h"
#include "mpc_launch.h"

template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) __attribute__((disable_tail_calls)) void mpc_step_sensw_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                        double *ws_base, size_t ws_stride, StepIO io, int reset, int pool_doubles)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>> eng(ex, c);
    eng.template control_step<true, true, true>(io, inst, reset != 0);
}

namespace mpcb {
StepFn step_sensw_kernel(int waves_per_sim, int wpe) { return MPCB_GEOMETRY_KERNEL(StepFn, mpc_step_sensw_kernel, waves_per_sim, wpe); }
}  // namespace mpcb
