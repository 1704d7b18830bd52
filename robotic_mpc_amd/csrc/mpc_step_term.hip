// mpc_step_term.hip -- gfx950 kernels of the controller step with the joint-wise terminal cost (mpcb_step_term, include/mpcbatch.h) on
// the latency engine: Engine<DevExec, true>::control_step<true>, the warm-start step of the engine built with its TERM flag -- the
// Riccati recursion starts from P_N = lm I + P, and the stage-N gradient, cost and stationarity rows take the terminal term
// (mpc_nlp.h term_*).
//
// A translation unit of its own for the reason given in mpc_step.hip: the kernels of mpcb_step ... mpcb_step_sens_w stay the code they
// are, whatever is compiled next to them.  Same geometries, dynamic-LDS pool, workspace and disable_tail_calls as mpc_step_kernel;
// mpcb_step_term launches these only when it is given a terminal cost and nowhere to write sensitivities.
#include <hip/hip_runtime.h>

#include "mpc_core.h"
#include "mpc_devexec.h"
#include "mpc_launch.h"

template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) __attribute__((disable_tail_calls)) void mpc_step_term_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                        double *ws_base, size_t ws_stride, StepIO io, int reset, int pool_doubles)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>, true> eng(ex, c);
    eng.template control_step<true>(io, inst, reset != 0);
}

namespace mpcb {
StepFn step_term_kernel(int waves_per_sim, int wpe) { return MPCB_GEOMETRY_KERNEL(StepFn, mpc_step_term_kernel, waves_per_sim, wpe); }
}  // namespace mpcb
