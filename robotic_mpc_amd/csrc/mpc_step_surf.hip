// mpc_step_surf.hip -- gfx950 kernels of the controller step over a scheduled, stage-varying surface (mpcb_step_surf,
// include/mpcbatch.h) on the latency engine: Engine<DevExec, 0, 0, 1>::control_step<true>, the warm-start step of the engine built with
// its SURF flag -- stage k of the horizon evaluates the task functions g1, g2 and their Jacobians on the quadric of row k of the
// simulation's surface window io.surf, in the linearisation and in the residual-only pass of the line search (task_lin's overload
// with coefficients, mpc_kin.h).  The lane that linearises stage k loads that row's six doubles itself, past the kinematics.
//
// A translation unit of its own for the reason given in mpc_step.hip: the kernels of mpcb_step ... mpcb_step_dist stay the code they
// are, whatever is compiled next to them.  Same geometries, dynamic-LDS pool, workspace and disable_tail_calls as mpc_step_kernel;
// mpcb_step_surf launches these only when it is given a window.
#include <hip/hip_runtime.h>

#include "mpc_core.h"
#include "mpc_devexec.h"
#include "mpc_launch.h"

template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) __attribute__((disable_tail_calls)) void mpc_step_surf_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                        double *ws_base, size_t ws_stride, StepIO io, int reset, int pool_doubles)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>, 0, 0, 1> eng(ex, c);
    eng.template control_step<true>(io, inst, reset != 0);
}

namespace mpcb {
StepFn step_surf_kernel(int waves_per_sim, int wpe) { return MPCB_GEOMETRY_KERNEL(StepFn, mpc_step_surf_kernel, waves_per_sim, wpe); }
}  // namespace mpcb
