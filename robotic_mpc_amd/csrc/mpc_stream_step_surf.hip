// mpc_stream_step_surf.hip -- gfx950 kernel of the controller step over a scheduled, stage-varying surface (mpcb_step_surf,
// include/mpcbatch.h) on the THROUGHPUT engine: se::control_step<double, true, false, false, false, false, true>, the warm-start step
// with the SURF flag on the passes that evaluate the task functions (mpc_stream.h lin_pass, merit_pass): stage k reads the six
// coefficients of row k of the simulation's surface window io.surf.  On a ragged batch every simulation has its own window, strided by
// the batch's longest horizon, and reads the rows of its own.
//
// A translation unit of its own, like mpc_stream_step.hip and for the same reason: the kernels of mpcb_step ... mpcb_step_dist stay
// the code they are.  Same launch shape, static LDS and disable_tail_calls; mpcb_step_surf launches it only when it is given a window.
#include <hip/hip_runtime.h>

#ifndef MPCB_STREAM_WPE
#define MPCB_STREAM_WPE 2
#endif
#include "mpc_launch.h"
#include "mpc_stream.h"

using namespace mpcb;

__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_step_surf_kernel(Problem pb, const Robot *__restrict__ rbd,
                                                                                const InstParams *__restrict__ params, double *ws_base,
                                                                                size_t ws_stride, StepIO io, int reset)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    se::control_step<double, true, false, false, false, false, true>(pb, params, rbd, ws_base, ws_stride, io, inst, reset != 0);
#endif
}

namespace mpcb {
StreamStepFn stream_step_surf_kernel() { return mpc_stream_step_surf_kernel; }
}  // namespace mpcb
