// mpc_stream_step_dist.hip -- gfx950 kernel of the controller step with an input disturbance in the prediction model (mpcb_step_dist,
// include/mpcbatch.h) on the THROUGHPUT engine: se::control_step<double, true, false, false, false, true>, the warm-start step with
// the DIST flag on every pass that reads u for the dynamics or for qddot -- x+ = Ad x + Bd (u + d): the defect, the qddot cost and its
// gradient rows and the shift's tail read the effective input (mpc_stream.h eff_u); the input cost row, the bounds and the stage
// Hessians are the ones they were.  On a ragged batch every simulation has its own d and its own horizon end.
//
// A translation unit of its own, like mpc_stream_step.hip and for the same reason: the kernels of mpcb_step ... mpcb_step_term stay
// the code they are.  Same launch shape, static LDS and disable_tail_calls; mpcb_step_dist launches it only when it is given a
// disturbance.
#include <hip/hip_runtime.h>

#ifndef MPCB_STREAM_WPE
#define MPCB_STREAM_WPE 2
#endif
#include "mpc_launch.h"
#include "mpc_stream.h"

using namespace mpcb;

__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_step_dist_kernel(Problem pb, const Robot *__restrict__ rbd,
                                                                                const InstParams *__restrict__ params, double *ws_base,
                                                                                size_t ws_stride, StepIO io, int reset)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    se::control_step<double, true, false, false, false, true>(pb, params, rbd, ws_base, ws_stride, io, inst, reset != 0);
#endif
}

namespace mpcb {
StreamStepFn stream_step_dist_kernel() { return mpc_stream_step_dist_kernel; }
}  // namespace mpcb
