// mpc_stream_step_sensw.hip -- gfx950 kernel of the controller step that returns, with the feedback gain and the reference sensitivity
// of u0, its sensitivity to the seven cost weights (mpcb_step_sens_w, include/mpcbatch.h) on the THROUGHPUT engine:
// se::control_step<double, true, true, true>, the warm-start step with se::sens_pass<true> between the QP solve and the closing
// linearisation.
//
// A translation unit of its own, like mpc_stream_step.hip and for the same reason: the kernels of mpcb_step ... mpcb_step_sens stay
// the code they are.  Same launch shape, static LDS and disable_tail_calls; mpcb_step_sens_w launches it only when it is given
// somewhere to write du0_dw.
#include <hip/hip_runtime.h>

#ifndef MPCB_STREAM_WPE
#define MPCB_STREAM_WPE 2
#endif
#include "mpc_launch.h"
#include "mpc_stream.h"

using namespace mpcb;

__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_step_sensw_kernel(Problem pb, const Robot *__restrict__ rbd,
                                                                                const InstParams *__restrict__ params, double *ws_base,
                                                                                size_t ws_stride, StepIO io, int reset)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    se::control_step<double, true, true, true>(pb, params, rbd, ws_base, ws_stride, io, inst, reset != 0);
#endif
}

namespace mpcb {
StreamStepFn stream_step_sensw_kernel() { return mpc_stream_step_sensw_kernel; }
}  // namespace mpcb
