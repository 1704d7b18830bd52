// mpc_stream_step_warm.hip -- gfx950 kernel of the controller step with a per-simulation warm start (mpcb_step_warm,
// include/mpcbatch.h) on the THROUGHPUT engine: se::control_step<double, true>, which reads each simulation's mode from StepIO::warm --
// carry, reset, or shift the carried solver memory one stage first (se::shift_pass).
//
// A translation unit of its own, like mpc_stream_step.hip and for the same reason: the kernel of mpcb_step / mpcb_step_ref stays the
// code it is.  Same launch shape, static LDS and disable_tail_calls; mpcb_step_warm launches it only when it is given a mode array.
#include <hip/hip_runtime.h>

#ifndef MPCB_STREAM_WPE
#define MPCB_STREAM_WPE 2
#endif
#include "mpc_launch.h"
#include "mpc_stream.h"

using namespace mpcb;

__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_step_warm_kernel(Problem pb, const Robot *__restrict__ rbd,
                                                                                const InstParams *__restrict__ params, double *ws_base,
                                                                                size_t ws_stride, StepIO io, int reset)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    se::control_step<double, true>(pb, params, rbd, ws_base, ws_stride, io, inst, reset != 0);
#endif
}

namespace mpcb {
StreamStepFn stream_step_warm_kernel() { return mpc_stream_step_warm_kernel; }
}  // namespace mpcb
