// mpc_stream_step_term_sens.hip -- gfx950 kernel of the controller step with the joint-wise terminal cost that also returns the
// sensitivities of u0 (mpcb_step_term with sens, include/mpcbatch.h) on the THROUGHPUT engine: se::control_step<double, true, true,
// false, true>, the step of mpc_stream_step_term.hip with se::sens_pass between the QP solve and the closing linearisation; the pass
// also forms d u0 / d x_e from the last stage of its recursion.
//
// A translation unit of its own, like mpc_stream_step.hip and for the same reason.  Same launch shape, static LDS and
// disable_tail_calls; mpcb_step_term launches it only when it is given a terminal cost and somewhere to write the sensitivities.
#include <hip/hip_runtime.h>

#ifndef MPCB_STREAM_WPE
#define MPCB_STREAM_WPE 2
#endif
#include "mpc_launch.h"
#include "mpc_stream.h"

using namespace mpcb;

__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_step_term_sens_kernel(Problem pb, const Robot *__restrict__ rbd,
                                                                                const InstParams *__restrict__ params, double *ws_base,
                                                                                size_t ws_stride, StepIO io, int reset)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    se::control_step<double, true, true, false, true>(pb, params, rbd, ws_base, ws_stride, io, inst, reset != 0);
#endif
}

namespace mpcb {
StreamStepFn stream_step_term_sens_kernel() { return mpc_stream_step_term_sens_kernel; }
}  // namespace mpcb
