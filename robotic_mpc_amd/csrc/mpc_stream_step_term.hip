// mpc_stream_step_term.hip -- gfx950 kernel of the controller step with the joint-wise terminal cost (mpcb_step_term,
// include/mpcbatch.h) on the THROUGHPUT engine: se::control_step<double, true, false, false, true>, the warm-start step with the TERM
// flag on every pass that sees stage N -- the Riccati recursion starts from P_N = lm I + P, and the stage-N gradient, cost and
// stationarity rows take the terminal term (mpc_nlp.h term_*).  On a ragged batch stage N is each simulation's own horizon end.
//
// A translation unit of its own, like mpc_stream_step.hip and for the same reason: the kernels of mpcb_step ... mpcb_step_sens_w stay
// the code they are.  Same launch shape, static LDS and disable_tail_calls; mpcb_step_term launches it only when it is given a
// terminal cost and nowhere to write sensitivities.
#include <hip/hip_runtime.h>

#ifndef MPCB_STREAM_WPE
#define MPCB_STREAM_WPE 2
#endif
#include "mpc_launch.h"
#include "mpc_stream.h"

using namespace mpcb;

__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_step_term_kernel(Problem pb, const Robot *__restrict__ rbd,
                                                                                const InstParams *__restrict__ params, double *ws_base,
                                                                                size_t ws_stride, StepIO io, int reset)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    se::control_step<double, true, false, false, true>(pb, params, rbd, ws_base, ws_stride, io, inst, reset != 0);
#endif
}

namespace mpcb {
StreamStepFn stream_step_term_kernel() { return mpc_stream_step_term_kernel; }
}  // namespace mpcb
