// mpc_stream_step_combined.hip -- gfx950 kernel of the controller step in which the terminal cost, the input disturbance, the surface
// window and the per-simulation warm start are in force at once (mpcb_step_combined, include/mpcbatch.h) on the THROUGHPUT engine:
// se::control_step<double, true, false, false, true, true, true>, one mpc_step carrying TermArg<1>, DistArg<1> and the SURF passes,
// after shift_pass<false, 1> for a simulation whose mode is MPCB_WARM_SHIFT.  On a ragged batch the terminal cost sits on each
// simulation's own last stage, and the reference and surface windows are strided by the batch's longest horizon.
//
// One kernel, not one per subset: a simulation that does not use a feature brings neutral data for it, which the host fills
// (mpc_rollout_combined.hip).  No sensitivities.
//
// A translation unit of its own, like mpc_stream_step.hip and for the same reason.  Same launch shape, static LDS and
// disable_tail_calls.
#include <hip/hip_runtime.h>

#ifndef MPCB_STREAM_WPE
#define MPCB_STREAM_WPE 2
#endif
#include "mpc_launch.h"
#include "mpc_stream.h"

using namespace mpcb;

// io.term [batch][NTERM], io.dist [batch][6], io.surf [batch][NMAX][NSURF]: not null; io.warm: [batch] or null (carry)
__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_step_combined_kernel(Problem pb, const Robot *__restrict__ rbd,
                                                                                const InstParams *__restrict__ params, double *ws_base,
                                                                                size_t ws_stride, StepIO io, int reset)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    se::control_step<double, true, false, false, true, true, true>(pb, params, rbd, ws_base, ws_stride, io, inst, reset != 0);
#endif
}

namespace mpcb {
StreamStepFn stream_step_combined_kernel() { return mpc_stream_step_combined_kernel; }
}  // namespace mpcb
