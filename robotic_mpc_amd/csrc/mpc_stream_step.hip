// mpc_stream_step.hip -- gfx950 kernel of the controller step (mpcb_step, include/mpcbatch.h) on the THROUGHPUT engine: one step of
// the solve from caller-supplied feedback states, without the plant (se::control_step, mpc_stream.h).
//
// A translation unit of its own for the reason given in mpc_step.hip: in one module with the rollout kernels, an extra kernel renumbers
// the kernel ids the LDS lowering hands to every pass, and the existing kernels would change code.  Same launch shape as a plain
// mpc_stream_kernel<double> launch: one wavefront per simulation, MPCB_STREAM_WPE wavefronts per SIMD, grid = batch, static LDS
// (g_ssm) only.  No work queue: one launch is one step of every simulation.
//
// disable_tail_calls, as in mpc_step.hip: without it the optimizer marks the first calls to the passes `tail` (nothing local has escaped
// yet), and lin_pass then saves and restores its callee-saved registers on every call (224 scratch operations instead of 0).
#include <hip/hip_runtime.h>

#ifndef MPCB_STREAM_WPE
#define MPCB_STREAM_WPE 2
#endif
#include "mpc_launch.h"
#include "mpc_stream.h"

using namespace mpcb;

__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_step_kernel(Problem pb, const Robot *__restrict__ rbd,
                                                                                const InstParams *__restrict__ params, double *ws_base,
                                                                                size_t ws_stride, StepIO io, int reset)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    se::control_step<double>(pb, params, rbd, ws_base, ws_stride, io, inst, reset != 0);
#endif
}

namespace mpcb {
StreamStepFn stream_step_kernel() { return mpc_stream_step_kernel; }
}  // namespace mpcb
