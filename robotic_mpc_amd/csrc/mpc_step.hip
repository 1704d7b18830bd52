// mpc_step.hip -- gfx950 kernels of the controller step (mpcb_step, include/mpcbatch.h): the latency engine's solve from
// caller-supplied feedback states, without the plant (Engine::control_step).
//
// A translation unit of its own, so that the rollout and throughput kernels of mpc_kernel.hip compile to the same code as
// without it: in one module the extra kernels renumber the kernel ids the LDS lowering hands to every pass.  Same geometries
// (DevExec<NWV, WPE>), dynamic-LDS pool and workspace as mpc_rollout_kernel.
//
// disable_tail_calls: the passes (MPC_PASS, noinline, internal) are compiled without callee-saved registers -- the backend's
// interprocedural register allocation lets an internal, non-recursive function clobber them when no call to it is a tail call.
// The rollout kernel's calls never are (its step loop passes local arrays to the passes first).  Here the passes of the first
// QP come before any local escapes, the optimizer marks those calls `tail`, and every pass then saved and restored ~100 callee-
// saved VGPRs and SGPRs on each call (fwd_resident<8,1>: 94 scratch operations instead of 2; nlp_direct<8,1>: 240).  No call in
// this kernel is in tail position, so the marker buys nothing; without it the passes save no callee-saved registers.
#include <hip/hip_runtime.h>

#include "mpc_core.h"
#include "mpc_devexec.h"
#include "mpc_launch.h"

// One controller step of every instance: one workgroup of NWV wavefronts per instance, grid = batch.
template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) __attribute__((disable_tail_calls)) void mpc_step_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                        double *ws_base, size_t ws_stride, StepIO io, int reset, int pool_doubles)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>> eng(ex, c);
    eng.control_step(io, inst, reset != 0);
}

namespace mpcb {
StepFn step_kernel(int waves_per_sim, int wpe) { return MPCB_GEOMETRY_KERNEL(StepFn, mpc_step_kernel, waves_per_sim, wpe); }
}  // namespace mpcb
