// mpc_step_term_sens.hip -- gfx950 kernels of the controller step with the joint-wise terminal cost that also returns the
// sensitivities of u0 (mpcb_step_term with sens, include/mpcbatch.h) on the latency engine: Engine<DevExec, true>::control_step<true,
// true>, the step of mpc_step_term.hip with Engine::sens_pass between the QP solve and the closing linearisation; the pass also
// forms d u0 / d x_e from the last stage of its recursion.
//
// A translation unit of its own for the reason given in mpc_step.hip.  Same geometries, dynamic-LDS pool, workspace and
// disable_tail_calls as mpc_step_kernel; mpcb_step_term launches these only when it is given a terminal cost and somewhere to write
// the sensitivities.
#include <hip/hip_runtime.h>

#include "mpc_core.h"
#include "mpc_devexec.h"

template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) __attribute__((disable_tail_calls)) void mpc_step_term_sens_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                        double *ws_base, size_t ws_stride, StepIO io, int reset, int pool_doubles)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>, true> eng(ex, c);
    eng.template control_step<true, true>(io, inst, reset != 0);
}

namespace mpcb {

const void *step_term_sens_kernel(int waves_per_sim, int wpe)
{
    return waves_per_sim == 8 ? (const void *)mpc_step_term_sens_kernel<8>
         : waves_per_sim == 4 ? (wpe == 2 ? (const void *)mpc_step_term_sens_kernel<4, 2> : (const void *)mpc_step_term_sens_kernel<4>)
         : waves_per_sim == 2 ? (const void *)mpc_step_term_sens_kernel<2> : (const void *)mpc_step_term_sens_kernel<1>;
}

void launch_step_term_sens(int waves_per_sim, int wpe, dim3 grid, size_t lds, hipStream_t s, const Problem &pb, const Robot &rb,
                      const InstParams *params, double *ws_base, size_t ws_stride, const StepIO &io, int reset, int pool_doubles)
{
    if (waves_per_sim == 8)
        hipLaunchKernelGGL(mpc_step_term_sens_kernel<8>, grid, dim3(WAVE * 8), lds, s, pb, rb, params, ws_base, ws_stride, io, reset, pool_doubles);
    else if (waves_per_sim == 4 && wpe == 2)
        hipLaunchKernelGGL((mpc_step_term_sens_kernel<4, 2>), grid, dim3(WAVE * 4), lds, s, pb, rb, params, ws_base, ws_stride, io, reset, pool_doubles);
    else if (waves_per_sim == 4)
        hipLaunchKernelGGL(mpc_step_term_sens_kernel<4>, grid, dim3(WAVE * 4), lds, s, pb, rb, params, ws_base, ws_stride, io, reset, pool_doubles);
    else if (waves_per_sim == 2)
        hipLaunchKernelGGL(mpc_step_term_sens_kernel<2>, grid, dim3(WAVE * 2), lds, s, pb, rb, params, ws_base, ws_stride, io, reset, pool_doubles);
    else
        hipLaunchKernelGGL(mpc_step_term_sens_kernel<1>, grid, dim3(WAVE), lds, s, pb, rb, params, ws_base, ws_stride, io, reset, pool_doubles);
}

}  // namespace mpcb
