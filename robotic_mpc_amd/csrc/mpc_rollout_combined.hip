// mpc_rollout_combined.hip -- gfx950 kernels of the rollout in which the terminal cost, the disturbance observer, the scheduled surface
// and the shift warm start are live at once (mpcb_rollout_combined, include/mpcbatch.h) on the latency engine:
// Engine<DevExec, TERM_TABLE, DIST_SHARED, 1>::rollout<true, true, true, true>, the perturbed rollout's closed loop on the engine built
// with all three of its flags.  Step t -- t the absolute step number, in every launch -- takes x_e from row t of the simulation's
// terminal table and its surface window from row t of its surface table, publishes the observer's d^_t into Smem (lv_dhat) and row t
// of the d_hat log, THEN shifts a simulation whose mode is MPCB_WARM_SHIFT (t >= 1; the tail takes u_{N-1} + d^_t), then solves.
//
// ONE instantiation per geometry, not one per subset: a simulation that does not use a feature runs with neutral data for it -- zero
// terminal blocks, observer gains l1 = l2 = 0 (d^ stays 0 and u + 0.0 is exact), a surface table whose rows all equal its own a..f,
// mode MPCB_WARM_CARRY.  The host fills those tables (mpcb_rollout_combined for a NULL argument, the Python layer per simulation);
// the kernel takes no branch on a null pointer, and mpc_neutral_surf_kernel below writes the one table that is not a constant fill.
//
// Nothing new carries between steps or launches: d^ crosses a launch in ST_OBS as in mpcb_rollout_obs; Smem, the pool and the workspace
// are those of every other kernel.  A translation unit of its own for the reason given in mpc_step.hip.  Same geometries as
// mpc_rollout_pert_kernel.  A `pert` whose three members are null is the nominal plant.
#include <hip/hip_runtime.h>

#include "mpc_core.h"
#include "mpc_devexec.h"
#include "mpc_launch.h"

// yref_sched: [batch][Nsim + N][NTASK], N = pb.N; pert: the three [batch][...] arrays of mpcb_plant_pert (each may be null);
// term: blocks [batch][18] and x_ref [batch][Nsim][12]; obs: gain [batch][12] (read) and d_hat [batch][Nsim][6] (written);
// surf_sched: [batch][Nsim + N][NSURF]; warm: [batch] of MPCB_WARM_* -- none of them null
template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) void mpc_rollout_combined_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                                    double *ws_base, size_t ws_stride, Outputs out, int step0,
                                                                    int step1, int pool_doubles, const double *__restrict__ yref_sched,
                                                                    PlantPert pert, TermTab term, ObsArg obs,
                                                                    const double *__restrict__ surf_sched, const int *__restrict__ warm)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>, TERM_TABLE, DIST_SHARED, 1> eng(ex, c);
    const size_t rows = (size_t)pb.Nsim + pb.N;
    const int mode = ex.uni(warm[inst]);
    eng.template rollout<true, true, true, true>(out, inst, step0, step1, yref_sched + (size_t)inst * rows * NTASK,
                                                 plant_pert_of(pert, inst, pb.Nsim), term_tab_of(term, inst, pb.Nsim),
                                                 obs_arg_of(obs, inst, pb.Nsim), surf_sched + (size_t)inst * rows * NSURF, mode);
}

// The neutral surface table: rows [0, rows) of simulation i all equal InstParams::coeffs of simulation i.  One thread per double.
__global__ __launch_bounds__(256) void mpc_neutral_surf_kernel(int batch, size_t rows, const InstParams *__restrict__ params, double *__restrict__ out)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x, per = rows * NSURF;
    if (e >= (size_t)batch * per) return;
    const size_t i = e / per;
    out[e] = params[i].coeffs[(e - i * per) % NSURF];
}

namespace mpcb {
RolloutCombinedFn rollout_combined_kernel(int waves_per_sim, int wpe)
{
    return MPCB_GEOMETRY_KERNEL(RolloutCombinedFn, mpc_rollout_combined_kernel, waves_per_sim, wpe);
}
void neutral_surf_fill(int batch, size_t rows, const InstParams *params, double *out, hipStream_t s)
{
    const size_t n = (size_t)batch * rows * NSURF;
    if (n == 0) return;
    hipLaunchKernelGGL(mpc_neutral_surf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, batch, rows, params, out);
}
}  // namespace mpcb
