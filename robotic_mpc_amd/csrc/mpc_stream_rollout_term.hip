// mpc_stream_rollout_term.hip -- gfx950 kernel of the rollout with the joint-wise terminal cost (mpcb_rollout_term, include/mpcbatch.h) on
// the THROUGHPUT engine: se::rollout<double, true, true, true> (mpc_stream.h), the perturbed rollout's closed loop with the TERM flag
// threaded through the step (as TERM_TABLE: the record is read from two arrays) -- every step's recursion starts from P_N = lm I + P, and its stage-N gradient, cost and stationarity rows
// take the terminal term (mpc_nlp.h term_*) against row t of the simulation's reference table.  On a ragged batch stage N is each
// simulation's own horizon end.  A `pert` whose three members are null is the nominal plant: one kernel serves both.
//
// A translation unit of its own for the reason given in mpc_step.hip.  The two launch shapes of mpc_stream_kernel (mpc_kernel.hip,
// where the protocol is described): one wavefront per simulation, or the work queue over (simulation, chunk of steps) items.  The
// pop / poll / release loop is REPEATED here as it is in mpc_stream_rollout_ref.hip, for the reason given there.  A change to the
// protocol is a change to all four.  What a work item hands to the next is what the perturbed rollout's hands on: the terminal cost
// adds nothing to it -- the next item reads its own rows of the table.  fp64 only.
//
// disable_tail_calls, as in mpc_stream_step.hip: the first pass of a step is called before anything local has escaped here as well.
#include <hip/hip_runtime.h>

#ifndef MPCB_STREAM_WPE
#define MPCB_STREAM_WPE 2
#endif
#include "mpc_stream.h"

using namespace mpcb;

// yref_sched: [batch][Nsim + N][NTASK], N = pb.N (the longest horizon of the batch); pert: the three [batch][...] arrays of
// mpcb_plant_pert (each may be null); term: blocks [batch][18] and x_ref [batch][Nsim][12] (neither null)
template <class FT>
__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) __attribute__((disable_tail_calls)) void mpc_stream_term_kernel(
    Problem pb, const Robot *__restrict__ rbd, const InstParams *__restrict__ params, double *ws_base, size_t ws_stride, Outputs out, int step0,
    int step1, int *queue, int chunk_steps, long long timeout_ticks, const double *__restrict__ yref_sched, PlantPert pert,
    TermTab term)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t rows = (size_t)pb.Nsim + pb.N;
    const bool queued = queue != nullptr;
    const int n_chunks = queued ? (step1 - step0 + chunk_steps - 1) / chunk_steps : 1;
    const int n_items = n_chunks * pb.batch;
    for (;;) {
        int inst = blockIdx.x, s0 = step0, s1 = step1, c = 0;
        if (queued) {
            int q = 0;
            if (threadIdx.x == 0) q = __hip_atomic_fetch_add(&queue[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            q = __builtin_amdgcn_readfirstlane(q);
            if (q >= n_items) break;
            c = q / pb.batch;
            inst = q - c * pb.batch;
            s0 = step0 + c * chunk_steps;
            s1 = s0 + chunk_steps < step1 ? s0 + chunk_steps : step1;
            if (c > 0) {
                int ok = 1;
                if (threadIdx.x == 0) {
                    const long long t_end = (long long)wall_clock64() + timeout_ticks;
                    while (__hip_atomic_load(&queue[2 + inst], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < c) {
                        if ((long long)wall_clock64() > t_end || __hip_atomic_load(&queue[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
                            __hip_atomic_store(&queue[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            ok = 0;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(32);
                    }
                }
                ok = __builtin_amdgcn_readfirstlane(ok);
                if (!ok) break;                                           // error flag set: every wavefront drains out
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");       // this CU's L1 may hold lines of an earlier chunk
                __builtin_amdgcn_s_waitcnt(0);
            }
        } else if (inst >= pb.batch) {
            break;
        }
        se::rollout<FT, true, true, true>(pb, params, rbd, ws_base, ws_stride, out, inst, s0, s1, yref_sched + (size_t)inst * rows * NTASK,
                                          plant_pert_of(pert, inst, pb.Nsim), term_tab_of(term, inst, pb.Nsim));
        if (!queued) break;
        __builtin_amdgcn_s_waitcnt(0);                                    // every store of this chunk has been acknowledged
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __builtin_amdgcn_s_waitcnt(0);
        if (threadIdx.x == 0) __hip_atomic_store(&queue[2 + inst], c + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#endif
}

namespace mpcb {

const void *stream_rollout_term_kernel() { return (const void *)mpc_stream_term_kernel<double>; }

void launch_stream_rollout_term(dim3 grid, hipStream_t s, const Problem &pb, const Robot *rbd, const InstParams *params, double *ws_base,
                                size_t ws_stride, const Outputs &out, int step0, int step1, int *queue, int chunk_steps,
                                long long timeout_ticks, const double *yref_sched, const PlantPert &pert, const TermTab &term)
{
    hipLaunchKernelGGL(mpc_stream_term_kernel<double>, grid, dim3(WAVE), 0, s, pb, rbd, params, ws_base, ws_stride, out, step0, step1, queue,
                       chunk_steps, timeout_ticks, yref_sched, pert, term);
}

}  // namespace mpcb
