// mpc_stream_queue.h -- the launch loop of the throughput engine's rollout kernels (mpc_stream_kernel in mpc_kernel.hip and the kernels of
// mpc_stream_rollout_{ref,pert,term}.hip), written once.
//
// Two launch shapes:
//   * one workgroup per simulation, all of [step0, step1) (queue == nullptr);
//   * WORK QUEUE (batch larger than the wavefronts resident at once): the grid is the resident set, every wavefront
//     pops items (simulation, chunk of `chunk_steps` closed-loop steps) off an atomic counter, chunk-major -- all
//     simulations advance together, fast wavefronts take more items, and the launch ends within one chunk of the
//     balanced time instead of with the slowest pair of whole simulations.  Chunk c of a simulation follows chunk c-1,
//     which may have run on any CU: the finishing wavefront releases (stores drained, agent-scope release, progress
//     counter), the next one polls the counter and acquires (MI355X_MICROARCH.md, hand-off recipe).  An item's
//     predecessor was popped earlier, so it is running or done: no wavefront ever waits for work nobody has taken.  A
//     bounded poll (`timeout_ticks` of the 100 MHz clock, queue_timeout_ticks in mpc_kernel.hip) turns a broken hand-off into an
//     error flag, never a hang.
//   queue[0] item counter, queue[1] error flag, queue[2 + i] chunks of simulation i done in this launch.
// The bound is a bug guard, not a schedule: a waiting item's predecessor is always running, so it is sized from the WORK LIMIT of
// one chunk (queue_timeout_ticks), never from typical times -- a legitimately slow chunk (full SQP at a long horizon, every
// QP running to qp_solver_iter_max) must not trip it and take the whole bucket down.
//
// A MACRO over the body, not a function template: the template compiled mpc_stream_kernel to other code than the loop written out
// does (same resources, other schedule); the macro hands the compiler the tokens it had before.  It expands in a kernel whose
// parameters are named pb, step0, step1, queue, chunk_steps and timeout_ticks; the argument is the call that runs steps [s0, s1) of
// simulation `inst`.  In the poll, a set error flag makes every wavefront drain out; the acquire is there because this CU's L1 may
// hold lines of an earlier chunk; the release follows a wait for the acknowledgement of every store of the chunk.
#pragma once

#define MPCB_STREAM_QUEUE_LOOP(...)                                                                                                  \
    const bool queued = queue != nullptr;                                                                                            \
    const int n_chunks = queued ? (step1 - step0 + chunk_steps - 1) / chunk_steps : 1;                                               \
    const int n_items = n_chunks * pb.batch;                                                                                         \
    for (;;) {                                                                                                                       \
        int inst = blockIdx.x, s0 = step0, s1 = step1, c = 0;                                                                        \
        if (queued) {                                                                                                                \
            int q = 0;                                                                                                               \
            if (threadIdx.x == 0) q = __hip_atomic_fetch_add(&queue[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);              \
            q = __builtin_amdgcn_readfirstlane(q);                                                                                   \
            if (q >= n_items) break;                                                                                                 \
            c = q / pb.batch;                                                                                                        \
            inst = q - c * pb.batch;                                                                                                 \
            s0 = step0 + c * chunk_steps;                                                                                            \
            s1 = s0 + chunk_steps < step1 ? s0 + chunk_steps : step1;                                                                \
            if (c > 0) {                                                                                                             \
                int ok = 1;                                                                                                          \
                if (threadIdx.x == 0) {                                                                                              \
                    const long long t_end = (long long)wall_clock64() + timeout_ticks;                                               \
                    while (__hip_atomic_load(&queue[2 + inst], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < c) {                    \
                        if ((long long)wall_clock64() > t_end ||                                                                     \
                            __hip_atomic_load(&queue[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {                         \
                            __hip_atomic_store(&queue[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                            \
                            ok = 0;                                                                                                  \
                            break;                                                                                                   \
                        }                                                                                                            \
                        __builtin_amdgcn_s_sleep(32);                                                                                \
                    }                                                                                                                \
                }                                                                                                                    \
                ok = __builtin_amdgcn_readfirstlane(ok);                                                                             \
                if (!ok) break;                                                                                                      \
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");                                                                   \
                __builtin_amdgcn_s_waitcnt(0);                                                                                       \
            }                                                                                                                        \
        } else if (inst >= pb.batch) {                                                                                               \
            break;                                                                                                                   \
        }                                                                                                                            \
        __VA_ARGS__;                                                                                                                 \
        if (!queued) break;                                                                                                          \
        __builtin_amdgcn_s_waitcnt(0);                                                                                               \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");                                                                           \
        __builtin_amdgcn_s_waitcnt(0);                                                                                               \
        if (threadIdx.x == 0) __hip_atomic_store(&queue[2 + inst], c + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);               \
    }
