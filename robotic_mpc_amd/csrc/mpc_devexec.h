// mpc_devexec.h -- DevExec<NWV, WPE>, the device executor of the latency engine (mpc_core.h), and the LDS it works in.
//
// Shared by the translation units that instantiate the engine template on the GPU: mpc_kernel.hip (rollout kernels, C ABI)
// and mpc_step.hip (controller step kernels).  Each is its own device code object with its own copy of the LDS objects.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "mpc_core.h"

using namespace mpcb;

// LDS of the workgroup (= one simulation): fixed working set + chunk pool.
__shared__ __attribute__((aligned(16))) Smem g_sm;
extern __shared__ __attribute__((aligned(16))) double g_pool[];

// Stateless on purpose: inside a non-inlined pass the executor is reached through `this`, and a
// data member (e.g. a cached lane id) would be re-loaded from the stack at every phase.
// NWV wavefronts (one workgroup) cooperate on one simulation.
#ifndef MPCB_POLL_SLEEP
#define MPCB_POLL_SLEEP 2
#endif

// WPE (wavefronts per SIMD the kernel is compiled for) only makes the executor -- and with it every pass of the
// engine template -- a distinct type per kernel variant, so each variant gets its own register allocation.
template <int NWV, int WPE = 1>
struct DevExec {
    static constexpr int NT = WAVE * NWV;
    static constexpr int VGPR_BUDGET = (WPE >= 2 || NWV > 4) ? 256 : 512;   // registers per lane this variant is compiled for (two wavefronts per SIMD: 256)
    __device__ __forceinline__ static int lane_id() { return (int)threadIdx.x; }
    __device__ __forceinline__ Smem &smem() const { return g_sm; }
    __device__ __forceinline__ double *pool() const { return g_pool; }
    // value known to be identical in every lane -> scalar register (and scalar control flow)
    __device__ __forceinline__ static int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
    __device__ __forceinline__ static bool uni(bool v) { return __builtin_amdgcn_readfirstlane((int)v) != 0; }
    __device__ __forceinline__ static double uni(double v)
    {
        return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
    }
    template <class T>
    __device__ __forceinline__ static T *uni(T *p)
    {
        const unsigned long long v = (unsigned long long)p;
        const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
        const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
        return (T *)(((unsigned long long)hi << 32) | lo);
    }
    // per-lane registers that live across phases
    template <class T>
    struct PerLane {
        T v;
        __device__ __forceinline__ T &at(int) { return v; }
    };
    __device__ __forceinline__ static void wave_fence()
    {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    // phase on all NT lanes, then a workgroup barrier (a wave-local fence when one wave owns the sim)
    template <class F>
    __device__ __forceinline__ void par(F &&f)
    {
        f(lane_id());
        if (NWV == 1) wave_fence();
        else __syncthreads();
    }
    // wave-local phase on EVERY wavefront, no workgroup barrier: consecutive wpar phases of one wavefront see each
    // other's LDS writes (in-order LDS); data of another wavefront needs a barrier() first
    template <class F>
    __device__ __forceinline__ void wpar(F &&f)
    {
        f(lane_id());
        wave_fence();
    }
    __device__ __forceinline__ static void barrier()
    {
        if (NWV == 1) wave_fence();
        else __syncthreads();
    }
    // phase on wavefront 0 only; consecutive seq phases need no s_barrier (one wave, in-order LDS)
    template <class F>
    __device__ __forceinline__ void seq(F &&f)
    {
        if (NWV == 1 || threadIdx.x < WAVE) {
            f(lane_id());
            wave_fence();
        }
    }
    // A stage-by-stage recursion (`fg`, made of seq phases, wavefront 0) with the other wavefronts
    // doing barrier-free background work `bg(lane, lanes)` (chunk copies for the neighbouring
    // chunks) in its shadow; ends with the workgroup barrier.  With one wavefront per simulation
    // the two simply run one after the other.
    template <class FG, class BG>
    __device__ __forceinline__ void overlap(FG &&fg, BG &&bg)
    {
        if (NWV == 1) {
            fg();
            wave_fence();
            bg(lane_id(), std::integral_constant<int, WAVE>{});
            wave_fence();
        } else {
            if (threadIdx.x < WAVE) fg();
            else bg(lane_id() - WAVE, std::integral_constant<int, WAVE *(NWV > 1 ? NWV - 1 : 1)>{});
            __syncthreads();
        }
    }
    // Three concurrent roles: wavefront 0 runs `fg` (seq phases), wavefront 1 runs `mid` (sub
    // phases, wave-local), the remaining wavefronts run the barrier-free `bg(lane, lanes)`.
    // With fewer wavefronts the roles run one after the other on the last wavefront.
    template <class FG, class MID, class BG>
    __device__ __forceinline__ void overlap3(FG &&fg, MID &&mid, BG &&bg)
    {
        if (NWV == 1) {
            fg(); wave_fence();
            mid(); wave_fence();
            bg(lane_id(), std::integral_constant<int, WAVE>{});
            wave_fence();
        } else if (NWV == 2) {
            if (threadIdx.x < WAVE) fg();
            else { mid(); wave_fence(); bg(lane_id() - WAVE, std::integral_constant<int, WAVE>{}); }
            __syncthreads();
        } else {
            if (threadIdx.x < WAVE) fg();
            else if (threadIdx.x < 2 * WAVE) mid();
            else bg(lane_id() - 2 * WAVE, std::integral_constant<int, WAVE *(NWV > 2 ? NWV - 2 : 1)>{});
            __syncthreads();
        }
    }
    // A loop of `nwin` windows of three roles WITHOUT workgroup barriers between the windows (four wavefronts and more):
    // every role runs its own loop and the roles meet through LDS counters (post / post_add / await) only; one barrier at
    // the end.  With fewer wavefronts (roles share a wavefront) each window is an overlap3 with its barrier.
    static constexpr int BG_WAVES = NWV > 2 ? NWV - 2 : 1;
    template <class FG, class MID, class BG>
    __device__ __forceinline__ void pipeline3(int nwin, FG &&fg, MID &&mid, BG &&bg)
    {
        if (NWV >= 4) {
            if (threadIdx.x < WAVE) { for (int ci = 0; ci < nwin; ci++) fg(ci); }
            else if (threadIdx.x < 2 * WAVE) { for (int ci = 0; ci < nwin; ci++) mid(ci); }
            else { for (int ci = 0; ci < nwin; ci++) { bg(ci, lane_id() - 2 * WAVE, std::integral_constant<int, WAVE * BG_WAVES>{}); wave_fence(); } }
            __syncthreads();
        } else {
            for (int ci = 0; ci < nwin; ci++)
                overlap3([&]() { fg(ci); }, [&]() { mid(ci); }, [&](int lane, auto nl) { bg(ci, lane, nl); });
        }
    }
    __device__ __forceinline__ static void post_add(int *flag, int v)
    {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __hip_atomic_fetch_add(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // progress counter between the recursion wavefront and the one following it (LDS, same CU):
    // a wavefront's LDS operations complete in issue order, so data written before post() is
    // visible to whoever has seen the posted value.
    __device__ __forceinline__ static void post(int *flag, int v)
    {
        // compiler-only ordering: the LDS unit executes one wavefront's DS instructions in issue order,
        // so no s_waitcnt is needed between the data writes and the flag write
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ static void await(int *flag, int v)
    {
        if (NWV > 1) {   // with a single wavefront the recursion has finished before the follower starts
            while (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < v) __builtin_amdgcn_s_sleep(MPCB_POLL_SLEEP);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // one step of a recursion that runs on a single wavefront inside overlap3's `mid`
    template <class F>
    __device__ __forceinline__ void sub(F &&f)
    {
        f(lane_id() & (WAVE - 1));
        wave_fence();
    }
    // ---- values handed from lane to lane between consecutive seq phases (registers, no LDS) ----
    // share(): publish this lane's value for the next phase (a register stays a register here);
    // gather(j): the value lane j published; shl6 / shr6: the value of lane + 6 / lane - 6
    // (DPP row shifts, rows of 16 lanes; used by lanes < 12 only).
    __device__ __forceinline__ static void share(double *, int, double) {}
    __device__ __forceinline__ static double gather(const double *, int j, double mine) { return row_lane(mine, j); }
    // entry `idx` of a small LDS array whose 16-byte item l lane l of this wavefront has just read (`mine` = the half
    // holding the entry, `src` = idx / 2): a scalar here; the host executor reads the array
    __device__ __forceinline__ static double lane_value(const double *, int, double mine, int src) { return row_lane(mine, src); }
    __device__ __forceinline__ static double shl6(const double *, int, double mine) { return dpp<0x106>(mine); }
    __device__ __forceinline__ static double shr6(const double *, int, double mine) { return dpp<0x116>(mine); }
    // ---- reductions over the NT lanes of a simulation ------------------------------------
    // put_*: called by every lane at the end of a par phase; the wavefront reduces its 64 values
    // with DPP row operations (no LDS round trips) and leaves one partial per wavefront in r[].
    // get_*: after the phase barrier, combines the NWV partials (same order in every lane).
    template <int CTRL>
    __device__ __forceinline__ static double dpp(double v)
    {
        const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);
        const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);
        return __hiloint2double(hi, lo);
    }
    __device__ __forceinline__ static double row_lane(double v, int l)
    {
        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
    }
    template <class Op>
    __device__ __forceinline__ static double wave_reduce(double v, Op op)
    {
        v = op(v, dpp<0xB1>(v));    // quad_perm [1,0,3,2]
        v = op(v, dpp<0x4E>(v));    // quad_perm [2,3,0,1]
        v = op(v, dpp<0x141>(v));   // row_half_mirror
        v = op(v, dpp<0x140>(v));   // row_mirror: every lane of a row of 16 holds the row result
        return op(op(row_lane(v, 0), row_lane(v, 16)), op(row_lane(v, 32), row_lane(v, 48)));
    }
    struct OpSum { __device__ __forceinline__ double operator()(double a, double b) const { return a + b; } };
    struct OpMax { __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); } };
    struct OpMin { __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); } };
    template <class Op>
    __device__ __forceinline__ static void put(double *r, int lane, double v, Op op)
    {
        const double t = wave_reduce(v, op);
        if ((lane & (WAVE - 1)) == 0) r[lane >> 6] = t;
    }
    __device__ __forceinline__ static void put_sum(double *r, int lane, double v) { put(r, lane, v, OpSum()); }
    __device__ __forceinline__ static void put_max(double *r, int lane, double v) { put(r, lane, v, OpMax()); }
    __device__ __forceinline__ static void put_min(double *r, int lane, double v) { put(r, lane, v, OpMin()); }
    template <class Op>
    __device__ __forceinline__ static double get(const double *r, Op op)
    {
        double tot = r[0];
#pragma unroll
        for (int w = 1; w < NWV; w++) tot = op(tot, r[w]);
        return uni(tot);
    }
    // single-wavefront variants (inside overlap3's `mid`): one result in r[0]
    __device__ __forceinline__ static void put1_sum(double *r, int lane, double v) { const double t = wave_reduce(v, OpSum()); if (lane == 0) r[0] = t; }
    __device__ __forceinline__ static void put1_min(double *r, int lane, double v) { const double t = wave_reduce(v, OpMin()); if (lane == 0) r[0] = t; }
    __device__ __forceinline__ static double get1(const double *r) { return uni(r[0]); }
    __device__ __forceinline__ static double get_sum(const double *r) { return get(r, OpSum()); }
    // per-wavefront partial sums (put_sum leaves exactly those) and the sum over wavefronts [w0, w0 + n)
    __device__ __forceinline__ static void put_wsum(double *r, int lane, double v) { put(r, lane, v, OpSum()); }
    __device__ __forceinline__ static double get_sum_range(const double *r, int w0, int n)
    {
        double tot = r[w0];
        for (int w = 1; w < n; w++) tot += r[w0 + w];
        return uni(tot);
    }
    __device__ __forceinline__ static double get_max(const double *r) { return get(r, OpMax()); }
    __device__ __forceinline__ static double get_min(const double *r) { return get(r, OpMin()); }
    // constant 100 MHz counter (s_memrealtime)
    __device__ __forceinline__ double clock() { return (double)wall_clock64() * 1e-8; }
};
