// mpc_kernel.hip -- gfx950 kernel + C ABI (include/mpcbatch.h) of the batched MPC engine.
//
// Launch geometry: one workgroup of NWV wavefronts (1, 2, 4 or 8; mpcb_setup picks it from the
// batch) per simulation instance, grid = batch.  DevExec<NWV> (mpc_devexec.h) is the device executor of the
// engine template (mpc_core.h): workgroup barriers between bulk-synchronous phases, wave-local
// fences inside a recursion, role-split windows (overlap3), DPP/readlane cross-lane helpers.
#include <hip/hip_runtime.h>
#include <type_traits>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/mpcbatch.h"
#include "mpc_core.h"
#include "mpc_devexec.h"
#include "mpc_launch.h"
#include "mpc_pack.h"
#include "mpc_stream.h"
#include "mpc_stream_queue.h"

using namespace mpcb;

static_assert(sizeof(mpcb_problem) == sizeof(Problem), "ABI struct mismatch");
static_assert(sizeof(mpcb_result) == sizeof(Outputs), "ABI struct mismatch");
static_assert(offsetof(StepIO, yref) == sizeof(mpcb_step_io), "ABI struct mismatch: StepIO is mpcb_step_io + the task reference");
static_assert(MPCB_NREF == NTASK, "task reference width");
static_assert(sizeof(Robot) == MPCB_NROBOT * sizeof(double), "robot layout");

// The kernels of the controller step and of the rollout variants live in translation units of their own (mpc_step.hip says why:
// instantiated here, next to the rollout kernels, they change the rollout kernels' code).  mpc_launch.h declares the getter of each.

// WPE = 1: one wavefront per SIMD owns the whole 512-entry register file (one simulation per CU: batch <= #CUs, and
// the 1 / 2 / 8-wavefront geometries).  WPE = 2: 256 registers, two 4-wavefront simulations resident per CU -- the
// geometry of batches beyond one simulation per CU (measured at batch 4096, N = 100: 540 k steps/s against 468 k for
// two 2-wavefront simulations per CU at 512 registers).
template <int NWV, int WPE = 1>
__global__ __launch_bounds__(WAVE *NWV, WPE) void mpc_rollout_kernel(Problem pb, Robot rb, const InstParams *__restrict__ params,
                                                           double *ws_base, size_t ws_stride, Outputs out, int step0,
                                                           int step1, int pool_doubles)
{
    const int inst = blockIdx.x;
    if (inst >= pb.batch) return;
    DevExec<NWV, WPE> ex;
    load_constants(ex, params + inst, &rb);
    Ctx c{&pb, ws_carve(ws_base + (size_t)inst * ws_stride, pb.N), pool_doubles, pb.N};
    Engine<DevExec<NWV, WPE>> eng(ex, c);
    eng.rollout(out, inst, step0, step1);
}

// THROUGHPUT engine (mpc_stream.h): one wavefront = one workgroup = one simulation, MPCB_STREAM_WPE wavefronts per SIMD.
#ifndef MPCB_STREAM_WPE
#define MPCB_STREAM_WPE 2
#endif
// The launch loop -- one workgroup per simulation, or the work queue over (simulation, chunk of steps) items -- is
// mpc_stream_queue.h's, shared with the rollout variants of this engine.
template <class FT>
__global__ __launch_bounds__(WAVE, MPCB_STREAM_WPE) void mpc_stream_kernel(Problem pb, const Robot *__restrict__ rbd, const InstParams *__restrict__ params,
                                                                           double *ws_base, size_t ws_stride, Outputs out, int step0, int step1,
                                                                           int *queue, int chunk_steps, long long timeout_ticks)
{
#if defined(__HIP_DEVICE_COMPILE__)
    MPCB_STREAM_QUEUE_LOOP(se::rollout<FT>(pb, params, rbd, ws_base, ws_stride, out, inst, s0, s1))
#endif
}

// Per-simulation summary of Simulator.get_summary (simulator.py:509-547) from the device logs: one wavefront per
// simulation streams its error rows and per-step statistics once (HBM-bound, coalesced).  out[MPCB_NSUMMARY]:
//   [0..4] rmse e1..e5  [5..9] itse e1..e5  [10] weighted_rmse  [11] total_sqp_iterations  [12] avg_sqp_iterations
//   [13] num_failures  [14] max_kkt_residual  [15] total_solver_time  [16] avg_mpc_time  [17] avg_solver_time
//   [18] avg_integration_time  [19] total_computation_time  [20] total_qp_iterations  [21..23] reserved
__global__ __launch_bounds__(WAVE) void mpc_summary_kernel(int batch, int Nsim, const InstParams *__restrict__ params, Outputs o,
                                                           double *__restrict__ summary)
{
    const int inst = blockIdx.x, lane = threadIdx.x;
    if (inst >= batch) return;
    const int T1 = Nsim + 1;
    const double dt = params[inst].dt;
    double se[5] = {0, 0, 0, 0, 0}, st[5] = {0, 0, 0, 0, 0};
    for (int c = lane; c < T1; c += WAVE) {
        const double tk = c * dt;                                    // simulator.py:367
#pragma unroll
        for (int j = 0; j < 5; j++) {
            const double e = o.errors[((size_t)inst * 7 + j) * T1 + c];
            se[j] += e * e;
            st[j] += tk * e * e;                                     // :368
        }
    }
    double sq = 0, qp = 0, fail = 0, kkt = 0, tsol = 0, tpl = 0, anynan = 0;   // (np.max propagates NaN, fmax drops it: flag)
    for (int i = lane; i < Nsim; i += WAVE) {
        const size_t k = (size_t)inst * Nsim + i;
        sq += o.sqp_iter[k]; qp += o.qp_iter[k]; fail += o.status[k] != 0 ? 1.0 : 0.0;
        tsol += o.solver_time[k]; tpl += o.plant_time[k];
        const double *r = o.residuals + k * 4;
        kkt = fmax(kkt, fmax(fmax(r[0], r[1]), fmax(r[2], r[3])));    // :402
        anynan += (r[0] != r[0] || r[1] != r[1] || r[2] != r[2] || r[3] != r[3]) ? 1.0 : 0.0;
    }
    using X = DevExec<1>;
    double wsum = 0.0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        se[j] = X::wave_reduce(se[j], X::OpSum());
        st[j] = X::wave_reduce(st[j], X::OpSum());
        wsum += params[inst].w_task[j] * se[j];                      // :383-384 (weights 50 each)
    }
    sq = X::wave_reduce(sq, X::OpSum()); qp = X::wave_reduce(qp, X::OpSum()); fail = X::wave_reduce(fail, X::OpSum());
    tsol = X::wave_reduce(tsol, X::OpSum()); tpl = X::wave_reduce(tpl, X::OpSum()); kkt = X::wave_reduce(kkt, X::OpMax());
    anynan = X::wave_reduce(anynan, X::OpSum());
    if (anynan > 0) kkt = __builtin_nan("");     // a diverged simulation (NaN residuals) must show in max_kkt_residual, as in the reference
    if (lane == 0) {
        double *s = summary + (size_t)inst * MPCB_NSUMMARY;
        for (int j = 0; j < 5; j++) { s[j] = sqrt(se[j] / T1); s[5 + j] = st[j] * dt; }
        s[10] = sqrt(wsum / T1);
        s[11] = sq; s[12] = sq / Nsim; s[13] = fail; s[14] = kkt; s[15] = tsol;
        // mpc_time (simulator.py:209-214) = the device time of the solve, integration_time (:224-226) = plant step + logging
        s[16] = tsol / Nsim; s[17] = tsol / Nsim; s[18] = tpl / Nsim; s[19] = tsol + tpl;
        s[20] = qp; s[21] = s[22] = s[23] = 0.0;
    }
}

// Run-time cost weights (mpcb_set_weights): the seven weight fields of every simulation's parameter record <- weights [batch][NWEIGHT]
// (mpc_layout.h put_weights).  One lane per simulation; plain vector stores.
__global__ __launch_bounds__(WAVE) void mpc_set_weights_kernel(int batch, InstParams *__restrict__ params, const double *__restrict__ weights)
{
    const int i = blockIdx.x * WAVE + threadIdx.x;
    if (i >= batch) return;
    double w[NWEIGHT];
#pragma unroll
    for (int p = 0; p < NWEIGHT; p++) w[p] = weights[(size_t)i * NWEIGHT + p];
    put_weights(params[i], w);
}

// Diagnostic entry (tests): the device linearisation task_lin on n points, one lane each.
__global__ void mpc_debug_task_lin_kernel(int n, Robot rb, const InstParams *__restrict__ params, const double *__restrict__ x,
                                          double *__restrict__ rec)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double xx[12], out[W2_LIN];
    for (int j = 0; j < 12; j++) xx[j] = x[(size_t)i * 12 + j];
    for (int j = 0; j < W2_LIN; j++) out[j] = 0.0;
    task_lin<true>(rb, params[i], xx, xx + 6, out);
    for (int j = 0; j < W2_LIN; j++) rec[(size_t)i * W2_LIN + j] = out[j];
}

// ------------------------------------------------------------------------------------ host
// The variants of the controller step and the kinds of rollout; each is one kernel (family) per engine, see with_kernel below.
enum StepVariant { STEP_BASE, STEP_WARM, STEP_SENS, STEP_SENSW, STEP_TERM, STEP_TERM_SENS, STEP_DIST, STEP_SURF, STEP_COMBINED };
enum RolloutKind { ROLLOUT_BASE, ROLLOUT_REF, ROLLOUT_PERT, ROLLOUT_TERM, ROLLOUT_OBS, ROLLOUT_SURF, ROLLOUT_SHIFT, ROLLOUT_SHIFT_SURF, ROLLOUT_COMBINED };

struct mpcb_handle {
    int device = -1;
    std::string err;
    Problem pb{};
    Robot rb{};
    bool ready = false;
    int next_step = 0;
    InstParams *d_params = nullptr;
    Robot *d_rb = nullptr;     // robot record in device memory (behind the parameter records)
    size_t params_cap = 0;
    double *d_ws = nullptr;
    size_t ws_cap = 0;
    size_t ws_stride = 0;
    int pool_doubles = POOL_DEFAULT_DOUBLES;
    int num_cus = 256;
    int waves_per_sim = 4;
    int wpe = 1;               // latency engine: kernel variant compiled for this many wavefronts per SIMD
    int engine = 0;            // 0: latency engine (mpc_core.h), 1: throughput engine (mpc_stream.h)
    int *d_queue = nullptr;    // throughput engine, work-queue launches: counter, error flag, per-simulation progress
    size_t queue_cap = 0;
    bool queue_used = false;   // the last launch went through the work queue (mpcb_sync checks its error flag)
    RolloutKind last_rollout = ROLLOUT_BASE;   // of the last rollout launch (mpcb_kernel_info reports its kernel)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipStream_t last_stream = nullptr;
    bool timed = false;
    bool controller = false;   // set up by mpcb_setup_controller: mpcb_step only (no rollouts)
    bool reset_next = false;   // the next mpcb_step starts from the initial guess whatever its flag says
    bool weights_changed = false;   // mpcb_set_weights since the last step: the carried linearisation is stale (as after ref_changed)
    double *d_neutral = nullptr;    // mpcb_step_combined / mpcb_rollout_combined: the neutral tables of the features given as NULL
    size_t neutral_cap = 0;         // (allocated on the first such call, never part of the workspace)
    size_t neutral_layout[5] = {0, 0, 0, 0, 0};   // what the block holds: entry (1 rollout, 2 step) and the doubles of its four runs;
                                    // {0, ..}: nothing -- mpcb_setup* invalidates it (the surface rows are the packed a..f)
};

static int fail(mpcb_handle *h, int code, const char *what, hipError_t e = hipSuccess)
{
    if (h) {
        h->err = what;
        if (e != hipSuccess) { h->err += ": "; h->err += hipGetErrorString(e); }
    }
    return code;
}
#define HIPCHK(h, call)                                                   \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) return fail((h), MPCB_EHIP, #call, e_);      \
    } while (0)

static int check_problem(mpcb_handle *h, const mpcb_problem *p)
{
    if (!p) return fail(h, MPCB_EINVAL, "problem is NULL");
    if (p->batch < 1) return fail(h, MPCB_EINVAL, "batch must be >= 1");
    if (p->N < 1 || p->N > 4096) return fail(h, MPCB_EINVAL, "prediction horizon N out of range [1,4096]");
    if (p->Nsim < 1) return fail(h, MPCB_EINVAL, "Nsim must be >= 1");
    if (p->solver_type != MPCB_SOLVER_SQP && p->solver_type != MPCB_SOLVER_SQP_RTI)
        return fail(h, MPCB_EINVAL, "solver_type must be MPCB_SOLVER_SQP or MPCB_SOLVER_SQP_RTI");
    if (p->max_iter < 1 || p->qp_iter_max < 1) return fail(h, MPCB_EINVAL, "iteration limits must be >= 1");
    if (p->precision != MPCB_PRECISION_FP64 && p->precision != MPCB_PRECISION_FP32_RICCATI)
        return fail(h, MPCB_EINVAL, "precision must be MPCB_PRECISION_FP64 or MPCB_PRECISION_FP32_RICCATI");
    if (p->precision == MPCB_PRECISION_FP32_RICCATI && p->solver_type != MPCB_SOLVER_SQP_RTI)
        return fail(h, MPCB_EINVAL, "the fp32 Riccati leg is validated for SQP_RTI only");
    return MPCB_OK;
}

// ---- the launch path: (handle, variant) -> kernel -> one launch site per signature, between the handle's two events
// the kernels of mpcb_rollout are this unit's own (the order of these two functions is the order of the kernels in the module)
static RolloutFn rollout_kernel(int waves_per_sim, int wpe) { return MPCB_GEOMETRY_KERNEL(RolloutFn, mpc_rollout_kernel, waves_per_sim, wpe); }
static StreamRolloutFn stream_rollout_kernel(int precision)
{
    return precision == MPCB_PRECISION_FP32_RICCATI ? mpc_stream_kernel<float> : mpc_stream_kernel<double>;
}

// The kernel that runs a step variant, or a kind of rollout, on the handle's engine and geometry: calls f with its typed pointer
// (mpc_launch.h) and returns what f returns.  The launch, the LDS ceiling and mpcb_kernel_info all ask here.
template <class F>
static int with_kernel(const mpcb_handle *h, StepVariant v, F &&f)
{
    const int nw = h->waves_per_sim, wpe = h->wpe;
    if (h->engine == 1)
        return f(v == STEP_COMBINED  ? stream_step_combined_kernel()
                 : v == STEP_SURF    ? stream_step_surf_kernel()
                 : v == STEP_DIST    ? stream_step_dist_kernel()
                 : v == STEP_TERM_SENS ? stream_step_term_sens_kernel() : v == STEP_TERM ? stream_step_term_kernel()
                 : v == STEP_SENSW   ? stream_step_sensw_kernel()     : v == STEP_SENS ? stream_step_sens_kernel()
                 : v == STEP_WARM    ? stream_step_warm_kernel()      : stream_step_kernel());
    return f(v == STEP_COMBINED  ? step_combined_kernel(nw, wpe)
             : v == STEP_SURF    ? step_surf_kernel(nw, wpe)
             : v == STEP_DIST    ? step_dist_kernel(nw, wpe)
             : v == STEP_TERM_SENS ? step_term_sens_kernel(nw, wpe) : v == STEP_TERM ? step_term_kernel(nw, wpe)
             : v == STEP_SENSW   ? step_sensw_kernel(nw, wpe)     : v == STEP_SENS ? step_sens_kernel(nw, wpe)
             : v == STEP_WARM    ? step_warm_kernel(nw, wpe)      : step_kernel(nw, wpe));
}
template <class F>
static int with_kernel(const mpcb_handle *h, RolloutKind kind, F &&f)
{
    const int nw = h->waves_per_sim, wpe = h->wpe;
    if (h->engine == 1)
        return kind == ROLLOUT_COMBINED ? f(stream_rollout_combined_kernel())
             : kind == ROLLOUT_SHIFT || kind == ROLLOUT_SHIFT_SURF ? f(stream_rollout_shift_kernel(kind == ROLLOUT_SHIFT_SURF))
             : kind == ROLLOUT_SURF ? f(stream_rollout_surf_kernel())
             : kind == ROLLOUT_OBS  ? f(stream_rollout_obs_kernel())
             : kind == ROLLOUT_TERM ? f(stream_rollout_term_kernel()) : kind == ROLLOUT_PERT ? f(stream_rollout_pert_kernel())
             : kind == ROLLOUT_REF  ? f(stream_rollout_ref_kernel())  : f(stream_rollout_kernel(h->pb.precision));
    return kind == ROLLOUT_COMBINED ? f(rollout_combined_kernel(nw, wpe))
         : kind == ROLLOUT_SHIFT || kind == ROLLOUT_SHIFT_SURF ? f(rollout_shift_kernel(nw, wpe, kind == ROLLOUT_SHIFT_SURF))
         : kind == ROLLOUT_SURF ? f(rollout_surf_kernel(nw, wpe))
         : kind == ROLLOUT_OBS  ? f(rollout_obs_kernel(nw, wpe))
         : kind == ROLLOUT_TERM ? f(rollout_term_kernel(nw, wpe)) : kind == ROLLOUT_PERT ? f(rollout_pert_kernel(nw, wpe))
         : kind == ROLLOUT_REF  ? f(rollout_ref_kernel(nw, wpe))  : f(rollout_kernel(nw, wpe));
}

// what a launch passes besides the handle's own state; each signature takes the members it declares
struct StepArgs { StepIO io; int reset; };
struct RolloutArgs {
    unsigned grid; Outputs out; int step0, step1;
    int *queue; int chunk_steps; long long timeout_ticks;   // throughput engine
    const double *yref_sched; PlantPert pert; TermTab term; ObsArg obs;  // ref / pert / term / obs
    const double *surf_sched;                                            // surf
    const int *warm;                                                     // shift
};

// Every kernel starts (pb, robot record, params, ws_base, ws_stride).  Latency engine: the record by value, a workgroup of
// waves_per_sim wavefronts, the dynamic-LDS pool.  Throughput engine: the record in device memory, one wavefront, static LDS only.
template <class K, class... A>
static void latency_launch(K k, const mpcb_handle *h, unsigned grid, hipStream_t s, const A &...a)
{
    hipLaunchKernelGGL(k, dim3(grid), dim3(WAVE * h->waves_per_sim), (size_t)h->pool_doubles * sizeof(double), s, h->pb, h->rb, h->d_params,
                       h->d_ws, h->ws_stride, a...);
}
template <class K, class... A>
static void stream_launch(K k, const mpcb_handle *h, unsigned grid, hipStream_t s, const A &...a)
{
    hipLaunchKernelGGL(k, dim3(grid), dim3(WAVE), 0, s, h->pb, h->d_rb, h->d_params, h->d_ws, h->ws_stride, a...);
}
static void launch(StepFn k, const mpcb_handle *h, hipStream_t s, const StepArgs &a)
{
    latency_launch(k, h, (unsigned)h->pb.batch, s, a.io, a.reset, h->pool_doubles);
}
static void launch(StreamStepFn k, const mpcb_handle *h, hipStream_t s, const StepArgs &a)
{
    stream_launch(k, h, (unsigned)h->pb.batch, s, a.io, a.reset);   // no work queue: one launch is one step of every simulation
}
static void launch(RolloutFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    latency_launch(k, h, a.grid, s, a.out, a.step0, a.step1, h->pool_doubles);
}
static void launch(RolloutRefFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    latency_launch(k, h, a.grid, s, a.out, a.step0, a.step1, h->pool_doubles, a.yref_sched);
}
static void launch(RolloutPertFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    latency_launch(k, h, a.grid, s, a.out, a.step0, a.step1, h->pool_doubles, a.yref_sched, a.pert);
}
static void launch(RolloutTermFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    latency_launch(k, h, a.grid, s, a.out, a.step0, a.step1, h->pool_doubles, a.yref_sched, a.pert, a.term);
}
static void launch(RolloutObsFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    latency_launch(k, h, a.grid, s, a.out, a.step0, a.step1, h->pool_doubles, a.yref_sched, a.pert, a.obs);
}
static void launch(RolloutSurfFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    latency_launch(k, h, a.grid, s, a.out, a.step0, a.step1, h->pool_doubles, a.yref_sched, a.pert, a.surf_sched);
}
static void launch(RolloutShiftFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    latency_launch(k, h, a.grid, s, a.out, a.step0, a.step1, h->pool_doubles, a.yref_sched, a.pert, a.surf_sched, a.warm);
}
static void launch(RolloutCombinedFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    latency_launch(k, h, a.grid, s, a.out, a.step0, a.step1, h->pool_doubles, a.yref_sched, a.pert, a.term, a.obs, a.surf_sched, a.warm);
}
static void launch(StreamRolloutFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    stream_launch(k, h, a.grid, s, a.out, a.step0, a.step1, a.queue, a.chunk_steps, a.timeout_ticks);
}
static void launch(StreamRolloutRefFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    stream_launch(k, h, a.grid, s, a.out, a.step0, a.step1, a.queue, a.chunk_steps, a.timeout_ticks, a.yref_sched);
}
static void launch(StreamRolloutPertFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    stream_launch(k, h, a.grid, s, a.out, a.step0, a.step1, a.queue, a.chunk_steps, a.timeout_ticks, a.yref_sched, a.pert);
}
static void launch(StreamRolloutTermFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    stream_launch(k, h, a.grid, s, a.out, a.step0, a.step1, a.queue, a.chunk_steps, a.timeout_ticks, a.yref_sched, a.pert, a.term);
}

static void launch(StreamRolloutObsFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    stream_launch(k, h, a.grid, s, a.out, a.step0, a.step1, a.queue, a.chunk_steps, a.timeout_ticks, a.yref_sched, a.pert, a.obs);
}

static void launch(StreamRolloutSurfFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    stream_launch(k, h, a.grid, s, a.out, a.step0, a.step1, a.queue, a.chunk_steps, a.timeout_ticks, a.yref_sched, a.pert, a.surf_sched);
}

static void launch(StreamRolloutShiftFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    stream_launch(k, h, a.grid, s, a.out, a.step0, a.step1, a.queue, a.chunk_steps, a.timeout_ticks, a.yref_sched, a.pert, a.surf_sched, a.warm);
}

static void launch(StreamRolloutCombinedFn k, const mpcb_handle *h, hipStream_t s, const RolloutArgs &a)
{
    stream_launch(k, h, a.grid, s, a.out, a.step0, a.step1, a.queue, a.chunk_steps, a.timeout_ticks, a.yref_sched, a.pert, a.term, a.obs,
                  a.surf_sched, a.warm);
}

// One launch of `variant`'s kernel on stream s, between the two events mpcb_last_kernel_ms reads.  Latency engine: the dynamic-LDS
// ceiling is a process-wide attribute of the kernel, not of this handle, so it is raised to the largest pool any handle can ask
// for, right before the launch.
template <class V, class Args>
static int timed_launch(mpcb_handle *h, V variant, hipStream_t s, const Args &args)
{
    return with_kernel(h, variant, [&](auto k) {
        static const int max_lds = (160 * 1024 - (int)sizeof(Smem) - 64) / 16 * 16;
        if (h->engine != 1)
            HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds));
        HIPCHK(h, hipEventRecord(h->ev0, s));
        launch(k, h, s, args);
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipEventRecord(h->ev1, s));
        h->last_stream = s;
        h->timed = true;
        return MPCB_OK;
    });
}

static int rollout_any(mpcb_handle *h, int step0, int step1, const mpcb_result *o, const double *yref_sched, const mpcb_plant_pert *pert_,
                       const double *term_blocks, const double *term_xref, const double *obs_gain, double *d_hat, void *stream,
                       const double *surf_sched = nullptr, const int *warm = nullptr, bool combined = false);

// mpcb_step_combined / mpcb_rollout_combined: the neutral tables of the features given as NULL, in one block of device memory the
// handle keeps: runs of n[0..3] doubles, [0] and [1] zeros (terminal record / blocks and x_ref; disturbance / gains and the d_hat
// scratch rows), [2] the neutral surface table of `rows` rows per simulation, [3] zeros read as MPCB_WARM_CARRY.  Called AFTER the
// entry has validated its arguments.  The tables are constants of the handle's setup: they are filled once -- on stream s, which is
// synchronised so that a later call on another stream finds them -- and again only when the layout changes or after a new setup.
static int neutral_tables(mpcb_handle *h, int entry, const size_t n[4], size_t rows, hipStream_t s, double **out)
{
    static_assert(WARM_CARRY == 0, "the neutral modes are a zero fill");
    const size_t total = n[0] + n[1] + n[2] + n[3], need = total * sizeof(double);
    const size_t layout[5] = {(size_t)entry, n[0], n[1], n[2], n[3]};
    *out = nullptr;
    if (total == 0) return MPCB_OK;
    if (need > h->neutral_cap) {
        if (h->d_neutral) (void)hipFree(h->d_neutral);      // (hipFree waits for the launches that read the old block)
        h->d_neutral = nullptr; h->neutral_cap = 0; h->neutral_layout[0] = 0;
        if (hipMalloc((void **)&h->d_neutral, need) != hipSuccess) return fail(h, MPCB_ENOMEM, "neutral table allocation failed");
        h->neutral_cap = need;
    }
    *out = h->d_neutral;
    if (std::memcmp(layout, h->neutral_layout, sizeof layout) == 0) return MPCB_OK;
    h->neutral_layout[0] = 0;
    HIPCHK(h, hipMemsetAsync(h->d_neutral, 0, need, s));
    if (n[2]) {
        neutral_surf_fill(h->pb.batch, rows, h->d_params, h->d_neutral + n[0] + n[1], s);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, hipStreamSynchronize(s));
    std::memcpy(h->neutral_layout, layout, sizeof layout);
    return MPCB_OK;
}

extern "C" {

int mpcb_version(void) { return MPCB_VERSION; }

int mpcb_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int mpcb_create(mpcb_handle **out, int device)
{
    if (!out) return MPCB_EINVAL;
    *out = nullptr;
    int n = mpcb_device_count();
    if (n <= 0 || device < 0 || device >= n) return MPCB_ENODEV;
    mpcb_handle *h = new (std::nothrow) mpcb_handle;
    if (!h) return MPCB_ENOMEM;
    h->device = device;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            h->num_cus = prop.multiProcessorCount;
    }
    if (hipSetDevice(device) != hipSuccess || hipEventCreate(&h->ev0) != hipSuccess ||
        hipEventCreate(&h->ev1) != hipSuccess) {
        delete h;
        return MPCB_EHIP;
    }
    *out = h;
    return MPCB_OK;
}

void mpcb_destroy(mpcb_handle *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->d_params) (void)hipFree(h->d_params);
    if (h->d_ws) (void)hipFree(h->d_ws);
    if (h->d_queue) (void)hipFree(h->d_queue);
    if (h->d_neutral) (void)hipFree(h->d_neutral);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
}

const char *mpcb_last_error(const mpcb_handle *h) { return h ? h->err.c_str() : "invalid handle"; }

// which kernel family runs `p` (see include/mpcbatch.h); `ragged`: the simulations have different horizons
static int pick_engine(const mpcb_problem *p, bool ragged = false)
{
    if (p->precision == MPCB_PRECISION_FP32_RICCATI || ragged) return 1;
    // Full SQP work per step is heavy-tailed while the closed loop settles (a few simulations run into
    // nlp_solver_max_iter): short or small runs end with those simulations' sequential chains, where the latency engine is
    // faster per simulation; long runs of large batches are throughput work again, and the work-queue launch balances them.
    // Measured at N = 100 (profiles/r03_engine_sweep.txt), throughput engine queued / latency engine (two simulations per CU,
    // register-resident sweeps), steps/s: batch 4096 x 600 steps 321 k / 289 k, x 100 steps 72 k / 80 k; batch 3072 x 600:
    // 265 k / 265 k; 2560 x 600: 229 k / 256 k.  (Round 2, before those sweeps: 299 k / 214 k, 67 k / 59 k, 245 k / 195 k.)
    int e = 0;
    if (p->solver_type == MPCB_SOLVER_SQP_RTI) e = p->batch >= MPCB_STREAM_MIN_BATCH ? 1 : 0;
    else e = p->batch >= MPCB_STREAM_MIN_BATCH_SQP && p->Nsim >= MPCB_STREAM_MIN_STEPS_SQP ? 1 : 0;
    if (const char *env = getenv("MPCB_ENGINE")) {
        if (!strcmp(env, "stream")) e = 1;
        else if (!strcmp(env, "latency")) e = 0;
    }
    return e;
}
// which kernel family runs the controller step of `p` under MPCB_ENGINE_AUTO (see include/mpcbatch.h): ragged batches need the
// throughput engine; a uniform batch crosses over at the measured batch sizes (profiles/controller_step_rate_stream.txt)
static int pick_controller_engine(const mpcb_problem *p, bool ragged)
{
    if (ragged) return MPCB_ENGINE_STREAM;
    // (full SQP: the latency engine at every batch size measured -- a step ends with its slowest simulation's chain of SQP iterations)
    int e = p->solver_type == MPCB_SOLVER_SQP_RTI && p->batch >= MPCB_STREAM_MIN_BATCH_STEP ? MPCB_ENGINE_STREAM : MPCB_ENGINE_LATENCY;
    if (const char *env = getenv("MPCB_ENGINE")) {
        if (!strcmp(env, "stream")) e = MPCB_ENGINE_STREAM;
        else if (!strcmp(env, "latency")) e = MPCB_ENGINE_LATENCY;
    }
    return e;
}
static size_t ws_doubles_for(const mpcb_problem *p, bool ragged = false)
{
    if (pick_engine(p, ragged) == 0) return ws_doubles_per_instance(p->N);
    const bool sqp = p->solver_type == MPCB_SOLVER_SQP;
    return p->precision == MPCB_PRECISION_FP32_RICCATI ? se::sws_doubles_per_instance<float>(p->N, sqp) : se::sws_doubles_per_instance<double>(p->N, sqp);
}

size_t mpcb_workspace_bytes(const mpcb_problem *p)
{
    if (!p || p->N < 1 || p->batch < 1) return 0;
    return (size_t)p->batch * ws_doubles_for(p) * sizeof(double);
}

size_t mpcb_result_bytes_per_sim(const mpcb_problem *p)
{
    if (!p) return 0;
    const size_t T1 = (size_t)p->Nsim + 1, S = (size_t)p->Nsim;
    return (12 + 6 + 12 + 3 + 6 + 7) * T1 * sizeof(double) + 3 * S * sizeof(int) + (4 + 1 + 1 + 1) * S * sizeof(double);
}

// mpcb_setup and mpcb_setup_controller(_on): validate, pack and upload the records, size the workspace, pick the geometry.
// `controller`: the controller step on kernel family `ctl_engine` (MPCB_ENGINE_*), fp64 only; ragged horizons on the throughput
// engine only, with SQP_RTI.
static int setup_impl(mpcb_handle *h, const mpcb_problem *p, const double *params_host, const double *robot_host, bool controller,
                      int ctl_engine = MPCB_ENGINE_LATENCY)
{
    if (!h) return MPCB_EINVAL;
    int rc = check_problem(h, p);
    if (rc) return rc;
    if (controller && ctl_engine != MPCB_ENGINE_LATENCY && ctl_engine != MPCB_ENGINE_STREAM && ctl_engine != MPCB_ENGINE_AUTO)
        return fail(h, MPCB_EINVAL, "engine must be MPCB_ENGINE_LATENCY, MPCB_ENGINE_STREAM or MPCB_ENGINE_AUTO");
    if (controller && p->precision != MPCB_PRECISION_FP64)
        return fail(h, MPCB_EINVAL, "the controller step is fp64 only (no fp32 Riccati leg on either engine)");
    if (!params_host || !robot_host) return fail(h, MPCB_EINVAL, "params/robot pointer is NULL");
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<InstParams> packed((size_t)p->batch);
    bool ragged = false;
    for (int i = 0; i < p->batch; i++) {
        const double *pp = params_host + (size_t)i * MPCB_NPARAM;
        if (pp[65] != 0.0) {
            if (!(pp[65] >= 1.0 && pp[65] <= (double)p->N) || pp[65] != std::floor(pp[65]))
                return fail(h, MPCB_EINVAL, "per-simulation horizon (parameter [65]) must be an integer in [1, N]");
            if ((int)pp[65] != p->N) ragged = true;
        }
        if (!(pp[0] > 0.0)) return fail(h, MPCB_EINVAL, "dt must be positive");
        for (int j = 0; j < 6; j++)
            if (!(pp[8 + j] > 0.0)) return fail(h, MPCB_EINVAL, "wcv must be positive");
        for (int j = 0; j < MPCB_NPARAM; j++)
            if (std::isnan(pp[j])) return fail(h, MPCB_EINVAL, "NaN in parameter record");
        pack_inst_params(pp, &packed[(size_t)i]);
    }
    if (controller && ctl_engine == MPCB_ENGINE_AUTO) ctl_engine = pick_controller_engine(p, ragged);
    if (controller && ragged && ctl_engine == MPCB_ENGINE_LATENCY)
        return fail(h, MPCB_EINVAL, "the latency engine's controller step needs one horizon for the whole batch (parameter [65] must be 0 or N)");
    if (controller && ragged && p->solver_type != MPCB_SOLVER_SQP_RTI)
        return fail(h, MPCB_EINVAL, "simulations of different horizons share a controller batch only with SQP_RTI");
    std::memcpy(&h->rb, robot_host, sizeof(Robot));
    std::memcpy(&h->pb, p, sizeof(Problem));
    const size_t pbytes = packed.size() * sizeof(InstParams);
    if (pbytes + sizeof(Robot) > h->params_cap) {   // the robot record rides behind the parameter records (throughput engine reads it from memory)
        if (h->d_params) (void)hipFree(h->d_params);
        h->d_params = nullptr; h->params_cap = 0;
        if (hipMalloc((void **)&h->d_params, pbytes + sizeof(Robot)) != hipSuccess) return fail(h, MPCB_ENOMEM, "hipMalloc(params)");
        h->params_cap = pbytes + sizeof(Robot);
    }
    HIPCHK(h, hipMemcpy(h->d_params, packed.data(), pbytes, hipMemcpyHostToDevice));
    h->d_rb = reinterpret_cast<Robot *>(reinterpret_cast<char *>(h->d_params) + pbytes);
    HIPCHK(h, hipMemcpy(h->d_rb, &h->rb, sizeof(Robot), hipMemcpyHostToDevice));
    h->engine = controller ? ctl_engine : pick_engine(p, ragged);
    h->ws_stride = !controller ? ws_doubles_for(p, ragged)
                 : h->engine == MPCB_ENGINE_STREAM ? se::sws_doubles_per_instance<double>(p->N, p->solver_type == MPCB_SOLVER_SQP)
                                                   : ws_doubles_per_instance(p->N);
    const size_t wbytes = (size_t)p->batch * h->ws_stride * sizeof(double);
    if (wbytes > h->ws_cap) {
        if (h->d_ws) (void)hipFree(h->d_ws);
        h->d_ws = nullptr; h->ws_cap = 0;
        if (hipMalloc((void **)&h->d_ws, wbytes) != hipSuccess) return fail(h, MPCB_ENOMEM, "hipMalloc(workspace)");
        h->ws_cap = wbytes;
    }
    // LDS chunk pool: the whole 160 KiB of a CU is shared by the waves resident on it, so size the
    // pool for the number of simulations per CU this batch implies (1 for batch <= #CUs).
    {
        // More than a few resident simulations per CU only shrinks the chunks (more, smaller bursts);
        // beyond that the grid simply queues.  MPCB_SIMS_PER_CU overrides the residency target.
        int wpc = (p->batch + h->num_cus - 1) / h->num_cus;
        if (wpc > 2) wpc = 2;
        // (Measured, N = 100, 600 steps, profiles/r03_engine_sweep.txt: batch 512 as two simulations per CU at half the pool on the
        // streaming path 730 k steps/s; as one per CU with the LDS-resident factor, the grid running in two rounds, 640 k: two
        // factorisation chains side by side on a CU beat one faster one, so the residency target stays 2 beyond #CUs.)
        if (const char *e2 = getenv("MPCB_SIMS_PER_CU")) { const int v = atoi(e2); if (v >= 1 && v <= 8) wpc = v; }
        h->pool_doubles = lay_pool_doubles(wpc);
        // wavefronts per simulation: the four SIMDs of a CU are otherwise idle at one simulation per CU
        const char *env = getenv("MPCB_WAVES_PER_SIM");
        // one simulation per CU: 4 wavefronts, 512 registers; beyond: two 4-wavefront simulations per CU at 256 registers
        int nw = wpc <= 2 ? 4 : 1;
        int wpe = wpc == 2 ? 2 : 1;
        // one simulation per CU AND the factor LDS-resident (Engine::resident_ok): every pass but the factorisation sweep is item- or
        // chunk-parallel then, and a second wavefront per SIMD buys issue slots (665 k vs 651 k steps/s on configs[1]); the streaming
        // path's role layout prefers 4 (round 1).
        {
            // (the device's own predicates, mpc_layout.h; 16 lane groups at four and at eight wavefronts)
            // (measured: N = 100 665 k vs 651 k; N = 50 1.045 M vs 1.054 M; N = 20 1.59 M vs 1.68 M -- short horizons have too few items)
            const bool resident = lay_resident_ok(p->N, h->pool_doubles, 16);
            // longer horizons at one simulation per CU run the same sweeps one LDS segment at a time (Engine::segment_ok): eight
            // wavefronts there as well (batch 256, N = 200: 244.8 k vs 234.5 k steps/s; N = 300: 144.5 k vs 137.9 k)
            const bool segments = lay_segment_ok(p->N, h->pool_doubles, 16);
            // Round 4, with one factorisation per step (the fast path) the item phases are a fifth of a step instead of two fifths, and
            // the recursion wavefront alone on its SIMD matters more (profiles/r04_geometry.txt, batch 256, 4 / 8 wavefronts, ms per
            // launch): N = 80 83.8 / 85.9, N = 100 99.9-100.6 / 101.6-102.4, N = 125 90.4 / 88.0 (400 steps), N = 200 116.4 / 115.4,
            // N = 300 139.0 / 135.1 -- eight from N = 112 on (80 in round 3).  End of round 4: those 256-register builds had been paying for
            // scratch spills around the library sincos in the NLP pass; with the joint-angle sincos of mpc_kin.h (no spills) eight win
            // from N = 80 again (profiles/r04_geometry2.txt: N = 50 58.7 / 59.7 ms, N = 80 84.4 / 83.7, N = 100 97.5 / 95.3,
            // N = 112 111.3 / 106.6)
            if (wpc == 1 && p->N >= 80 && (resident || segments)) nw = 8;
        }
        if (env && (atoi(env) == 1 || atoi(env) == 2 || atoi(env) == 4 || atoi(env) == 8)) { nw = atoi(env); wpe = 1; }
        if (const char *e3 = getenv("MPCB_WPE")) { if (atoi(e3) == 2 && nw == 4) wpe = 2; else if (atoi(e3) == 1) wpe = 1; }
        h->waves_per_sim = nw;
        h->wpe = wpe;
        if (h->engine == 1) { h->waves_per_sim = 1; h->pool_doubles = 0; }   // throughput engine: one wavefront, static LDS only
    }
    h->ready = true;
    h->next_step = 0;
    h->neutral_layout[0] = 0;       // (new parameter records: the neutral surface table is stale)
    h->last_rollout = ROLLOUT_BASE;
    h->timed = false;
    h->controller = controller;
    h->reset_next = true;
    h->weights_changed = false;
    return MPCB_OK;
}

int mpcb_setup(mpcb_handle *h, const mpcb_problem *p, const double *params_host, const double *robot_host)
{
    return setup_impl(h, p, params_host, robot_host, false);
}

int mpcb_setup_controller(mpcb_handle *h, const mpcb_problem *p, const double *params_host, const double *robot_host)
{
    return setup_impl(h, p, params_host, robot_host, true);
}

int mpcb_setup_controller_on(mpcb_handle *h, const mpcb_problem *p, const double *params_host, const double *robot_host, int engine)
{
    return setup_impl(h, p, params_host, robot_host, true, engine);
}

int mpcb_controller_engine_for(const mpcb_problem *p, int ragged)
{
    if (!p || p->N < 1 || p->batch < 1) return MPCB_EINVAL;
    return pick_controller_engine(p, ragged != 0);
}

// Hand-off timeout of the work-queue launch in ticks of the 100 MHz clock: the most work one chunk of one simulation can be
// (chunk_steps x SQP iterations x (interior-point iterations + 1) x (N + 1) stage-iterations), priced at 20 us per stage-iteration --
// more than 10x what a wavefront sharing its SIMD takes, profiling and eight buckets in flight included -- times 4, plus 30 s.
// MPCB_QUEUE_TIMEOUT_S overrides it (seconds).
static long long queue_timeout_ticks(const Problem &pb, int chunk_steps)
{
    if (const char *e = getenv("MPCB_QUEUE_TIMEOUT_S")) { const double v = atof(e); if (v > 0) return (long long)(v * 1e8); }
    const double sqp = pb.solver_type == MPCB_SOLVER_SQP ? (double)(pb.max_iter > 1 ? pb.max_iter : 1) : 1.0;
    const double work_s = (double)(chunk_steps > 1 ? chunk_steps : 1) * sqp * (double)(pb.qp_iter_max + 1) * (double)(pb.N + 1) * 20e-6;
    return (long long)((4.0 * work_s + 30.0) * 1e8);
}

int mpcb_rollout(mpcb_handle *h, int step0, int step1, const mpcb_result *o, void *stream)
{
    return mpcb_rollout_ref(h, step0, step1, o, nullptr, stream);
}

// (yref_sched == NULL: the kernels of mpcb_rollout; otherwise those of the scheduled rollout, mpc_rollout_ref.hip /
// mpc_stream_rollout_ref.hip -- one launch path: queue sizing, timeout, events and next_step are the same, only the kernel and one
// argument differ)
int mpcb_rollout_ref(mpcb_handle *h, int step0, int step1, const mpcb_result *o, const double *yref_sched, void *stream)
{
    return mpcb_rollout_pert(h, step0, step1, o, yref_sched, nullptr, stream);
}

// (pert == NULL: the kernels above, chosen by yref_sched; otherwise those of the perturbed rollout, mpc_rollout_pert.hip /
// mpc_stream_rollout_pert.hip, through the same launch path with one argument more)
int mpcb_rollout_pert(mpcb_handle *h, int step0, int step1, const mpcb_result *o, const double *yref_sched, const mpcb_plant_pert *pert_,
                      void *stream)
{
    return mpcb_rollout_term(h, step0, step1, o, yref_sched, pert_, nullptr, nullptr, stream);
}

// (term_blocks == NULL: the kernels above, chosen by pert and yref_sched; otherwise those of the rollout with a terminal cost,
// mpc_rollout_term.hip / mpc_stream_rollout_term.hip, through the same launch path with one argument more -- a null pert is the
// nominal plant inside them)
int mpcb_rollout_term(mpcb_handle *h, int step0, int step1, const mpcb_result *o, const double *yref_sched, const mpcb_plant_pert *pert_,
                      const double *term_blocks, const double *term_xref, void *stream)
{
    return rollout_any(h, step0, step1, o, yref_sched, pert_, term_blocks, term_xref, nullptr, nullptr, stream);
}

// (obs_gain == NULL: the kernels of mpcb_rollout_pert, chosen by pert and yref_sched; otherwise those of the rollout with an observer,
// mpc_rollout_obs.hip / mpc_stream_rollout_obs.hip, through the same launch path -- a null pert is the nominal plant inside them)
int mpcb_rollout_obs(mpcb_handle *h, int step0, int step1, const mpcb_result *o, const double *yref_sched, const mpcb_plant_pert *pert_,
                     const double *obs_gain, double *d_hat, void *stream)
{
    return rollout_any(h, step0, step1, o, yref_sched, pert_, nullptr, nullptr, obs_gain, d_hat, stream);
}

// (surf_sched == NULL: the kernels of mpcb_rollout_pert, chosen by pert and yref_sched; otherwise those of the rollout over a scheduled
// surface, mpc_rollout_surf.hip / mpc_stream_rollout_surf.hip, through the same launch path -- a null pert is the nominal plant inside them)
int mpcb_rollout_surf(mpcb_handle *h, int step0, int step1, const mpcb_result *o, const double *yref_sched, const mpcb_plant_pert *pert_,
                      const double *surf_sched, void *stream)
{
    return rollout_any(h, step0, step1, o, yref_sched, pert_, nullptr, nullptr, nullptr, nullptr, stream, surf_sched);
}

// (warm == NULL: mpcb_rollout_surf, hence with surf_sched == NULL mpcb_rollout_pert; otherwise the kernels of the rollout with the shift
// warm start, mpc_rollout_shift.hip / mpc_stream_rollout_shift.hip, built without or with the scheduled surface)
int mpcb_rollout_warm(mpcb_handle *h, int step0, int step1, const mpcb_result *o, const double *yref_sched, const mpcb_plant_pert *pert_,
                      const double *surf_sched, const int *warm, void *stream)
{
    return rollout_any(h, step0, step1, o, yref_sched, pert_, nullptr, nullptr, nullptr, nullptr, stream, surf_sched, warm);
}

// (always the kernels of mpc_rollout_combined.hip / mpc_stream_rollout_combined.hip; a feature given as NULL gets its neutral table here)
int mpcb_rollout_combined(mpcb_handle *h, int step0, int step1, const mpcb_result *o, const double *yref_sched, const mpcb_plant_pert *pert_,
                          const mpcb_term_table *term, const mpcb_observer *obs, const double *surf_sched, const int *warm, void *stream)
{
    if (!h) return MPCB_EINVAL;
    if (!h->ready) return fail(h, MPCB_ESTATE, "mpcb_rollout before mpcb_setup");
    if (h->controller) return fail(h, MPCB_ESTATE, "mpcb_rollout on a controller handle (mpcb_setup_controller): use mpcb_step");
    if (h->pb.precision == MPCB_PRECISION_FP32_RICCATI)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_combined: the combined rollout is offered in fp64 only (no fp32 Riccati leg)");
    if (h->pb.solver_type != MPCB_SOLVER_SQP_RTI)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_combined: the combined rollout is offered with SQP_RTI only");
    if (!yref_sched)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_combined: the combined rollout needs a reference schedule (the packed rows when there is none)");
    if (term && (!term->blocks || !term->x_ref))
        return fail(h, MPCB_EINVAL, "mpcb_rollout_combined: term needs blocks and x_ref");
    if (obs && (!obs->gain || !obs->d_hat))
        return fail(h, MPCB_EINVAL, "mpcb_rollout_combined: obs needs gain and d_hat");
    return rollout_any(h, step0, step1, o, yref_sched, pert_, term ? term->blocks : nullptr, term ? term->x_ref : nullptr,
                       obs ? obs->gain : nullptr, obs ? obs->d_hat : nullptr, stream, surf_sched, warm, true);
}

}  // extern "C"

// The one launch path of every rollout: at most one of term_blocks, obs_gain and surf_sched is given; warm goes with neither
// term_blocks nor obs_gain.  `combined` (mpcb_rollout_combined): all of them are given, and the combined kernels run.
static int rollout_any(mpcb_handle *h, int step0, int step1, const mpcb_result *o, const double *yref_sched, const mpcb_plant_pert *pert_,
                       const double *term_blocks, const double *term_xref, const double *obs_gain, double *d_hat, void *stream,
                       const double *surf_sched, const int *warm, bool combined)
{
    if (!h) return MPCB_EINVAL;
    if (!h->ready) return fail(h, MPCB_ESTATE, "mpcb_rollout before mpcb_setup");
    if (h->controller) return fail(h, MPCB_ESTATE, "mpcb_rollout on a controller handle (mpcb_setup_controller): use mpcb_step");
    if (yref_sched && h->pb.precision == MPCB_PRECISION_FP32_RICCATI)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_ref: a reference schedule is offered in fp64 only (no fp32 Riccati leg)");
    if (pert_ && h->pb.precision == MPCB_PRECISION_FP32_RICCATI)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_pert: a perturbed plant is offered in fp64 only (no fp32 Riccati leg)");
    if (pert_ && !yref_sched)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_pert: a perturbed rollout needs a reference schedule (the packed rows when there is none)");
    if (term_blocks && h->pb.precision == MPCB_PRECISION_FP32_RICCATI)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_term: a terminal cost is offered in fp64 only (no fp32 Riccati leg)");
    if (term_blocks && h->pb.solver_type != MPCB_SOLVER_SQP_RTI)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_term: a terminal cost is offered with SQP_RTI only");
    if (term_blocks && !yref_sched)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_term: a rollout with a terminal cost needs a reference schedule (the packed rows when there is none)");
    if (term_blocks && !term_xref)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_term: term_blocks needs term_xref, the table of terminal references");
    if (obs_gain && h->pb.precision == MPCB_PRECISION_FP32_RICCATI)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_obs: a disturbance observer is offered in fp64 only (no fp32 Riccati leg)");
    if (obs_gain && h->pb.solver_type != MPCB_SOLVER_SQP_RTI)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_obs: a disturbance observer is offered with SQP_RTI only");
    if (obs_gain && !yref_sched)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_obs: a rollout with an observer needs a reference schedule (the packed rows when there is none)");
    if (obs_gain && !d_hat)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_obs: obs_gain needs d_hat, the log of the estimates");
    if (surf_sched && h->pb.precision == MPCB_PRECISION_FP32_RICCATI)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_surf: a surface schedule is offered in fp64 only (no fp32 Riccati leg)");
    if (surf_sched && h->pb.solver_type != MPCB_SOLVER_SQP_RTI)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_surf: a surface schedule is offered with SQP_RTI only");
    if (surf_sched && !yref_sched)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_surf: a rollout over a scheduled surface needs a reference schedule (the packed rows when there is none)");
    if (warm && h->pb.precision == MPCB_PRECISION_FP32_RICCATI)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_warm: the shift warm start is offered in fp64 only (no fp32 Riccati leg)");
    if (warm && h->pb.solver_type != MPCB_SOLVER_SQP_RTI)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_warm: the shift warm start is offered with SQP_RTI only");
    if (warm && !yref_sched)
        return fail(h, MPCB_EINVAL, "mpcb_rollout_warm: a rollout with the shift warm start needs a reference schedule (the packed rows when there is none)");
    if (!o) return fail(h, MPCB_EINVAL, "result pointer is NULL");
    if (step0 != h->next_step && step0 != 0)
        return fail(h, MPCB_ESTATE, "step0 must continue the previous rollout (or be 0 to restart)");
    if (step1 <= step0 || step1 > h->pb.Nsim) return fail(h, MPCB_EINVAL, "step range out of bounds");
    if (!o->z || !o->u || !o->ee_pose || !o->ee_rpy || !o->ee_vel || !o->status || !o->sqp_iter || !o->qp_iter ||
        !o->residuals || !o->cost || !o->solver_time || !o->errors || !o->plant_time)
        return fail(h, MPCB_EINVAL, "every result array must be provided");
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (combined) {
        // every argument is validated: the neutral tables of the features given as NULL (zero blocks -- x_e then multiplies zeros --,
        // zero gains with the d_hat log going to scratch rows, the packed surface on every row, all modes MPCB_WARM_CARRY)
        const size_t B = (size_t)h->pb.batch, Nsim = (size_t)h->pb.Nsim, rows = Nsim + (size_t)h->pb.N;
        const size_t n[4] = {term_blocks ? 0 : B * 18 + B * Nsim * 12, obs_gain ? 0 : B * 12 + B * Nsim * 6,
                             surf_sched ? 0 : B * rows * NSURF, warm ? 0 : (B + 1) / 2};
        double *nb = nullptr;
        if (int rc = neutral_tables(h, 1, n, rows, s, &nb)) return rc;
        if (!term_blocks) { term_blocks = nb; term_xref = nb + B * 18; }
        if (!obs_gain) { obs_gain = nb + n[0]; d_hat = nb + n[0] + B * 12; }
        if (!surf_sched) surf_sched = nb + n[0] + n[1];
        if (!warm) warm = reinterpret_cast<const int *>(nb + n[0] + n[1] + n[2]);
    }
    const RolloutKind kind = combined ? ROLLOUT_COMBINED : warm ? (surf_sched ? ROLLOUT_SHIFT_SURF : ROLLOUT_SHIFT) : surf_sched ? ROLLOUT_SURF : obs_gain ? ROLLOUT_OBS : term_blocks ? ROLLOUT_TERM : pert_ ? ROLLOUT_PERT : yref_sched ? ROLLOUT_REF : ROLLOUT_BASE;
    RolloutArgs args{};
    args.yref_sched = yref_sched;
    if (pert_) args.pert = PlantPert{pert_->wcv, pert_->u_dist, pert_->x_noise};
    args.term = TermTab{term_blocks, term_xref};
    args.obs = ObsArg{obs_gain, d_hat};
    args.surf_sched = surf_sched;
    args.warm = warm;
    std::memcpy(&args.out, o, sizeof args.out);
    args.step0 = step0;
    args.step1 = step1;
    args.grid = (unsigned)h->pb.batch;
    if (h->engine == 1) {
        // at least as many simulations as resident wavefronts: work queue over (simulation, chunk of steps) items.
        // Measured at N=100, 600 steps (profiles/r02_work_queue.txt): batch 4096 890 -> 968 k steps/s, 2560 668 -> 939 k,
        // 2048 876 -> 909 k; chunks of 8..20 steps are equivalent, 1 step costs 2.5 %, 50 steps 1.4 %.  Full SQP: only for
        // runs of >= 100 steps (see pick_engine: the settling phase is heavy-tailed, hand-off waits then add to the chains).
        const int slots = h->num_cus * 4 * MPCB_STREAM_WPE;
        int chunk = 10;
        bool chunk_forced = false;                                   // (an explicit MPCB_STREAM_CHUNK also applies to full SQP)
        if (const char *e = getenv("MPCB_STREAM_CHUNK")) { chunk = atoi(e); chunk_forced = true; }
        int nslots = slots;
        if (const char *e = getenv("MPCB_STREAM_SLOTS")) { if (atoi(e) > 0) nslots = atoi(e); }   // (tests: force hand-offs on small batches)
        const bool queued = chunk > 0 && h->pb.batch >= nslots && (h->pb.solver_type == 1 || chunk_forced || h->pb.Nsim >= 100);
        int *queue = nullptr;
        if (queued) {
            const size_t need = (size_t)(2 + h->pb.batch) * sizeof(int);
            if (need > h->queue_cap) {
                if (h->d_queue) (void)hipFree(h->d_queue);
                h->d_queue = nullptr; h->queue_cap = 0;
                if (hipMalloc((void **)&h->d_queue, need) != hipSuccess) return fail(h, MPCB_ENOMEM, "work queue allocation failed");
                h->queue_cap = need;
            }
            HIPCHK(h, hipMemsetAsync(h->d_queue, 0, need, s));
            queue = h->d_queue;
        }
        h->queue_used = queued;
        args.grid = (unsigned)(queued ? nslots : h->pb.batch);
        args.queue = queue;
        args.chunk_steps = chunk;
        args.timeout_ticks = queue_timeout_ticks(h->pb, chunk);
    }
    h->last_rollout = kind;
    if (int rc = timed_launch(h, kind, s, args)) return rc;
    h->next_step = step1;
    return MPCB_OK;
}

extern "C" {

int mpcb_set_weights(mpcb_handle *h, const double *weights, void *stream)
{
    if (!h) return MPCB_EINVAL;
    if (!h->ready || !h->controller) return fail(h, MPCB_ESTATE, "mpcb_set_weights needs a handle set up by mpcb_setup_controller");
    if (!weights) return fail(h, MPCB_EINVAL, "weights pointer is NULL");
    HIPCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(mpc_set_weights_kernel, dim3((unsigned)((h->pb.batch + WAVE - 1) / WAVE)), dim3(WAVE), 0, (hipStream_t)stream,
                       h->pb.batch, h->d_params, weights);
    HIPCHK(h, hipGetLastError());
    h->weights_changed = true;
    return MPCB_OK;
}

int mpcb_step(mpcb_handle *h, const mpcb_step_io *io, int reset, void *stream)
{
    return mpcb_step_ref(h, io, nullptr, 0, reset, stream);
}

int mpcb_step_ref(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, int reset, void *stream)
{
    return mpcb_step_warm(h, io, yref, ref_changed, nullptr, reset, stream);
}

int mpcb_step_warm(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, const int *warm, int reset, void *stream)
{
    return mpcb_step_sens(h, io, yref, ref_changed, warm, reset, nullptr, stream);
}

// (sens == NULL and warm == NULL: the kernels of mpcb_step / mpcb_step_ref, which know no modes; sens == NULL: the warm-start kernels;
// otherwise the kernels that run the sensitivity pass, which are supersets of the warm-start ones)
int mpcb_step_sens(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, const int *warm, int reset,
                   const mpcb_step_sens_out *sens, void *stream)
{
    return mpcb_step_sens_w(h, io, yref, ref_changed, warm, reset, sens, nullptr, stream);
}

static int step_impl(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, const int *warm, int reset,
                     const mpcb_step_sens_out *sens, double *du0_dw, const double *term, int term_changed, double *du0_dxe, void *stream,
                     const double *dist = nullptr, int dist_changed = 0, const double *surf = nullptr, int surf_changed = 0,
                     bool combined = false);

// (du0_dw == NULL: all of the above; otherwise the kernels that also form the weight sensitivity, supersets of the sens ones)
int mpcb_step_sens_w(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, const int *warm, int reset,
                     const mpcb_step_sens_out *sens, double *du0_dw, void *stream)
{
    return step_impl(h, io, yref, ref_changed, warm, reset, sens, du0_dw, nullptr, 0, nullptr, stream);
}

// (term == NULL: mpcb_step_sens, after term_changed from a fresh linearisation; otherwise the kernels built with the terminal cost --
// supersets of the warm-start ones, and with sens of the sens ones)
int mpcb_step_term(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, const int *warm, int reset,
                   const mpcb_step_sens_out *sens, const double *term, int term_changed, double *du0_dxe, void *stream)
{
    return step_impl(h, io, yref, ref_changed, warm, reset, sens, nullptr, term, term_changed, du0_dxe, stream);
}

// (dist == NULL: mpcb_step_warm, after dist_changed from a fresh linearisation; otherwise the kernels built with the input disturbance
// in the prediction model -- supersets of the warm-start ones)
int mpcb_step_dist(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, const int *warm, int reset,
                   const double *dist, int dist_changed, void *stream)
{
    return step_impl(h, io, yref, ref_changed, warm, reset, nullptr, nullptr, nullptr, 0, nullptr, stream, dist, dist_changed);
}

// (surf == NULL: mpcb_step_warm, after surf_changed from a fresh linearisation; otherwise the kernels built with the scheduled surface --
// supersets of the warm-start ones)
int mpcb_step_surf(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, const int *warm, int reset,
                   const double *surf, int surf_changed, void *stream)
{
    return step_impl(h, io, yref, ref_changed, warm, reset, nullptr, nullptr, nullptr, 0, nullptr, stream, nullptr, 0, surf, surf_changed);
}

// (always the kernels of mpc_step_combined.hip / mpc_stream_step_combined.hip; a feature given as NULL gets its neutral table here, and
// warm == NULL stays NULL: the step reads it as MPCB_WARM_CARRY for all)
int mpcb_step_combined(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, const int *warm, int reset,
                       const double *term, int term_changed, const double *dist, int dist_changed, const double *surf, int surf_changed,
                       void *stream)
{
    if (!h) return MPCB_EINVAL;
    if (!h->ready) return fail(h, MPCB_ESTATE, "mpcb_step before mpcb_setup_controller");
    if (!h->controller) return fail(h, MPCB_ESTATE, "mpcb_step needs a handle set up by mpcb_setup_controller");
    if (h->pb.solver_type != MPCB_SOLVER_SQP_RTI)
        return fail(h, MPCB_EINVAL, "mpcb_step_combined: the combined step is offered with SQP_RTI; this controller runs full SQP");
    if (h->pb.precision == MPCB_PRECISION_FP32_RICCATI)
        return fail(h, MPCB_EINVAL, "mpcb_step_combined: the combined step is offered in fp64 only (no fp32 Riccati leg)");
    return step_impl(h, io, yref, ref_changed, warm, reset, nullptr, nullptr, term, term_changed, nullptr, stream, dist, dist_changed, surf,
                     surf_changed, true);
}

static int step_impl(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, const int *warm, int reset,
                     const mpcb_step_sens_out *sens, double *du0_dw, const double *term, int term_changed, double *du0_dxe, void *stream,
                     const double *dist, int dist_changed, const double *surf, int surf_changed, bool combined)
{
    if (!h) return MPCB_EINVAL;
    if (!h->ready) return fail(h, MPCB_ESTATE, "mpcb_step before mpcb_setup_controller");
    if (!h->controller) return fail(h, MPCB_ESTATE, "mpcb_step needs a handle set up by mpcb_setup_controller");
    if (!io) return fail(h, MPCB_EINVAL, "step io pointer is NULL");
    if (!io->xhat || !io->u0 || !io->status || !io->sqp_iter || !io->qp_iter || !io->residuals || !io->cost || !io->solver_time)
        return fail(h, MPCB_EINVAL, "every step array but x_pred / u_pred must be provided");
    if (sens) {
        if (h->pb.solver_type != MPCB_SOLVER_SQP_RTI)
            return fail(h, MPCB_EINVAL, "mpcb_step_sens: the sensitivities of u0 are those of an SQP_RTI step's QP; this controller runs full SQP");
        if (!sens->du0_dx || !sens->valid) return fail(h, MPCB_EINVAL, "mpcb_step_sens: du0_dx and valid must be provided");
    }
    if (du0_dw && !sens) return fail(h, MPCB_EINVAL, "mpcb_step_sens_w: du0_dw needs sens (du0_dx and valid)");
    if (term && h->pb.solver_type != MPCB_SOLVER_SQP_RTI)
        return fail(h, MPCB_EINVAL, "mpcb_step_term: the terminal cost is offered with SQP_RTI; this controller runs full SQP");
    if (du0_dxe && (!sens || !term)) return fail(h, MPCB_EINVAL, "mpcb_step_term: du0_dxe needs sens (du0_dx and valid) and term");
    if (dist && h->pb.solver_type != MPCB_SOLVER_SQP_RTI)
        return fail(h, MPCB_EINVAL, "mpcb_step_dist: the input disturbance is offered with SQP_RTI; this controller runs full SQP");
    if (surf && h->pb.solver_type != MPCB_SOLVER_SQP_RTI)
        return fail(h, MPCB_EINVAL, "mpcb_step_surf: the scheduled surface is offered with SQP_RTI; this controller runs full SQP");
    if (surf && h->pb.precision == MPCB_PRECISION_FP32_RICCATI)
        return fail(h, MPCB_EINVAL, "mpcb_step_surf: the scheduled surface is offered in fp64 only (no fp32 Riccati leg)");
    const StepVariant variant = combined ? STEP_COMBINED : surf ? STEP_SURF : dist ? STEP_DIST : term ? (sens ? STEP_TERM_SENS : STEP_TERM) : du0_dw ? STEP_SENSW : sens ? STEP_SENS : warm ? STEP_WARM : STEP_BASE;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = (hipStream_t)stream;
    if (combined) {
        // every argument is validated: the neutral tables of the features given as NULL (a zero record, d = 0, the packed surface)
        const size_t B = (size_t)h->pb.batch;
        const size_t n[4] = {term ? 0 : B * NTERM, dist ? 0 : B * NU, surf ? 0 : B * (size_t)h->pb.N * NSURF, 0};
        double *nb = nullptr;
        if (int rc = neutral_tables(h, 2, n, (size_t)h->pb.N, s, &nb)) return rc;
        if (!term) term = nb;
        if (!dist) dist = nb + n[0];
        if (!surf) surf = nb + n[0] + n[1];
    }
    StepArgs args;
    StepIO &sio = args.io;
    std::memcpy(&sio, io, sizeof(mpcb_step_io));
    sio.yref = yref;
    // (new weights, a new terminal cost, a new input disturbance or a new surface window make the carried linearisation stale exactly
    // as a new reference does)
    sio.ref_changed = (ref_changed != 0 || term_changed != 0 || dist_changed != 0 || surf_changed != 0 || h->weights_changed) ? 1 : 0;
    sio.warm = warm;
    sio.du0_dw = du0_dw;
    sio.term = term;
    sio.du0_dxe = du0_dxe;
    sio.dist = dist;
    sio.surf = surf;
    if (sens) { sio.du0_dx = sens->du0_dx; sio.du0_dyref = sens->du0_dyref; sio.sens_valid = sens->valid; }
    args.reset = (reset != 0 || h->reset_next) ? 1 : 0;
    if (int rc = timed_launch(h, variant, s, args)) return rc;
    h->queue_used = false;
    h->reset_next = false;
    h->weights_changed = false;
    return MPCB_OK;
}

int mpcb_sync(mpcb_handle *h)
{
    if (!h) return MPCB_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->last_stream));
    if (h->engine == 1 && h->queue_used && h->d_queue) {
        int flag = 0;
        HIPCHK(h, hipMemcpy(&flag, h->d_queue + 1, sizeof flag, hipMemcpyDeviceToHost));
        if (flag) return fail(h, MPCB_EHIP, "work-queue hand-off timed out (results of this launch are incomplete)");
    }
    return MPCB_OK;
}

int mpcb_last_kernel_ms(mpcb_handle *h, float *ms)
{
    if (!h || !ms) return MPCB_EINVAL;
    if (!h->timed) return fail(h, MPCB_ESTATE, "no rollout has been launched");
    HIPCHK(h, hipEventSynchronize(h->ev1));
    HIPCHK(h, hipEventElapsedTime(ms, h->ev0, h->ev1));
    return MPCB_OK;
}

int mpcb_kernel_info(mpcb_handle *h, int *vgprs, int *sgprs, int *lds_bytes, int *scratch_bytes)
{
    if (!h) return MPCB_EINVAL;
    hipFuncAttributes a;
    auto attributes = [&](auto k) { HIPCHK(h, hipFuncGetAttributes(&a, reinterpret_cast<const void *>(k))); return MPCB_OK; };
    // a controller handle: the base step kernel whatever variant ran last; otherwise the kernel of the last rollout launch, where a
    // scheduled rollout counts as the base one
    const RolloutKind kind = h->last_rollout == ROLLOUT_REF ? ROLLOUT_BASE : h->last_rollout;
    if (int rc = h->controller ? with_kernel(h, STEP_BASE, attributes) : with_kernel(h, kind, attributes)) return rc;
    if (vgprs) *vgprs = a.numRegs;
    if (sgprs) *sgprs = 0;
    if (lds_bytes) *lds_bytes = (int)a.sharedSizeBytes;
    if (scratch_bytes) *scratch_bytes = (int)a.localSizeBytes;
    return MPCB_OK;
}

int mpcb_engine(mpcb_handle *h)
{
    if (!h || !h->ready) return MPCB_EINVAL;
    return h->engine;
}

int mpcb_queue_used(mpcb_handle *h)
{
    if (!h || !h->ready) return MPCB_EINVAL;
    return h->queue_used ? 1 : 0;
}

int mpcb_engine_for(const mpcb_problem *p)
{
    if (!p || p->N < 1 || p->batch < 1) return MPCB_EINVAL;
    return pick_engine(p);
}

int mpcb_launch_info(mpcb_handle *h, int *waves_per_sim, int *pool_bytes)
{
    if (!h || !h->ready) return MPCB_EINVAL;
    if (waves_per_sim) *waves_per_sim = h->waves_per_sim;
    if (pool_bytes) *pool_bytes = h->pool_doubles * (int)sizeof(double);
    return MPCB_OK;
}

// Diagnostic builds only (-DMPCB_PROFILE): per-section device seconds accumulated by instance
// `inst`; all zeros in the product build.  Not part of include/mpcbatch.h.
int mpcb_debug_profile(mpcb_handle *h, int inst, double *out16)
{
    if (!h || !out16 || !h->ready || inst < 0 || inst >= h->pb.batch) return MPCB_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    const double *src = h->d_ws + (size_t)inst * h->ws_stride + (h->ws_stride - STATE_DOUBLES) + 32;
    HIPCHK(h, hipMemcpy(out16, src, NPROF * sizeof(double), hipMemcpyDeviceToHost));
    return MPCB_OK;
}

// Diagnostic: copy one simulation's HBM workspace to the host (layout: mpc_layout.h ws_carve).
int mpcb_debug_workspace(mpcb_handle *h, int inst, double *out, size_t n_doubles)
{
    if (!h || !out || !h->ready || inst < 0 || inst >= h->pb.batch) return MPCB_EINVAL;
    if (n_doubles > h->ws_stride) n_doubles = h->ws_stride;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(out, h->d_ws + (size_t)inst * h->ws_stride, n_doubles * sizeof(double), hipMemcpyDeviceToHost));
    return MPCB_OK;
}

int mpcb_summary(mpcb_handle *h, const mpcb_result *o, double *summary_dev, void *stream)
{
    if (!h) return MPCB_EINVAL;
    if (!h->ready) return fail(h, MPCB_ESTATE, "mpcb_summary before mpcb_setup");
    if (h->controller) return fail(h, MPCB_ESTATE, "mpcb_summary on a controller handle: it keeps no rollout logs");
    if (!o || !summary_dev || !o->errors || !o->status || !o->sqp_iter || !o->qp_iter || !o->residuals || !o->solver_time ||
        !o->plant_time)
        return fail(h, MPCB_EINVAL, "mpcb_summary needs the errors, status, iteration, residual and time arrays");
    HIPCHK(h, hipSetDevice(h->device));
    Outputs out;
    std::memcpy(&out, o, sizeof out);
    hipLaunchKernelGGL(mpc_summary_kernel, dim3((unsigned)h->pb.batch), dim3(WAVE), 0, (hipStream_t)stream, h->pb.batch, h->pb.Nsim,
                       h->d_params, out, summary_dev);
    HIPCHK(h, hipGetLastError());
    return MPCB_OK;
}

// Diagnostic (tests/test_gpu_parity.py): evaluate the device linearisation (task residual r, dg/dq, dg5/dqdot) at
// n points; params_host = n parameter records, x_host = n x 12 [q; qdot], rec_host = n x 60 (layout of a G2 record,
// mpc_layout.h O_R / O_GQ / O_GV).  Not part of include/mpcbatch.h.
int mpcb_debug_task_lin(mpcb_handle *h, int n, const double *params_host, const double *robot_host, const double *x_host,
                        double *rec_host)
{
    if (!h || n < 1 || !params_host || !robot_host || !x_host || !rec_host) return MPCB_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<InstParams> packed((size_t)n);
    for (int i = 0; i < n; i++) pack_inst_params(params_host + (size_t)i * MPCB_NPARAM, &packed[(size_t)i]);
    Robot rb;
    std::memcpy(&rb, robot_host, sizeof rb);
    InstParams *dp = nullptr;
    double *dx = nullptr, *dr = nullptr;
    int rc = MPCB_OK;
    if (hipMalloc((void **)&dp, n * sizeof(InstParams)) != hipSuccess || hipMalloc((void **)&dx, (size_t)n * 12 * 8) != hipSuccess ||
        hipMalloc((void **)&dr, (size_t)n * W2_LIN * 8) != hipSuccess)
        rc = fail(h, MPCB_ENOMEM, "hipMalloc(debug)");
    if (rc == MPCB_OK && (hipMemcpy(dp, packed.data(), n * sizeof(InstParams), hipMemcpyHostToDevice) != hipSuccess ||
                          hipMemcpy(dx, x_host, (size_t)n * 12 * 8, hipMemcpyHostToDevice) != hipSuccess))
        rc = fail(h, MPCB_EHIP, "hipMemcpy(debug in)");
    if (rc == MPCB_OK) {
        hipLaunchKernelGGL(mpc_debug_task_lin_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, nullptr, n, rb, dp, dx, dr);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(rec_host, dr, (size_t)n * W2_LIN * 8, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(h, MPCB_EHIP, "debug task_lin kernel");
    }
    if (dp) (void)hipFree(dp);
    if (dx) (void)hipFree(dx);
    if (dr) (void)hipFree(dr);
    return rc;
}

int mpcb_run(mpcb_handle *h, const mpcb_problem *p, const double *params_host, const double *robot_host,
             const mpcb_result *oh)
{
    if (!h) return MPCB_EINVAL;
    if (!oh) return fail(h, MPCB_EINVAL, "result pointer is NULL");
    int rc = mpcb_setup(h, p, params_host, robot_host);
    if (rc) return rc;
    const size_t B = (size_t)p->batch, T1 = (size_t)p->Nsim + 1, S = (size_t)p->Nsim;
    const size_t nd[6] = {12 * T1, 6 * T1, 12 * T1, 3 * T1, 6 * T1, 7 * T1};
    const size_t dbl_total = B * (nd[0] + nd[1] + nd[2] + nd[3] + nd[4] + nd[5] + 7 * S);
    const size_t int_total = B * 3 * S;
    double *dd = nullptr;
    int *di = nullptr;
    if (hipMalloc((void **)&dd, dbl_total * sizeof(double)) != hipSuccess) return fail(h, MPCB_ENOMEM, "hipMalloc(results)");
    if (hipMalloc((void **)&di, int_total * sizeof(int)) != hipSuccess) { (void)hipFree(dd); return fail(h, MPCB_ENOMEM, "hipMalloc(results)"); }
    mpcb_result od;
    double *pd = dd;
    od.z = pd; pd += B * nd[0];
    od.u = pd; pd += B * nd[1];
    od.ee_pose = pd; pd += B * nd[2];
    od.ee_rpy = pd; pd += B * nd[3];
    od.ee_vel = pd; pd += B * nd[4];
    od.errors = pd; pd += B * nd[5];
    od.residuals = pd; pd += B * 4 * S;
    od.cost = pd; pd += B * S;
    od.solver_time = pd; pd += B * S;
    od.plant_time = pd; pd += B * S;
    od.status = di; od.sqp_iter = di + B * S; od.qp_iter = di + 2 * B * S;
    rc = mpcb_rollout(h, 0, p->Nsim, &od, nullptr);
    if (rc == MPCB_OK) rc = mpcb_sync(h);
    if (rc == MPCB_OK) {
        struct { void *dst; const void *src; size_t n; } cp[] = {
            {oh->z, od.z, B * nd[0] * 8}, {oh->u, od.u, B * nd[1] * 8}, {oh->ee_pose, od.ee_pose, B * nd[2] * 8},
            {oh->ee_rpy, od.ee_rpy, B * nd[3] * 8}, {oh->ee_vel, od.ee_vel, B * nd[4] * 8}, {oh->errors, od.errors, B * nd[5] * 8},
            {oh->residuals, od.residuals, B * 4 * S * 8}, {oh->cost, od.cost, B * S * 8},
            {oh->solver_time, od.solver_time, B * S * 8}, {oh->plant_time, od.plant_time, B * S * 8}, {oh->status, od.status, B * S * 4},
            {oh->sqp_iter, od.sqp_iter, B * S * 4}, {oh->qp_iter, od.qp_iter, B * S * 4}};
        for (auto &c : cp) {
            if (!c.dst) continue;
            hipError_t e = hipMemcpy(c.dst, c.src, c.n, hipMemcpyDeviceToHost);
            if (e != hipSuccess) { rc = fail(h, MPCB_EHIP, "hipMemcpy(results)", e); break; }
        }
    }
    (void)hipFree(dd);
    (void)hipFree(di);
    return rc;
}

}  // extern "C"
