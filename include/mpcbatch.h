/*
 * mpcbatch.h -- C ABI of libmpcbatch.so, the MI355X-native batched MPC rollout engine.
 *
 * Drop-in boundary for the hot path of lynet55/robotic-mpc:
 *     SimulationManager.run_all -> Simulator.__init__ / Simulator.run
 *     (simulator.py:641-676, 18-127, 199-241)
 * i.e. everything the reference does through acados_template's ctypes binding to its
 * per-instance generated libacados_ocp_solver_<model>.so:
 *     AcadosOcpSolver(ocp, json_file)            trajectory_optimizer.py:183-186
 *     solver.set(0,'lbx'|'ubx',x)                simulator.py:210-211
 *     solver.solve()                             simulator.py:212
 *     solver.get(0,'u')                          simulator.py:213
 *     solver.get_stats('sqp_iter'|'time_tot')    simulator.py:218,220
 *     solver.get_residuals(), get_cost()         simulator.py:219,221
 * plus the plant step and logging of simulation_model.Robot.update
 * (simulation_model.py:85-91).  Where the reference builds and drives ONE solver per
 * simulation, this ABI takes a BATCH of simulations (one 72-double parameter record each)
 * and runs all closed loops on the GPU, one wavefront per simulation.
 *
 * Conventions: plain C, no exceptions; every function returns 0 on success or a negative
 * MPCB_E* code, with text in mpcb_last_error(); the caller owns every buffer it passes;
 * a handle is bound to one device and is not thread-safe; per-simulation solver failures
 * are DATA (status arrays, acados codes 0/1/2/3/4), never call failures.
 * There is no CPU fallback: without a HIP device mpcb_create fails.
 */
#ifndef MPCBATCH_H
#define MPCBATCH_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCB_VERSION 200      /* 0.2.0 */
#define MPCB_NPARAM 72        /* doubles per simulation, layout below */
#define MPCB_NROBOT 105       /* doubles of kinematic constants, layout below */

#define MPCB_OK 0
#define MPCB_EINVAL (-1)      /* bad argument / inconsistent sizes */
#define MPCB_ENODEV (-2)      /* no usable HIP device */
#define MPCB_ENOMEM (-3)      /* device allocation failed */
#define MPCB_EHIP (-4)        /* HIP runtime error, see mpcb_last_error */
#define MPCB_ESTATE (-5)      /* call order violated (e.g. rollout before setup) */

#define MPCB_SOLVER_SQP 0     /* trajectory_optimizer.py:60 (default) */
#define MPCB_SOLVER_SQP_RTI 1 /* solver_options {'nlp_solver_type': 'SQP_RTI'} */

#define MPCB_PRECISION_FP64 0          /* everything in fp64 (the reference's arithmetic)                      */
#define MPCB_PRECISION_FP32_RICCATI 1  /* Riccati factor K, P, R~^-1, p and the three solve sweeps in fp32; iterate,
                                          residuals, right-hand sides, steps and all outputs stay fp64
                                          (BASELINE.json configs[4]; SQP_RTI on the throughput engine only).
                                          An OPT-IN study leg: slower than fp64 at every size measured (-6..-12 %),
                                          never chosen by mpcb_setup's routing -- only by this field.             */

/* Two kernel families sit behind this ABI: the LATENCY engine (one workgroup of 4-8
 * wavefronts and half or all of a CU's LDS per simulation; batches up to a few simulations per CU, and most SQP runs) and
 * the THROUGHPUT engine (one wavefront per simulation, records streamed; SQP_RTI batches of >= MPCB_STREAM_MIN_BATCH
 * simulations, full-SQP batches of >= MPCB_STREAM_MIN_BATCH_SQP simulations running >= MPCB_STREAM_MIN_STEPS_SQP steps,
 * every fp32-Riccati run, every ragged batch).  mpcb_setup picks; the environment variable MPCB_ENGINE=latency|stream
 * overrides the choice where both apply.  An SQP_RTI bucket of at least as many simulations as the GPU holds wavefronts of
 * the throughput engine (8 per CU) is launched as a work queue over (simulation, MPCB_STREAM_CHUNK = 10 closed-loop steps)
 * items: same results bit for bit, balanced launch (MPCB_STREAM_CHUNK=0 turns it off; a hand-off that does not complete
 * within a bound derived from the work limit of one chunk -- 4 x chunk steps x SQP iterations x QP iterations x (N+1) x 20 us
 * + 30 s; MPCB_QUEUE_TIMEOUT_S overrides it -- is reported by mpcb_sync as MPCB_EHIP instead of hanging). */
/* Measured crossovers, N=100, 600 steps, one MI355X, fast path of the QP solve on, the throughput engine's first pass of a step
 * item-parallel (profiles/r04_engine_sweep2.txt; latency engine two simulations per CU vs throughput engine, steps/s).  SQP_RTI: 1024
 * simulations 2.40 M vs 2.10 M, 1280: 2.34 M vs 2.55 M, 2048: 2.55 M vs 3.69 M, 4096: 2.67 M vs 4.08 M.  Full SQP: 2048 simulations
 * 474 k vs 435 k, 2560: 447 k vs 489 k, 4096: 503 k vs 601 k -- and once more at the round's last kernels (joint-angle sincos, SQP merit pass without
 * spills: the latency engine gained more; profiles/r04_engine_sweep3.txt): 2560: 620 k vs 600 k, 3072: 665 k vs 670 k, 3584: 686 k vs 715 k, 4096: 723 k
 * vs 758 k; 200 steps: 3072: 283 k vs 244 k, 4096: 308 k vs 307 k (after the throughput engine's last SQP fixes, r04_engine_sweep4.txt: 2560: 618 k
 * vs 615-647 k, 3072: 661-671 k vs 685-713 k, 4096: 845-870 k on the throughput engine; 3072 x 200 steps: 282 k vs 261 k -- thresholds unchanged).  SQP_RTI there: 1280: 2.49 M vs 2.60 M, 4096: 4.23 M on the throughput engine. */
#define MPCB_STREAM_MIN_BATCH_SQP 3072   /* full SQP: from this many simulations on ... */
#define MPCB_STREAM_MIN_STEPS_SQP 300    /* ... for runs of at least this many closed-loop steps */
#define MPCB_STREAM_MIN_BATCH 1280

typedef struct mpcb_handle mpcb_handle;

/* Batch-uniform part of the configuration (one launch = one bucket of simulations that
 * share these). Mirrors Simulator.__init__ / MPC.__init__ arguments as noted. */
typedef struct {
    int batch;        /* number of simulations in this call                               */
    int N;            /* prediction_horizon (simulator.py:42)                             */
    int Nsim;         /* int(simulation_time/dt) (simulator.py:41)                        */
    int solver_type;  /* MPCB_SOLVER_*                                                    */
    int max_iter;     /* nlp_solver_max_iter (trajectory_optimizer.py:67)                 */
    int qp_iter_max;  /* acados qp_solver_iter_max (default 50)                           */
    int fixed_step;   /* 1: globalization FIXED_STEP, 0: MERIT_BACKTRACKING (:68)         */
    int precision;    /* MPCB_PRECISION_*: arithmetic of the Riccati factor and solve sweeps */
} mpcb_problem;

/* Per-simulation parameter record, MPCB_NPARAM doubles (simulator.py:18-35):
 *   [0] dt  [1] tol (acados nlp tol, 1e-6)  [2] qp_tol (trajectory_optimizer.py:63)
 *   [3] w_u [4] w_qddot [5] px_ref [6] vy_ref [7] plant integrator (0 RK4, 1 Euler, 2 RK2, 3 RK3; simulation_model.py:39-49)
 *   [8..13] wcv   [14..19] q_0   [20..25] qdot_0   [26..31] q_min   [32..37] q_max
 *   [38..43] qdot_min (lbu)   [44..49] qdot_max (ubu)
 *   [50..55] surface_coeffs a,b,c,d,e,f (surface.py:14-17)
 *   [56..60] task weights (trajectory_optimizer.py:44-48, all 50.0)
 *   [61] nlp_solver_tol_eq [62] nlp_solver_tol_ineq [63] nlp_solver_tol_comp -- 0 means "same as [1]", which is
 *        nlp_solver_tol_stat (any acados option reaches the solver through simulator.py:129-135)
 *   [64] levenberg_marquardt (acados: dt*lm*I added to every stage Hessian, lm*I to the terminal one)
 *   [65] this simulation's prediction horizon, when the simulations of one call have DIFFERENT horizons ("ragged"
 *        batch, e.g. a grid search over prediction_horizon run as one launch): 1 <= [65] <= mpcb_problem.N, and
 *        mpcb_problem.N is the largest of them; 0 means N.  Ragged batches run on the throughput engine.
 *   [66] bound-inactive fast path of the QP solve (csrc/mpc_ipm.h): 0 = on (the default), 1 = off.  On: a QP whose
 *        equality-constrained minimiser -- ONE Riccati factorisation -- keeps every bounded component >= 1e-3 inside its bounds is
 *        solved by that factorisation alone (the solution of the strictly convex QP, lam = 0); every other QP, and every QP when
 *        off, goes through the HPIPM-style interior-point loop.  `qp_iter` then counts Riccati factorisations.  Not used by the
 *        fp32-Riccati leg (one fp32 solve is not a solution to qp_tol).
 *   [67..71] reserved (0)
 * Bounds with |value| >= 1e29 are treated as absent.
 *
 * Kinematic constants, MPCB_NROBOT doubles (what loader.py:24-36 extracts from the URDF):
 *   [0..83]  7 placements [R row-major (9); p (3)]: joint i in its parent at q=0, i=0..5,
 *            then the end-effector frame in the last link
 *   [84..101] 6 unit joint axes   [102..104] translation_ee_t (prediction_model.py:9)
 */

/* Result logs, batch-major; per simulation the shapes of the reference's own logs
 * (simulation_model.py:25-29, simulator.py:59-65).  T1 = Nsim+1. */
typedef struct {
    double *z;           /* [batch][12][T1]  q;qdot                      */
    double *u;           /* [batch][6][T1]   u[:,0]=qdot_0, u[:,i+1]=u_i */
    double *ee_pose;     /* [batch][12][T1]  p; R row-major              */
    double *ee_rpy;      /* [batch][3][T1]                               */
    double *ee_vel;      /* [batch][6][T1]   J_world * qdot              */
    int *status;         /* [batch][Nsim]    acados status 0/1/2/3/4     */
    int *sqp_iter;       /* [batch][Nsim]                                */
    int *qp_iter;        /* [batch][Nsim]    Riccati factorisations: interior-point iterations (+1 per fast-path attempt) */
    double *residuals;   /* [batch][Nsim][4] stat, eq, ineq, comp        */
    double *cost;        /* [batch][Nsim]                                */
    double *solver_time; /* [batch][Nsim]    device seconds of solver.solve() (simulator.py:209-214,220)  */
    double *errors;      /* [batch][7][T1]   e1..e5, p_task_z, p_ee_y of Simulator.errors (simulator.py:265-344),
                                             computed with the log column on the device                  */
    double *plant_time;  /* [batch][Nsim]    device seconds of the plant step + FK / J qdot / error logging
                                             (integration_time, simulator.py:224-226)                    */
} mpcb_result;

#define MPCB_NSUMMARY 24      /* doubles per simulation written by mpcb_summary, layout below */

int mpcb_version(void);
/* Number of HIP devices visible; 0 when none (never an error by itself). */
int mpcb_device_count(void);

/* Create a handle on `device` (>= 0).  Fails with MPCB_ENODEV when no GPU is usable. */
int mpcb_create(mpcb_handle **h, int device);
void mpcb_destroy(mpcb_handle *h);
const char *mpcb_last_error(const mpcb_handle *h);

/* Bytes of device workspace mpcb_setup will hold for `p`. */
size_t mpcb_workspace_bytes(const mpcb_problem *p);
/* Bytes of one simulation's result logs (sum over the mpcb_result arrays). */
size_t mpcb_result_bytes_per_sim(const mpcb_problem *p);

/* Replaces Simulator.__init__ + MPC.finalize_solver for the whole batch: packs the
 * parameter records (host pointers), uploads them, sizes the workspace.  No code generation. */
int mpcb_setup(mpcb_handle *h, const mpcb_problem *p, const double *params_host, const double *robot_host);

/* Replaces the Simulator.run loop for closed-loop steps [step0, step1) of every simulation.
 * `out_dev` holds DEVICE pointers (caller-allocated, e.g. torch tensors); `stream` is a
 * hipStream_t (NULL = default stream).  Asynchronous; step0 must continue where the previous
 * call stopped, or be 0, which restarts every simulation from its initial state. */
int mpcb_rollout(mpcb_handle *h, int step0, int step1, const mpcb_result *out_dev, void *stream);

/* Wait for the stream of the last rollout. */
int mpcb_sync(mpcb_handle *h);

/* Device time of the last mpcb_rollout launch, measured with HIP events on its stream (ms). */
int mpcb_last_kernel_ms(mpcb_handle *h, float *ms);

/* Static resources of the rollout kernel: VGPRs, SGPRs(0 if unknown), LDS bytes, scratch bytes. */
int mpcb_kernel_info(mpcb_handle *h, int *vgprs, int *sgprs, int *lds_bytes, int *scratch_bytes);

/* Kernel family mpcb_setup chose for the current problem: 0 latency engine, 1 throughput engine (< 0: error). */
int mpcb_engine(mpcb_handle *h);
/* The family mpcb_setup WOULD choose for a uniform (not ragged) problem of this shape: host logic only, no device touched. */
int mpcb_engine_for(const mpcb_problem *p);

/* Launch geometry chosen by mpcb_setup for the current batch: wavefronts cooperating on one
 * simulation (one workgroup per simulation), and the dynamic-LDS chunk pool per workgroup. */
int mpcb_launch_info(mpcb_handle *h, int *waves_per_sim, int *pool_bytes);

/* Replaces Simulator.metrics / solver_stats / timings / get_summary (simulator.py:347-448, 509-547) for the whole
 * batch: one pass over the device logs of a finished rollout.  `out_dev` as for mpcb_rollout; `summary_dev` is a
 * DEVICE array [batch][MPCB_NSUMMARY]:
 *   [0..4] rmse_e1..e5  [5..9] itse_e1..e5  [10] weighted_rmse  [11] total_sqp_iterations  [12] avg_sqp_iterations
 *   [13] num_failures  [14] max_kkt_residual  [15] total_solver_time  [16] avg_mpc_time  [17] avg_solver_time
 *   [18] avg_integration_time  [19] total_computation_time  [20] total_qp_iterations  [21..23] reserved.
 * mpc_time and solver_time are both the device time of the solve (no Python call overhead exists here),
 * integration_time is `plant_time`.  Asynchronous on `stream`. */
int mpcb_summary(mpcb_handle *h, const mpcb_result *out_dev, double *summary_dev, void *stream);

/* Convenience for callers without device buffers of their own: setup + rollout(0,Nsim) +
 * copy-back into HOST arrays `out_host`. */
int mpcb_run(mpcb_handle *h, const mpcb_problem *p, const double *params_host, const double *robot_host,
             const mpcb_result *out_host);

/* ---- controller step: the MPC solve from caller-supplied states, for a plant the caller owns ----
 * (acados solver.set(0,'lbx'|'ubx',x); solver.solve(); solver.get(0,'u') -- simulator.py:210-221 -- for a whole batch.)
 * All pointers are DEVICE pointers, batch-major.  x_pred / u_pred may be NULL (not written); every other array is required. */
typedef struct {
    const double *xhat;  /* [batch][12]     feedback state q;qdot of each simulation (in)                      */
    double *u0;          /* [batch][6]      solver.get(0,'u'): the input to apply                              */
    int *status;         /* [batch]         acados status 0/1/2/3/4                                            */
    int *sqp_iter;       /* [batch]                                                                            */
    int *qp_iter;        /* [batch]         Riccati factorisations, as in mpcb_result                          */
    double *residuals;   /* [batch][4]      stat, eq, ineq, comp                                               */
    double *cost;        /* [batch]                                                                            */
    double *solver_time; /* [batch]         device seconds of the solve                                        */
    double *x_pred;      /* [batch][N+1][12] predicted states x_0..x_N of the iterate, or NULL                 */
    double *u_pred;      /* [batch][N][6]   predicted inputs u_0..u_{N-1} of the iterate, or NULL              */
} mpcb_step_io;

/* Like mpcb_setup (same validation and packing; Nsim is checked but not used), for mpcb_step: always the latency engine,
 * at any batch size, with mpcb_setup's geometry rules.  Refuses ragged horizons (parameter [65] != 0 and != N) and
 * MPCB_PRECISION_FP32_RICCATI with MPCB_EINVAL (mpcb_setup_controller_on below runs the step on the throughput engine,
 * ragged horizons included).  On the handle this sets
 * up, mpcb_rollout and mpcb_summary return MPCB_ESTATE; mpcb_setup or mpcb_run set it up for rollouts again. */
int mpcb_setup_controller(mpcb_handle *h, const mpcb_problem *p, const double *params_host, const double *robot_host);

/* One MPC step of every simulation from the states io->xhat: the iterate, the linearisation and the QP memory carry
 * over from the previous step (the warm start of a real-time controller); `reset` != 0 starts from the initial guess
 * (x_k = [q_0; qdot_0], u_k = 0, multipliers 0), and so does the first step after mpcb_setup_controller.  No plant
 * step, no logs.  Asynchronous on `stream` (a hipStream_t, NULL = default stream), no host synchronisation;
 * mpcb_sync and mpcb_last_kernel_ms apply to it.  MPCB_ESTATE on a handle not set up by mpcb_setup_controller.
 * mpcb_kernel_info and mpcb_launch_info report the step kernel on a controller handle. */
int mpcb_step(mpcb_handle *h, const mpcb_step_io *io, int reset, void *stream);

/* ---- the controller step against a time-varying task reference (acados solver.set(k, 'yref', ...) between solves) ---- */
#define MPCB_NREF 5              /* task outputs g1..g5: S(x,y) - z, n . z_task, y_task.x, p_x, v_task.y    */
/* mpcb_step with the targets of the five task outputs given per simulation AND per stage: the stage-k residual is
 * g(x_k) - yref[i][k] instead of g(x_k) - g_ref, g_ref = [0, 1, 0, px_ref, vy_ref] the references packed by mpcb_setup_controller
 * (parameters [5] and [6]).  `yref` is a DEVICE pointer [batch][N][MPCB_NREF], N the longest horizon of the batch (stage N
 * has no task cost, so there is no row N); on a ragged batch rows k >= the simulation's own horizon are never read.  NULL means
 * the packed references.  The targets of the u and qddot cost rows stay 0.  The array is read during the launch only (the
 * reference in force is the caller's to keep: pass it again with every step).
 * `ref_changed` != 0 says that the reference differs from the previous step's (NULL counting as the packed one): the step then
 * linearises again at its start instead of reusing the linearisation carried from the previous step, which was formed against the
 * old reference.  Everything else carries as in mpcb_step.  With yref == NULL and ref_changed == 0 this is mpcb_step exactly:
 * mpcb_step(h, io, reset, s) == mpcb_step_ref(h, io, NULL, 0, reset, s).  MPCB_ESTATE on a handle not set up as a controller. */
int mpcb_step_ref(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, int reset, void *stream);

/* ---- the controller step with a warm start chosen per simulation ---- */
#define MPCB_WARM_CARRY 0        /* iterate, linearisation and QP memory carry over (mpcb_step)                       */
#define MPCB_WARM_RESET 1        /* this simulation starts from the initial guess, as `reset` does for the whole batch  */
#define MPCB_WARM_SHIFT 2        /* the carried solver memory moves one stage towards stage 0 before the step           */
/* mpcb_step_ref with one mode per simulation: `warm` is a DEVICE array [batch] of MPCB_WARM_* (any other value counts as
 * MPCB_WARM_CARRY), read during the launch only; NULL means MPCB_WARM_CARRY for all, and then this is mpcb_step_ref exactly:
 * mpcb_step_ref(h, io, y, rc, reset, s) == mpcb_step_warm(h, io, y, rc, NULL, reset, s).
 * MPCB_WARM_SHIFT is the shift initialisation of a receding horizon whose schedule moves one stage per step: the previous solution
 * at stage k + 1 is the guess for stage k.  For a simulation of horizon N (its own horizon on a ragged batch):
 *   u_k <- u_{k+1} for k = 0..N-2, u_{N-1} is held;  x_k <- x_{k+1} for k = 0..N-1;
 *   x_N <- Ad x_N + Bd u_{N-1} from the old x_N and the held input, so the tail stays dynamically feasible;
 *   every other quantity carried between steps and indexed by stage moves with its stage, the last stage's duplicated: the equality
 *   multipliers (stages 0..N), the bound multipliers and slacks of the QP memory and the per-stage merit weights (stages 0..N-1);
 *   stage 0 has no state bounds, so what arrives there from stage 1's state bounds is zeroed;
 *   what is kept per simulation stays (the last feedback state, the fast-path suspension, the x_0 merit weights);
 *   the carried linearisation of a shifted simulation is stale: that simulation linearises again at the start of the step, as
 *   after ref_changed, and its neighbours keep theirs;  rows past a simulation's own horizon are not touched.
 * N = 1 is legal (nothing moves in u, x_0 <- x_1, x_1 is propagated again).  On the first step after mpcb_setup_controller, or with
 * `reset` != 0, every mode is a reset.  MPCB_ESTATE on a handle not set up as a controller. */
int mpcb_step_warm(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed,
                   const int *warm /* DEVICE [batch] or NULL */, int reset, void *stream);

/* ---- the controller step with the feedback gain and the reference sensitivity of u0 ---- */
/* For an SQP_RTI step whose QP was solved by an accepted bound-inactive fast-path attempt (status 0), u0 = U_0 + du_0 with du the
 * solution of the bound-free Gauss-Newton QP at the carried linearisation point: an affine function of the feedback state xhat and of
 * the task reference.  Its exact Jacobians, the linearisation point held fixed (the derivatives of this step's QP):
 *   du0_dx[i]        = d u0 / d xhat            6 x 12 (minus the stage-0 Riccati gain)
 *   du0_dyref[i][k]  = (d u0 / d yref_k)'       5 x 6, k = 0 .. N-1, N the longest horizon of the batch
 * Row k = 0 is exactly zero (x_0 is pinned to xhat); on a ragged batch so are the rows k >= the simulation's own horizon.
 * Where they do not exist -- the QP went through the interior-point loop (fast path off, attempt rejected, attempt skipped during a
 * back-off suspension) or status != 0 -- every entry of both arrays of that simulation is NaN and valid[i] = 0.  Sensitivities through
 * active bounds, and of x_pred / u_pred, are not provided. */
typedef struct {
    double *du0_dx;     /* [batch][6][12]                          */
    double *du0_dyref;  /* [batch][N][5][6], N the longest horizon; may be NULL */
    int    *valid;      /* [batch] 1: exact sensitivities written, 0: NaN */
} mpcb_step_sens_out;   /* device pointers */
/* mpcb_step_warm that also writes the sensitivities.  sens == NULL is mpcb_step_warm exactly (the same kernel, bit-identical outputs):
 * mpcb_step_warm(h, io, y, rc, w, reset, s) == mpcb_step_sens(h, io, y, rc, w, reset, NULL, s).  With sens the step itself (u0,
 * statistics, prediction, solver memory) is what it is without.  MPCB_EINVAL on a full-SQP controller or with du0_dx or valid NULL;
 * MPCB_ESTATE on a handle not set up as a controller. */
int mpcb_step_sens(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, const int *warm, int reset,
                   const mpcb_step_sens_out *sens, void *stream);

/* ---- run-time cost weights, and the sensitivity of u0 to them ---- */
#define MPCB_NWEIGHT 7   /* w_u, w_qddot, task weights of g1..g5: parameters [3], [4], [56..60], in this order */
/* Overwrites the seven cost weights of every simulation's device parameter record with `weights`, a DEVICE array
 * [batch][MPCB_NWEIGHT].  Asynchronous on `stream` (a small kernel); the array is read during that launch only.  Ordering against
 * the steps is the caller's: set the weights on the stream of the steps, or order the streams with an event, so that no step is
 * running while the weights change and the next one starts after they have.  Nothing else of the record depends on the weights.
 * The handle remembers that the carried linearisation is stale: the next mpcb_step* linearises again at its start for every
 * simulation, exactly as after ref_changed != 0.  Everything else carries (the iterate, the multipliers, the QP memory, the merit
 * weights, the fast-path suspension).  The weights stay in force across steps and resets until they are set again or
 * mpcb_setup_controller* packs the configuration's own.  They are not validated: keep every weight >= 0 and
 * w_u + w_qddot + levenberg_marquardt > 0, or the input Hessian is singular.
 * MPCB_ESTATE on a handle not set up as a controller, MPCB_EINVAL on NULL. */
int mpcb_set_weights(mpcb_handle *h, const double *weights /* DEVICE [batch][MPCB_NWEIGHT] */, void *stream);

/* mpcb_step_sens that also writes du0_dw[i][p] = d u0 / d weight_p, 6 doubles each: DEVICE [batch][MPCB_NWEIGHT][6].
 * du0_dw == NULL is mpcb_step_sens exactly.  sens (with du0_dx and valid) is required; sens->du0_dyref may be NULL.
 * Where valid[i] == 0 every entry of du0_dw[i] is NaN.
 * Like du0_dx, this is the exact derivative of this step's QP with its linearisation point held fixed (the QP's matrices are affine
 * in the weights): of one real-time iteration, not of a converged solve, and without the dependence of the carried iterate on
 * the weights of earlier steps.  A weight of 0 has its derivative.  With a horizon of 1 the five task rows are exactly zero. */
int mpcb_step_sens_w(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, const int *warm, int reset,
                     const mpcb_step_sens_out *sens, double *du0_dw, void *stream);

/* ---- joint-wise terminal cost with a terminal reference ---- */
#define MPCB_NTERM 30   /* pqq[6] pqv[6] pvv[6] x_e[12] */
/* mpcb_step_sens with a terminal cost on the last stage of each simulation's horizon (SQP_RTI controllers):
 *   l_N(x) = 1/2 sum_j [q_j - q_e,j, v_j - v_e,j] [[pqq_j, pqv_j], [pqv_j, pvv_j]] [.]',   x = [q; qdot], x_e = [q_e; qdot_e],
 * one symmetric 2x2 block per joint -- the shape of the discrete LQR cost-to-go of this prediction model, six decoupled two-state
 * joints, for diagonal state and input weights.  It is NOT scaled by dt.  term[i] = pqq[6] | pqv[6] | pvv[6] | x_e[12] of simulation i,
 * a DEVICE array [batch][MPCB_NTERM] read during the launch only, like yref; all-zero blocks are exactly no terminal cost.  Keep every
 * block positive semidefinite (pqq, pvv >= 0, pqq pvv >= pqv^2); nothing is validated.
 * In the Gauss-Newton QP of the step at the iterate (X, U), with P the 12x12 matrix of the blocks:
 *   H_N = levenberg_marquardt I + P,   g_N = P (X_N - x_e);
 * the cost output adds l_N at the returned iterate and the stage-N rows of the stationarity residual include P (X_N - x_e); the
 * bound-inactive fast path and the interior-point loop both solve this QP.  On a ragged batch stage N is each simulation's own
 * horizon end.  MPCB_WARM_SHIFT is unchanged (x_N is propagated by the model as before).
 * term_changed != 0 (the blocks or x_e differ from the previous step's, or the terminal cost was switched on or off) makes every
 * simulation linearise again at the start of the step, exactly as ref_changed does.
 * With sens, du0_dx and du0_dyref are the exact Jacobians of this QP as before (the gain recursion starts from P_N), and
 * du0_dxe[i] = d u0 / d x_e, DEVICE [batch][6][12] or NULL, is written next to them: NaN where valid[i] == 0.  With a horizon of 1 it
 * is not zero.
 * term == NULL && term_changed == 0 && du0_dxe == NULL is mpcb_step_sens exactly (same kernels, same bits); term == NULL with
 * term_changed != 0 is mpcb_step_sens from a fresh linearisation.  MPCB_EINVAL: term != NULL on a full-SQP controller; du0_dxe
 * without sens or without term.  MPCB_ESTATE on a handle not set up as a controller.  The weight sensitivity (mpcb_step_sens_w) is
 * not offered together with a terminal cost. */
int mpcb_step_term(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, const int *warm, int reset,
                   const mpcb_step_sens_out *sens, const double *term /* DEVICE [batch][MPCB_NTERM] or NULL */, int term_changed,
                   double *du0_dxe /* DEVICE [batch][6][12] or NULL */, void *stream);

/* ---- input disturbance in the prediction model (offset-free MPC) ---- */
/* mpcb_step_warm whose prediction model carries a constant input disturbance (SQP_RTI controllers): dist[i] = d of simulation i, six
 * doubles in rad/s (the units of u), a DEVICE array [batch][6] read during the launch only, like yref; constant over the horizon.
 *   x_{k+1} = Ad x_k + Bd (u_k + d), k = 0 .. N-1;   qddot_k = (qdot_{k+1} - qdot_k) / dt of that model = cq_j (u_j + d_j - v_j).
 * The input cost row stays u (not u + d) and the bounds on u stay lbu / ubu.  In the Gauss-Newton QP of the step at the iterate (X, U):
 *   b_k = Ad X_k + Bd (U_k + d) - X_{k+1},   residual rows 11..16 gain (Sel Bd / dt) d,   g_k = dt Jr' W r with that residual,
 * H_k is unchanged -- the Riccati factorisation, the fast-path test and the interior point are the ones of mpcb_step_warm.  The cost
 * output and the stat / eq residual norms are those of this problem.  MPCB_WARM_SHIFT propagates the tail with this step's
 * disturbance, x_N <- Ad x_N + Bd (u_{N-1} + d); the reset guess is unchanged (x_k = [q_0; qdot_0], u_k = 0).  d = 0 is the
 * arithmetic of mpcb_step_warm.  Both engines run it, ragged horizons included on the throughput engine.
 * dist_changed != 0 (d differs from the previous step's, or the disturbance was switched on or off) makes every simulation
 * linearise again at the start of the step, exactly as ref_changed does.  An estimate that moves every step sets it every step.
 * dist == NULL && dist_changed == 0 is mpcb_step_warm exactly (same kernels, same bits); dist == NULL with dist_changed != 0 is
 * mpcb_step_warm from a fresh linearisation (the disturbance switched off).  MPCB_EINVAL: dist != NULL on a full-SQP controller.
 * MPCB_ESTATE on a handle not set up as a controller.  The sensitivities (mpcb_step_sens), the weight sensitivity
 * (mpcb_step_sens_w) and the terminal cost (mpcb_step_term) are not offered together with a disturbance; d u0 / d d is not
 * offered, nor a per-stage disturbance profile.  (A rollout whose steps take the estimate of an on-device observer: mpcb_rollout_obs.) */
int mpcb_step_dist(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, const int *warm, int reset,
                   const double *dist /* DEVICE [batch][6] or NULL */, int dist_changed, void *stream);

/* ---- a scheduled, stage-varying surface in the controller step ---- */
#define MPCB_NSURF 6 /* a row of a surface table: a b c d e f of S(x, y) = a x^2 + b y^2 + c x y + d x + e y + f (parameters [50..55]) */
/* mpcb_step_warm whose task functions are evaluated on a surface that differs from stage to stage (SQP_RTI controllers): surf[i][k] =
 * the six coefficients of simulation i at stage k = 0 .. N_i - 1, a DEVICE array [batch][N][MPCB_NSURF], N = mpcb_problem.N (the
 * longest horizon of the batch; rows past a simulation's own horizon are never read), read during the launch only, like yref.  At
 * stage k the row replaces parameters [50..55] wherever the task functions use them: S, its gradient (Sx, Sy), the unit normal n
 * and the derivatives of n in g1 = S(X, Y) - Z and g2 = n . z_task, in the residual r_k, in the Jacobian of the Gauss-Newton QP
 * (H_k, g_k) and in the cost.  g3, g4 and g5 do not depend on the surface.  Stage N has no task residual.  The reset guess, the
 * warm-start modes and everything that carries are those of mpcb_step_warm.  Both engines run it, ragged horizons included on the
 * throughput engine.  A window whose every row equals the packed coefficients is the arithmetic of mpcb_step_warm.
 * surf_changed != 0 (the window differs from the previous step's -- a window that slides along a table does at every step -- or it
 * was switched on or off) makes every simulation linearise again at the start of the step, exactly as ref_changed does.
 * surf == NULL && surf_changed == 0 is mpcb_step_warm exactly (same kernels, same bits); surf == NULL with surf_changed != 0 is
 * mpcb_step_warm from a fresh linearisation (the window switched off: the packed surface again).  MPCB_EINVAL: surf != NULL on a
 * full-SQP controller.  MPCB_ESTATE on a handle not set up as a controller.  The sensitivities (mpcb_step_sens, mpcb_step_sens_w),
 * the terminal cost (mpcb_step_term) and the input disturbance (mpcb_step_dist) are not offered together with a surface window. */
int mpcb_step_surf(mpcb_handle *h, const mpcb_step_io *io, const double *yref, int ref_changed, const int *warm, int reset,
                   const double *surf /* DEVICE [batch][N][MPCB_NSURF] or NULL */, int surf_changed, void *stream);

/* ---- the controller step on either kernel family ---- */
#define MPCB_ENGINE_AUTO (-1)    /* mpcb_controller_engine_for decides                                  */
#define MPCB_ENGINE_LATENCY 0    /* one workgroup of 4-8 wavefronts per simulation (mpc_step_kernel)     */
#define MPCB_ENGINE_STREAM 1     /* one wavefront per simulation (mpc_stream_step_kernel)                */
/* Crossover of the controller step (profiles/controller_step_rate_stream.txt): N = 100, SQP_RTI, a closed loop of 600 steps over a
 * torch RK4 plant, device time of the 600 step launches, latency vs throughput engine: 1024 simulations 272 vs 313 ms, 1280: 346 vs
 * 338 ms, 2048: 492 vs 399 ms, 4096: 925 vs 694 ms (1.33x; kernel trace at 4096: median step 1404 vs 990 us).  Full SQP never crossed
 * over: at 4096 simulations 5.70 s vs 9.35 s -- a step launch ends with its slowest simulation, and in the settling phase that is a
 * chain of many SQP iterations, which the latency engine's four wavefronts per simulation run faster than one (a rollout's work
 * queue spreads such chains over its items; one step cannot).  So a uniform full-SQP batch stays on the latency engine. */
#define MPCB_STREAM_MIN_BATCH_STEP 1280       /* SQP_RTI: the throughput engine from this many simulations on */

/* Like mpcb_setup_controller, on the kernel family `engine` (MPCB_ENGINE_*).  MPCB_ENGINE_LATENCY is mpcb_setup_controller.
 * MPCB_ENGINE_STREAM runs each simulation's step on one wavefront, and accepts ragged horizons (parameter [65], SQP_RTI only,
 * as in a rollout); mpcb_problem.N is then the longest horizon, and the rows of x_pred / u_pred beyond a simulation's own
 * horizon are written as NaN.  MPCB_ENGINE_AUTO takes mpcb_controller_engine_for's choice; there, and only there, the environment
 * variable MPCB_ENGINE=latency|stream overrides it for a uniform batch.  MPCB_EINVAL: an unknown engine, ragged horizons on the
 * latency engine or with full SQP, MPCB_PRECISION_FP32_RICCATI on any engine.  mpcb_step, mpcb_engine, mpcb_kernel_info and
 * mpcb_launch_info (1 wavefront per simulation, no LDS pool) report the family chosen. */
int mpcb_setup_controller_on(mpcb_handle *h, const mpcb_problem *p, const double *params_host, const double *robot_host, int engine);

/* The family MPCB_ENGINE_AUTO picks for the controller step of `p` (0 latency, 1 throughput engine; < 0: error).  Host logic only,
 * no device touched.  `ragged` != 0: the simulations have different horizons (always the throughput engine).  A uniform SQP_RTI
 * batch goes to the throughput engine from MPCB_STREAM_MIN_BATCH_STEP simulations on, a uniform full-SQP batch to the latency
 * engine at every size.  Nsim is ignored: a controller has no run length. */
int mpcb_controller_engine_for(const mpcb_problem *p, int ragged);

/* ---- rollouts that track a time-varying task reference schedule ---- */
/* mpcb_rollout whose closed loop tracks a schedule of the five task targets instead of the two constants packed at setup
 * (parameters [5] and [6]).  `yref_sched` is a DEVICE pointer [batch][Nsim + N][MPCB_NREF], N = mpcb_problem.N (the longest horizon
 * of the batch); row r of a simulation is the target at time r * dt.  Closed-loop step t (0 <= t < Nsim) of simulation i, of own
 * horizon N_i, uses yref_sched[i][t + k] as the target of g1..g5 at stage k = 0 .. N_i - 1; row t, t = 0 .. Nsim, is also what
 * column t of the `errors` log is measured against (hence Nsim + N rows, which keeps N = 1 legal):
 *   e1 = g1 - y0, e2 = y1 - n . z_task, e3 = y_task.x - y2, e4 = y3 - X, e5 = y4 - v_task.y   (rows 5 and 6 unchanged)
 * -- with the packed row [0, 1, 0, px_ref, vy_ref] the formula of mpcb_rollout term by term; mpcb_summary reduces the logged rows.
 * The array is read during the launch only; pass the same array to every launch of one run.
 *
 * Step t is mpcb_step_ref(window t, ref_changed = 1) followed by the built-in plant step and log: it linearises at its start
 * against its own window, and its cost and residuals are those of the returned iterate against window t.  The iterate, the
 * multipliers, the QP memory, the merit weights and the fast-path suspension carry as in mpcb_rollout; the warm start is not
 * shifted.  An SQP_RTI step therefore runs one NLP pass more than mpcb_rollout's.  Measured at N = 100, 600 steps
 * (profiles/rollout_ref_rate.txt, device time): 1.09x mpcb_rollout's time at 256 simulations on the latency engine, 1.24x at 4096 on
 * the throughput engine (queued; the deferred norms are lost too) -- and 1 / 1.20 and 1 / 1.17 of the 600 mpcb_step_ref launches it
 * replaces.
 *
 * yref_sched == NULL is mpcb_rollout exactly (the same kernels).  Whichever engine mpcb_setup chose runs the scheduled rollout, work
 * queue and ragged horizons included.  MPCB_ESTATE on a controller handle or before mpcb_setup; MPCB_EINVAL with
 * MPCB_PRECISION_FP32_RICCATI; the step-range rules of mpcb_rollout. */
int mpcb_rollout_ref(mpcb_handle *h, int step0, int step1, const mpcb_result *out_dev,
                     const double *yref_sched /* DEVICE [batch][Nsim + N][MPCB_NREF] or NULL */, void *stream);

/* ---- rollouts over a perturbed plant: model mismatch, input disturbance, measurement noise ---- */
/* mpcb_rollout_ref whose built-in plant is not the model the controller predicts with.  With z the TRUE plant state (q; qdot) of
 * simulation i:
 *   z_0 = [q_0; qdot_0]
 *   for t = 0 .. Nsim - 1:
 *       xhat_t  = z_t + x_noise[i][t]                        what the controller sees
 *       u_t     = u0 of mpcb_step_ref(xhat_t, window t of yref_sched, ref_changed = 1)
 *       z_{t+1} = plant step (the configured integrator, wcv[i], dt) from z_t with the input u_t + u_dist[i][t]
 * The solver memory carries as in mpcb_rollout_ref, the first step starts from the packed initial guess x_k = [q_0; qdot_0] (not from
 * xhat_0), and there is no shift.  The logs record the truth: z, ee_pose, ee_rpy, ee_vel and errors come from z_t (errors against
 * schedule row t, as in mpcb_rollout_ref), u[:, t + 1] = u_t is the COMMANDED input (not u_t + u_dist); cost, residuals, status,
 * sqp_iter and qp_iter are those of the step solved from xhat_t.  The model keeps the bandwidths of parameter [8..13].
 *
 * Every member is a DEVICE pointer and may be NULL (= that perturbation off); the arrays are read during the launch only -- pass the
 * same arrays to every launch of one run: what carries from one launch (and one work-queue item) to the next is the true state, and
 * each forms its first feedback state from x_noise[step0].  No row Nsim is read.
 *
 * pert == NULL is mpcb_rollout_ref exactly (the same kernels, the same bits).  pert != NULL with all three members NULL is legal:
 * the nominal loop through the kernels of the perturbed rollout (the scheduled rollout's results to rounding; its plant step runs
 * after the solve, never inside the last NLP pass).  pert != NULL needs yref_sched (MPCB_EINVAL without: a run without a schedule
 * passes the packed row [0, 1, 0, px_ref, vy_ref] on every row) and fp64 (MPCB_EINVAL with MPCB_PRECISION_FP32_RICCATI).
 * MPCB_ESTATE on a controller handle or before mpcb_setup; the step-range rules of mpcb_rollout.  Whichever engine mpcb_setup chose
 * runs it, work queue and ragged horizons included; mpcb_queue_used and mpcb_last_kernel_ms apply, and after such a launch
 * mpcb_kernel_info reports the perturbed rollout's kernel.  The 30 values a step reads are fetched from global memory by the lanes
 * that use them: no workspace, LDS or mpcb_workspace_bytes changes.  Measured at N = 100, 600 steps
 * (profiles/rollout_pert_rate.txt, device time): 1.02x mpcb_rollout_ref's time at 256 simulations on the latency engine (the plant
 * step and the log of the new state follow the solve), 1.001x at 4096 on the throughput engine (queued). */
typedef struct {
    const double *wcv;     /* [batch][6]        the plant's bandwidths                                  */
    const double *u_dist;  /* [batch][Nsim][6]  added to u_t before the plant step                      */
    const double *x_noise; /* [batch][Nsim][12] added to z_t to form the feedback state of step t       */
} mpcb_plant_pert;

int mpcb_rollout_pert(mpcb_handle *h, int step0, int step1, const mpcb_result *out_dev,
                      const double *yref_sched /* DEVICE [batch][Nsim + N][MPCB_NREF] */, const mpcb_plant_pert *pert /* or NULL */,
                      void *stream);

/* ---- rollouts with the joint-wise terminal cost and a table of terminal references ---- */
/* mpcb_rollout_pert whose step t closes the horizon of every simulation i with the terminal cost of mpcb_step_term (the QP terms,
 * the cost and the stationarity rows are described in the comment there):
 *   l_N(x) = 1/2 (x - term_xref[i][t])' P_i (x - term_xref[i][t])   at the last stage of the simulation's own horizon,
 * P_i the six 2x2 joint blocks term_blocks[i] = pqq[6] | pqv[6] | pvv[6], constant over the run; row t of term_xref[i] is x_e of step
 * t, so a tracking task can move the terminal reference with the tool.  It is the closed loop
 *   u_t = u0 of mpcb_step_term(xhat_t, window t of yref_sched, ref_changed = 1, term = [term_blocks[i] | term_xref[i][t]])
 * over the plant of mpcb_rollout_pert (pert == NULL: the nominal plant; the same kernels serve both).  A step linearises again at its
 * start, so a new row needs nothing else: nothing new carries between steps, launches or work-queue items, and there is no shift.
 * Both arrays are DEVICE pointers read during the launch only, by uniform loads where stage N uses them -- 18 + 12 doubles per step,
 * no [batch][Nsim][30] table, no workspace, LDS or mpcb_workspace_bytes change; pass the same arrays to every launch of one run.
 * Keep every block positive semidefinite; nothing is validated.  All-zero blocks are no terminal cost, through these kernels.
 *
 * term_blocks == NULL is mpcb_rollout_pert exactly (the same kernels, the same bits; term_xref is then ignored).  MPCB_EINVAL:
 * term_blocks with MPCB_PRECISION_FP32_RICCATI, on a full-SQP problem, without yref_sched (a run without a schedule passes the
 * packed row on every row) or without term_xref.  MPCB_ESTATE on a controller handle or before mpcb_setup; the step-range rules of
 * mpcb_rollout.  Whichever engine mpcb_setup chose runs it, work queue and ragged horizons included; mpcb_queue_used and
 * mpcb_last_kernel_ms apply, and after such a launch mpcb_kernel_info reports this rollout's kernel. */
int mpcb_rollout_term(mpcb_handle *h, int step0, int step1, const mpcb_result *out_dev,
                      const double *yref_sched /* DEVICE [batch][Nsim + N][MPCB_NREF] */, const mpcb_plant_pert *pert /* or NULL */,
                      const double *term_blocks /* DEVICE [batch][18] or NULL */,
                      const double *term_xref /* DEVICE [batch][Nsim][12] */, void *stream);

/* ---- rollouts with an on-device disturbance observer: offset-free MPC over the perturbed plant ---- */
/* mpcb_rollout_pert whose step t predicts with the input disturbance of mpcb_step_dist, estimated inside the kernel from the measured
 * velocities.  Per joint j of simulation i, with a22, b2 of the MODEL (parameters [8..13], dt) and obs_gain[i] = l1[6] | l2[6]:
 *   v^_0 = y_0,  d^_0 = 0
 *   for t = 0 .. Nsim - 1:
 *       xhat_t  = z_t + x_noise[i][t],   y_t = its velocities (what the observer measures is what the controller sees)
 *       u_t     = u0 of mpcb_step_dist(xhat_t, window t of yref_sched, ref_changed = 1, dist = d^_t, dist_changed = 1);  d_hat[i][t] = d^_t
 *       z_{t+1} = plant step of mpcb_rollout_pert from z_t with u_t + u_dist[i][t]
 *       v^_{t+1} = a22 v^_t + b2 (u_t + d^_t) + l1 (y_t - v^_t),   d^_{t+1} = d^_t + l2 (y_t - v^_t)      (u_t: the COMMANDED input)
 * -- the two-state Luenberger predictor of robotic_mpc_amd/observer.py (DisturbanceObserver.update), whose gains for both error poles
 * at p are l1 = a22 + 1 - 2 p, l2 = (1 - p)^2 / b2.  Logs, errors, cost and residuals follow mpcb_rollout_pert; cost and residuals
 * are those of the problem with d^_t.  There is no shift.  obs_gain is a DEVICE array read during the launch; d_hat is a DEVICE array
 * the launch WRITES (rows [step0, step1)) and never reads: the step's estimate stays on chip, and what carries from one launch (and
 * one work-queue item) to the next are the twelve doubles (v^, d^) in the simulation's workspace, next to the true state -- no
 * workspace, pool or mpcb_workspace_bytes change.  l2 = 0 keeps d^ at zero: the perturbed rollout through these kernels.
 *
 * obs_gain == NULL is mpcb_rollout_pert exactly (the same kernels, the same bits; d_hat is then ignored).  MPCB_EINVAL: obs_gain
 * without d_hat or without yref_sched (a run without a schedule passes the packed row on every row), on a full-SQP problem, or with
 * MPCB_PRECISION_FP32_RICCATI.  MPCB_ESTATE on a controller handle or before mpcb_setup; the step-range rules of mpcb_rollout.
 * Whichever engine mpcb_setup chose runs it, work queue and ragged horizons included; mpcb_queue_used and mpcb_last_kernel_ms apply,
 * and after such a launch mpcb_kernel_info reports this rollout's kernel.  Not offered together with the terminal cost
 * (mpcb_rollout_term) or the sensitivities. */
int mpcb_rollout_obs(mpcb_handle *h, int step0, int step1, const mpcb_result *out_dev,
                     const double *yref_sched /* DEVICE [batch][Nsim + N][MPCB_NREF] */, const mpcb_plant_pert *pert /* or NULL */,
                     const double *obs_gain /* DEVICE [batch][12] = l1[6] | l2[6], or NULL */,
                     double *d_hat /* DEVICE [batch][Nsim][6], written: row t = the estimate step t used */, void *stream);

/* ---- rollouts over a scheduled, stage-varying surface ---- */
/* mpcb_rollout_pert whose surface moves with time: `surf_sched` is a DEVICE pointer [batch][Nsim + N][MPCB_NSURF], N =
 * mpcb_problem.N (the longest horizon of the batch); row r of a simulation is a, b, c, d, e, f at time r * dt.  Closed-loop step t
 * (0 <= t < Nsim) of simulation i, of own horizon N_i, uses surf_sched[i][t + k] at stage k = 0 .. N_i - 1 (stage N_i has no task
 * residual), and column t of the `errors` log, t = 0 .. Nsim, is measured against surface row t and reference row t.  It is the
 * closed loop
 *   u_t = u0 of mpcb_step_surf(xhat_t, window t of yref_sched, ref_changed = 1, surf = window t of surf_sched, surf_changed = 1)
 * over the plant of mpcb_rollout_pert (pert == NULL: the nominal plant; the same kernels serve both); cost and residuals are those
 * of the returned iterate against window t.  Everything that carries in mpcb_rollout_pert carries, and nothing more: a step
 * linearises again at its start, the row index is the absolute step number, and there is no shift.  The array is read during the
 * launch only, by the lanes that linearise a stage (six doubles each) and by uniform loads for the error log: no workspace, LDS or
 * mpcb_workspace_bytes change; pass the same array to every launch of one run.
 *
 * surf_sched == NULL is mpcb_rollout_pert exactly (the same kernels, the same bits).  A schedule whose every row equals the packed
 * coefficients gives the perturbed rollout's results through these kernels.  MPCB_EINVAL: surf_sched on a full-SQP problem, with
 * MPCB_PRECISION_FP32_RICCATI or without yref_sched (a run without a reference schedule passes the packed row on every row).
 * MPCB_ESTATE on a controller handle or before mpcb_setup; the step-range rules of mpcb_rollout.  Whichever engine mpcb_setup chose
 * runs it, work queue and ragged horizons included; mpcb_queue_used and mpcb_last_kernel_ms apply, and after such a launch
 * mpcb_kernel_info reports this rollout's kernel.  Not offered together with the terminal cost (mpcb_rollout_term), the disturbance
 * observer (mpcb_rollout_obs) or the sensitivities.  Measured at 600 steps (profiles/rollout_surf_rate.txt, device time, an all-equal
 * schedule against mpcb_rollout_pert on the same closed loop): 1.018x at 256 simulations on the latency engine and 1.008x at 4096 on
 * the throughput engine (queued) at N = 100, 1.011x and 1.018x at N = 20; the loop of mpcb_step_surf launches it replaces takes
 * 1.17x - 1.73x.  The 256-register latency kernels hold 40 - 48 bytes more scratch per lane than the perturbed rollout's (the row is
 * live from the end of the kinematics through the Jacobian loop); the throughput engine's kernel holds what it held. */
int mpcb_rollout_surf(mpcb_handle *h, int step0, int step1, const mpcb_result *out_dev,
                      const double *yref_sched /* DEVICE [batch][Nsim + N][MPCB_NREF] */, const mpcb_plant_pert *pert /* or NULL */,
                      const double *surf_sched /* DEVICE [batch][Nsim + N][MPCB_NSURF] or NULL */, void *stream);

/* ---- rollouts with the shift warm start ---- */
/* mpcb_rollout_surf in which every simulation chooses how its solver memory enters a step: `warm` is a DEVICE array [batch] of
 * MPCB_WARM_CARRY | MPCB_WARM_SHIFT, the mode of simulation i, constant over the run (any value other than MPCB_WARM_SHIFT counts
 * as carry, as in mpcb_step_warm; one uniform load per simulation and launch or work item).  It is the closed loop
 *   u_t = u0 of mpcb_step_warm(xhat_t, window t of yref_sched, ref_changed = 1, warm[i] = (t >= 1 ? mode_i : MPCB_WARM_CARRY))
 * over the plant of mpcb_rollout_pert (pert == NULL: the nominal plant); with a surface table, mpcb_step_surf with window t of
 * surf_sched takes the place of mpcb_step_warm.  t is the absolute step number: the first step of a run starts from the initial
 * guess and does not shift; the first step of a later launch and the first step of a later work-queue item do.  The windows of
 * mpcb_rollout_ref, _pert and _surf slide one row per step, so stage k + 1 of step t - 1 and stage k of step t read the same rows
 * of the tables: the shifted iterate is linearised where the previous step left the solution of those rows, the carried one a stage
 * late.  Everything MPCB_WARM_SHIFT moves or keeps is as stated for mpcb_step_warm: the tail x_N <- Ad x_N + Bd u_{N-1} at each
 * simulation's own horizon end on a ragged batch, zeros for what arrives at stage 0 from stage 1's state bounds, N = 1 legal.
 * Nothing new carries between steps, launches or work-queue items: no workspace, LDS or mpcb_workspace_bytes change.
 *
 * warm == NULL is mpcb_rollout_surf exactly (the same kernels, the same bits); with surf_sched == NULL as well that is
 * mpcb_rollout_pert.  MPCB_EINVAL: warm on a full-SQP problem (there the shift costs iterations in the start-up transient and the
 * loops converge to the same point), with MPCB_PRECISION_FP32_RICCATI or without yref_sched (a run without a reference schedule
 * passes the packed row on every row).  MPCB_ESTATE on a controller handle or before mpcb_setup; the step-range rules of
 * mpcb_rollout.  Whichever engine mpcb_setup chose runs it, work queue and ragged horizons included; mpcb_queue_used and
 * mpcb_last_kernel_ms apply, and after such a launch mpcb_kernel_info reports this rollout's kernel.  Not offered together with the
 * terminal cost (mpcb_rollout_term) or the disturbance observer (mpcb_rollout_obs).  Device time against mpcb_rollout_pert, the
 * share of the shift pass and the loop of mpcb_step_warm launches it replaces: profiles/rollout_shift_rate.txt; what the shift does
 * to the closed loop: profiles/rollout_shift_closed_loop.txt. */
int mpcb_rollout_warm(mpcb_handle *h, int step0, int step1, const mpcb_result *out_dev,
                      const double *yref_sched /* DEVICE [batch][Nsim + N][MPCB_NREF] */, const mpcb_plant_pert *pert /* or NULL */,
                      const double *surf_sched /* DEVICE [batch][Nsim + N][MPCB_NSURF] or NULL */,
                      const int *warm /* DEVICE [batch] of MPCB_WARM_CARRY | MPCB_WARM_SHIFT, or NULL */, void *stream);

/* ---- terminal cost, input disturbance / observer, scheduled surface and shift in ONE step and ONE rollout ---- */
/* The entries above each add one closed-loop capability and refuse the others.  These two run all four at once, opt-in; nothing above
 * changes.  Both are SQP_RTI and fp64 only (MPCB_EINVAL otherwise), on whichever engine the handle was set up with, ragged horizons
 * and the work queue included.
 *
 * One kernel per entry and engine, not one per subset.  Each of term, dist / obs, surf and warm may be NULL = that feature is absent
 * for the whole batch; a simulation of a batch that does not use a feature brings NEUTRAL data for it:
 *   terminal cost      zero blocks (x_e is then multiplied by zeros; any finite rows)
 *   disturbance        d = 0 (step); observer gains l1 = l2 = 0 (rollout): d^ stays 0, and u + 0.0 is exact
 *   surface            a window / table whose rows all equal the simulation's own packed a..f
 *   warm start         MPCB_WARM_CARRY
 * The HOST fills the neutral tables, the kernels take no branch on a null pointer: for a NULL argument these entries fill them in
 * device memory the handle keeps for this purpose (allocated and filled at the first such call after a setup, once every argument has
 * been validated -- that one call synchronises its stream -- sized by the tables it stands for, reused by later calls, freed by
 * mpcb_destroy; the workspace and mpcb_workspace_bytes do not grow).  A caller who passes all tables allocates nothing here.
 *
 * mpcb_step_combined: one real-time iteration of the NLP in which stage k evaluates its task outputs on row k of `surf`
 * (mpcb_step_surf), the model is x+ = Ad x + Bd (u + d), d = `dist`, with the qddot rows of that model (mpcb_step_dist), and
 * l_N = 1/2 (x_N - x_e)' P (x_N - x_e) from `term` is added, not scaled by dt (mpcb_step_term).  With MPCB_WARM_SHIFT the carried
 * memory moves one stage first and the tail is x_N <- Ad x_N + Bd (u_{N-1} + d), THIS step's d.  term_changed, dist_changed and
 * surf_changed act as ref_changed does.  No sensitivities.  Array shapes as in the single-feature entries.  MPCB_ESTATE on a handle
 * not set up as a controller.
 *
 * mpcb_rollout_combined: the closed loop over the plant of mpcb_rollout_pert in which step t -- t the absolute step number, in every
 * launch and work-queue item -- is
 *   mpcb_step_combined(xhat_t, window t of yref_sched, ref_changed = 1, warm = (t >= 1 ? mode_i : MPCB_WARM_CARRY),
 *                      term = [blocks_i | x_ref[i][t]], dist = d^_t, surf = rows t .. t + N of surf_sched)
 * with d^_t the estimate of the observer of mpcb_rollout_obs (d^_0 = 0), written to d_hat[i][t] BEFORE the shift, which uses it.
 * Step 0 never shifts.  On a ragged batch the terminal cost sits on each simulation's own last stage.  Nothing new carries: d^
 * crosses a launch in the slots mpcb_rollout_obs uses.  MPCB_ESTATE on a controller handle or before mpcb_setup; the step-range rules
 * of mpcb_rollout; yref_sched is required (the packed rows when there is none).  After such a launch mpcb_kernel_info reports this
 * rollout's kernel.  Device time against the single-feature rollouts: profiles/rollout_combined_rate.txt. */
typedef struct {
    const double *blocks;  /* DEVICE [batch][18]        pqq 6 | pqv 6 | pvv 6, as mpcb_rollout_term's term_blocks */
    const double *x_ref;   /* DEVICE [batch][Nsim][12]  row t = x_e of step t                                      */
} mpcb_term_table;
typedef struct {
    const double *gain;    /* DEVICE [batch][12]        l1[6] | l2[6], as mpcb_rollout_obs's obs_gain              */
    double *d_hat;         /* DEVICE [batch][Nsim][6]   written: row t = the estimate step t used                  */
} mpcb_observer;
int mpcb_step_combined(mpcb_handle *h, const mpcb_step_io *io, const double *yref /* DEVICE [batch][N][MPCB_NREF] or NULL */,
                       int ref_changed, const int *warm /* DEVICE [batch] of MPCB_WARM_* or NULL */, int reset,
                       const double *term /* DEVICE [batch][30] or NULL */, int term_changed,
                       const double *dist /* DEVICE [batch][6] or NULL */, int dist_changed,
                       const double *surf /* DEVICE [batch][N][MPCB_NSURF] or NULL */, int surf_changed, void *stream);
int mpcb_rollout_combined(mpcb_handle *h, int step0, int step1, const mpcb_result *out_dev,
                          const double *yref_sched /* DEVICE [batch][Nsim + N][MPCB_NREF] */, const mpcb_plant_pert *pert /* or NULL */,
                          const mpcb_term_table *term /* or NULL */, const mpcb_observer *obs /* or NULL */,
                          const double *surf_sched /* DEVICE [batch][Nsim + N][MPCB_NSURF] or NULL */,
                          const int *warm /* DEVICE [batch] of MPCB_WARM_CARRY | MPCB_WARM_SHIFT, or NULL */, void *stream);

/* 1: the last mpcb_rollout / mpcb_rollout_ref / mpcb_rollout_pert / mpcb_rollout_term / mpcb_rollout_obs / mpcb_rollout_surf / mpcb_rollout_warm launch of this handle went through the throughput
 * engine's work queue, 0: it did not (< 0: error).  Host state only. */
int mpcb_queue_used(mpcb_handle *h);

#ifdef __cplusplus
}
#endif
#endif /* MPCBATCH_H */
