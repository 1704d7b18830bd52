// mpc_layout.h -- data layout of the batched MPC rollout engine (gfx950).
//
// One workgroup (1-8 wavefronts) owns one simulation instance.  All per-instance solver state
// lives in an HBM workspace, STAGE-MAJOR, split into five record groups so that every pass of
// the solver streams whole contiguous stage records:
//     G1 ITER  iterate + QP iterate      G2 LINR  linearisation + Newton right-hand sides
//     G3 STEP  residuals + Newton step   G4 FACT  Riccati factor (K, R^-1 h_u, e, p, P, w, R^-1)
//     G5 SQPX  SQP-only extras (NLP multipliers, trial point, merit weights)
// A pass copies a CHUNK of consecutive stages HBM -> LDS in one coalesced burst (16 B per
// lane, all loads in flight together), works on the chunk entirely in LDS -- the sequential
// Riccati recursions never touch HBM inside the stage loop -- and writes its outputs back in
// one burst.  This matters on gfx950 because a `s_waitcnt vmcnt` that covers a store costs
// ~1 us (stores are acknowledged from the memory side), so per-stage loads/stores would
// serialise the whole recursion on memory latency.
//
// Reference being replaced: simulator.py:199-241 (Simulator.run) and the acados / HPIPM
// solver behind trajectory_optimizer.py:183-186.
#pragma once

#include <stddef.h>

#define MPC_HD __host__ __device__ __forceinline__
// a solver pass: its own function (own register allocation) so the kernel does not become one
// giant inlined body that the register allocator spills
#define MPC_PASS __host__ __device__ __noinline__

namespace mpcb {

constexpr int WAVE = 64;
constexpr int NWV_MAX = 8;    // at most eight wavefronts cooperate on one simulation
constexpr int NT_MAX = WAVE * NWV_MAX;
constexpr int NQ = 6;   // joints
constexpr int NX = 12;  // state  x = [q; qdot]              (prediction_model.py:46)
constexpr int NU = 6;   // input  u = qdot_ref                (prediction_model.py:47)
constexpr int NW = 18;  // stage variable w = [u; q; qdot]
constexpr int NB = 12;  // bounded components per stage: u (6) then q (6)
constexpr int NL = 24;  // multipliers / slacks per stage: lower (12) then upper (12)
constexpr int NTASK = 5;

// ---- G1 ITER ----------------------------------------------------------------------
constexpr int W1 = 96;
constexpr int O_X = 0, O_U = 12, O_QW = 18, O_QPI = 36, O_QLAM = 48, O_QT = 72;
// ---- G2 LINR ----------------------------------------------------------------------
constexpr int W2 = 112;
constexpr int O_R = 0;     // r = g - g_ref (5)
constexpr int O_Y = 5;     // y = W (r + G delta) (5)
constexpr int O_BD = 12;   // dynamics defect of the NLP iterate (12)
constexpr int O_GQ = 24;   // d g / d q (5x6)
constexpr int O_GV = 54;   // d g5 / d qdot (6)
constexpr int O_GAM = 60;  // Gamma = lam/t (12)
constexpr int O_GT = 72;   // condensed gradient of the Newton system (18)
constexpr int O_RB = 90;   // dynamics residual of the QP iterate (12)
constexpr int W2_LIN = 60;   // [R..GV]: what a linearisation produces
// ---- G3 STEP ----------------------------------------------------------------------
constexpr int W3 = 144;
constexpr int O_RG = 0, O_RD = 18, O_RM = 42;  // residuals g (18), d (24), m (24)
constexpr int O_DW = 66;    // Newton step [du; dq; dqdot] (18)
constexpr int O_DPI = 84;   // step of the multiplier of dynamics k-1 -> k (12)   (note the shift)
constexpr int O_DLAM = 96, O_DT = 120;
// ---- G4 FACT ----------------------------------------------------------------------
// Ordered by consumer: the forward sweeps read a prefix ([K..E] predictor, [K..P] final sweep), the
// corrector reads K and the tail [w, R~^-1].
constexpr int W4 = 228;
constexpr int O_K = 0;      // Kfb = R~^-1 S~ (6x12)
constexpr int O_VH = 72;    // R~^-1 h_u (6)
constexpr int O_E = 78;     // e = rb - B R~^-1 h_u (12): the part of dx_{k+1} that does not depend on dx_k
constexpr int O_PV = 90;    // p_k (12)
constexpr int O_PM = 102;   // P_k, symmetric 12x12 PACKED: upper triangle by rows (78), see tri()
constexpr int NPM = 78;
constexpr int O_WV = 180;   // w_k = P_{k+1} rb_k (12): reused by the corrector's backward solve
constexpr int O_RI = 192;   // R~^-1 (6x6)
constexpr int W4_AFF = O_PV;   // what the predictor sweep loads
constexpr int W4_FWD = O_WV;   // what the final forward sweep loads
// ---- G5 SQPX ----------------------------------------------------------------------
constexpr int W5 = 116;
constexpr int O_NPI = 0, O_NLAM = 12, O_NT = 36, O_TX = 60, O_TU = 72, O_MW = 78;  // MW: dyn 12 + ineq 24

constexpr int STAGE_DOUBLES = W1 + W2 + W3 + W4 + W5;
// The scalars at the end of a simulation's workspace, carried from one launch to the next (`state`): slots
constexpr int ST_Z = 0;            // [12] plant state z
constexpr int ST_LIN_COST = 12;    // cost of the held linearisation
constexpr int ST_X0_MW = 13;       // [12] merit weights of the x0 constraint
constexpr int ST_LIN_VALID = 25;   // linearisation-valid flag
constexpr int ST_FAST = 26;        // [2] fast path: QPs left before the next attempt, length of the current suspension
constexpr int ST_CUR = 28;         // throughput engine, SQP_RTI: the slot of the stage records that holds the QP iterate (0: G1, 1: G3)
constexpr int ST_PROF = 32;        // [NPROF] profile counters (diagnostic build)
constexpr int NPROF = 16;
constexpr int ST_OBS = 48;         // [12] the rollout's disturbance observer (mpcb_rollout_obs): v^ [6] | d^ [6] of the next step
constexpr int STATE_DOUBLES = 64;

// Kinematic constants (robots.py KinematicChain.packed): 105 doubles
struct Robot {
    double place[7][12];  // [R row-major (9); p (3)] of joint i in its parent, [6] = EE frame
    double axis[6][3];
    double t_ee[3];       // prediction_model.py:9
};

// Per-instance parameters, one record per instance in HBM (packed by pack_inst_params).
struct InstParams {
    double dt, tol, qp_tol, w_u, w_qddot, px_ref, vy_ref, integ;   // integ: plant integrator code
    double wcv[6], q0[6], qdot0[6], qmin[6], qmax[6], umin[6], umax[6];
    double coeffs[6];   // a b c d e f   (surface.py:14-17)
    double w_task[5];   // trajectory_optimizer.py:44-48
    double lm;          // acados levenberg_marquardt: dt*lm*I on the stage Hessians, lm*I on the terminal one
    // derived on the host in C (prediction_model.py:87-115, 322-326)
    double a12[6], a22[6], b1[6], b2[6];
    double cq[6];       // qddot gain (1-a22)/Ts
    // acados nlp_solver_tol_eq / _ineq / _comp (`tol` above is nlp_solver_tol_stat)
    double tol_eq, tol_ineq, tol_comp;
    double n_hor;       // this simulation's prediction horizon when it differs from the launch's (throughput engine: ragged batches); 0 = Problem::N
    double fast_off;    // 0: the bound-inactive fast path of the QP solve is on (mpc_ipm.h, ipm::FAST_MARGIN); 1: every QP through the interior-point loop
};

// The cost weights that can change at run time (mpcb_set_weights): w_u, w_qddot, w_task[0..4] -- parameters [3], [4], [56..60] of the
// packed record, in this order.  Nothing else of InstParams is derived from them (mpc_pack.h pack_inst_params).
constexpr int NWEIGHT = 7;
MPC_HD void put_weights(InstParams &P, const double *w)
{
    P.w_u = w[0]; P.w_qddot = w[1];
    for (int i = 0; i < NTASK; i++) P.w_task[i] = w[2 + i];
}

// The joint-wise terminal cost of a controller step (mpcb_step_term): per simulation the 2x2 blocks (pqq_j, pqv_j, pvv_j) of the six
// joints and the terminal reference x_e = [q_e; qdot_e] -- NTERM doubles, in this order (formulas: mpc_nlp.h term_*).
constexpr int NTERM = 30;

// Batch-uniform problem description (== mpcb_problem).
struct Problem {
    int batch;
    int N;            // prediction_horizon
    int Nsim;         // closed-loop steps
    int solver_type;  // 0 = SQP, 1 = SQP_RTI
    int max_iter;     // nlp_solver_max_iter
    int qp_iter_max;  // HPIPM iter_max
    int fixed_step;   // globalization FIXED_STEP instead of MERIT_BACKTRACKING
    int precision;    // 0: fp64 everywhere; 1: Riccati factor and solve sweeps in fp32 (throughput engine only)
};

// Device pointers to the result logs (== mpcb_result), batch-major, per-instance shapes of
// the reference's logs (simulation_model.py:25-29, simulator.py:59-65).
struct Outputs {
    double *z;         // [batch][12][Nsim+1]
    double *u;         // [batch][6][Nsim+1]
    double *ee_pose;   // [batch][12][Nsim+1]
    double *ee_rpy;    // [batch][3][Nsim+1]
    double *ee_vel;    // [batch][6][Nsim+1]
    int *status;       // [batch][Nsim]
    int *sqp_iter;     // [batch][Nsim]
    int *qp_iter;      // [batch][Nsim]
    double *residuals; // [batch][Nsim][4]
    double *cost;      // [batch][Nsim]
    double *solver_time; // [batch][Nsim] seconds (device realtime counter)
    double *errors;    // [batch][7][Nsim+1]  e1..e5, p_task_z, p_ee_y (simulator.py:265-344)
    double *plant_time; // [batch][Nsim] seconds: plant step + FK / J qdot / error logging (simulator.py:224-226)
};

// Device pointers of one controller step (mpcb_step_io, then the task reference of mpcb_step_ref): the caller's feedback states in,
// solver.get(0,'u') and the step's statistics out, batch-major.  x_pred / u_pred may be null (not written).  The members past
// u_pred are not part of mpcb_step_io; an initialiser that stops at u_pred means "the packed references, unchanged", one that stops
// at ref_changed "every simulation carries its solver memory", one that stops at warm "no sensitivities", one that stops at sens_valid "none to the weights",
// one that stops at du0_dw "no terminal cost", one that stops at du0_dxe "no input disturbance", one that stops at dist "the packed surface".
struct StepIO {
    const double *xhat;  // [batch][12]
    double *u0;          // [batch][6]
    int *status;         // [batch]
    int *sqp_iter;       // [batch]
    int *qp_iter;        // [batch]
    double *residuals;   // [batch][4]
    double *cost;        // [batch]
    double *solver_time; // [batch] seconds (device realtime counter)
    double *x_pred;      // [batch][N+1][12] or null
    double *u_pred;      // [batch][N][6] or null
    const double *yref = nullptr;   // [batch][N][NTASK] targets of g1..g5 at stages 0..N-1, or null: each instance's packed g_ref
    int ref_changed = 0;            // != 0: the reference differs from the previous step's (the carried linearisation is stale)
    const int *warm = nullptr;      // [batch] WARM_* of each simulation (mpcb_step_warm), or null: WARM_CARRY for all
    // mpcb_step_sens (mpcb_step_sens_out): the feedback gain and reference sensitivity of u0, read by the sens kernels only
    double *du0_dx = nullptr;       // [batch][6][12] d u0 / d xhat
    double *du0_dyref = nullptr;    // [batch][N][NTASK][6] (d u0 / d yref_k)', or null (not written)
    int *sens_valid = nullptr;      // [batch] 1: exact sensitivities written, 0: NaN
    // mpcb_step_sens_w: the sensitivity of u0 to the seven cost weights, read by the sens_w kernels only
    double *du0_dw = nullptr;       // [batch][NWEIGHT][6] d u0 / d weight_p
    // mpcb_step_term: the joint-wise terminal cost and the sensitivity of u0 to its reference, read by the term kernels only
    const double *term = nullptr;   // [batch][NTERM] pqq 6 | pqv 6 | pvv 6 | x_e 12 (mpc_nlp.h term_*)
    double *du0_dxe = nullptr;      // [batch][6][12] d u0 / d x_e, or null (not written)
    // mpcb_step_dist: the input disturbance of the prediction model x+ = Ad x + Bd (u + d), read by the dist kernels only
    const double *dist = nullptr;   // [batch][6] d, rad/s
    // mpcb_step_surf: the surface window, row k = a..f at stage k, read by the surf kernels only
    const double *surf = nullptr;   // [batch][N][NSURF]
};

// How a simulation's solver memory enters a controller step (MPCB_WARM_*); any other value is WARM_CARRY.
constexpr int WARM_CARRY = 0, WARM_RESET = 1, WARM_SHIFT = 2;
// WARM_SHIFT moves the carried solver memory of a simulation of horizon N one stage towards stage 0.  Which stages hold a column of
// a stage record decides how it moves:
//   SH_X  a quantity of stages 0..N (states, state steps, equality multipliers): k <- k + 1 for k < N, stage N's stays (duplicated)
//   SH_U  a quantity of stages 0..N-1 (inputs, input steps, input-bound multipliers and slacks): k <- k + 1 for k < N - 1, stage N-1's
//         stays (the input is held)
//   SH_Q  as SH_U, of the state bounds (stages 1..N-1): stage 0 has none, so what arrives there is zeroed
// Afterwards x_N <- Ad x_N + Bd u_{N-1} from the old x_N and the held input (shift_tail): the tail stays dynamically feasible.
constexpr int SH_X = 0, SH_U = 1, SH_Q = 2;
MPC_HD int shift_class_bounds(int q) { return q % 12 < 6 ? SH_U : SH_Q; }   // q: column in [lower 12 | upper 12] x n, each u 6 | q 6
// column c of a G1 record (and of the QP iterate's second home on the throughput engine, G3 [O_DW, W3) = G1 [O_QW, W1))
MPC_HD int shift_class_g1(int c) { return c < O_U ? SH_X : c < O_QW + NU ? SH_U : c < O_QLAM ? SH_X : shift_class_bounds(c - O_QLAM); }
// column c of a G5 record: NLP multipliers, trial point, merit weights
MPC_HD int shift_class_g5(int c)
{
    return c < O_NLAM ? SH_X : c < O_TX ? shift_class_bounds(c - O_NLAM) : c < O_TU ? SH_X : c < O_MW ? SH_U
         : c < O_MW + 12 ? SH_X : c < O_MW + 36 ? shift_class_bounds(c - O_MW - 12) : SH_X;
}
// does stage k of a column of class cl take stage k + 1's value?
MPC_HD bool shift_moves(int cl, int k, int N) { return k < (cl == SH_X ? N : N - 1); }
// component i of the new x_N: x [12] the old x_N, u [6] the held u_{N-1}
template <class X, class U>
MPC_HD double shift_tail(const InstParams &P, int i, const X &x, const U &u)
{
    return i < 6 ? x[i] + P.a12[i] * x[6 + i] + P.b1[i] * u[i] : P.a22[i - 6] * x[i] + P.b2[i - 6] * u[i - 6];
}

// The task reference of one instance in a controller step: its [N][NTASK] rows of StepIO::yref, or null for the packed
// g_ref = [0, 1, 0, px_ref, vy_ref].  Also the tag that selects the reference-tracking variant of a pass (an overload taking
// it first), which only the controller step kernels instantiate: the rollout kernels keep their passes as they are.
struct TaskRef {
    const double *y;
};

// The plant perturbation of ONE simulation in a perturbed rollout (mpcb_plant_pert with the simulation's offsets applied): device
// pointers, each null = that perturbation off.  Read from global memory by the lanes that use them, during the launch only.
struct PlantPert {
    const double *wcv;      // [6]        the plant's bandwidths (the model keeps InstParams::wcv)
    const double *u_dist;   // [Nsim][6]  added to u_t before the plant step
    const double *x_noise;  // [Nsim][12] added to z_t to form the feedback state of step t
};
// ... of simulation `inst` of a launch (`a`: the three [batch][...] arrays)
MPC_HD PlantPert plant_pert_of(const PlantPert &a, int inst, int Nsim)
{
    return PlantPert{a.wcv ? a.wcv + (size_t)inst * 6 : nullptr, a.u_dist ? a.u_dist + (size_t)inst * Nsim * 6 : nullptr,
                     a.x_noise ? a.x_noise + (size_t)inst * Nsim * 12 : nullptr};
}

// Value of the engines' TERM flag in the kernels of mpcb_rollout_term: the terminal-cost record is two arrays (1, or true: the one
// record of mpcb_step_term).
constexpr int TERM_TABLE = 2;
// The terminal cost of ONE simulation in a rollout (mpcb_rollout_term; the simulation's offsets applied): its constant joint blocks
// [pqq 6 | pqv 6 | pvv 6] and its table of terminal references, row t = x_e of step t.  Device pointers, read during the launch only.
struct TermTab {
    const double *blocks;   // [18]
    const double *x_ref;    // [Nsim][12]
};
// ... of simulation `inst` of a launch (`a`: the two [batch][...] arrays)
MPC_HD TermTab term_tab_of(const TermTab &a, int inst, int Nsim)
{
    return TermTab{a.blocks + (size_t)inst * 18, a.x_ref + (size_t)inst * Nsim * 12};
}

// Value of the engines' DIST flag in the kernels of mpcb_rollout_obs: the model's input disturbance is the estimate of the rollout's own
// observer, kept in the engine's shared block (1, or true: the caller's device buffer of mpcb_step_dist).
constexpr int DIST_SHARED = 2;
// ... where entry j of that estimate lives in Smem::logv (and in the throughput engine's logv, same layout): the slots no log row
// uses, [21..23] and [43..45].  No kernel's shared block grows.
MPC_HD int lv_dhat(int j) { return j < 3 ? 21 + j : 40 + j; }
// The disturbance observer of ONE simulation in a rollout (mpcb_rollout_obs; the simulation's offsets applied): its gains, read once,
// and the log of its estimates, row t = the d^ that step t's model took -- written by the kernel, never read by it.
struct ObsArg {
    const double *gain;     // [12] l1 [6] | l2 [6]
    double *d_hat;          // [Nsim][6]
};
// ... of simulation `inst` of a launch (`a`: the two [batch][...] arrays)
MPC_HD ObsArg obs_arg_of(const ObsArg &a, int inst, int Nsim)
{
    return ObsArg{a.gain + (size_t)inst * 12, a.d_hat + (size_t)inst * Nsim * 6};
}
// A row of a surface table (mpcb_step_surf, mpcb_rollout_surf): the quadric's coefficients a b c d e f, as InstParams::coeffs.
constexpr int NSURF = 6;
static_assert(ST_OBS >= ST_PROF + NPROF && ST_OBS + 12 <= STATE_DOUBLES, "the observer's slots lie past the profile counters, inside the state block");

// One instance's workspace: five stage-major group arrays + persistent scalars.
struct Ws {
    double *G1, *G2, *G3, *G4, *G5, *PH, *state;
};
// Segmented residency of the latency engine (horizons whose Riccati factor does not fit a CU's LDS): the solve sweeps hold the
// factor of one SEGMENT of SEG_T transitions at a time (16 chunks of SEG_L); PH keeps the chunk transition matrices (12x12 each).
// Segment geometry by pool size: a whole CU's pool holds 16 chunks of 7 transitions, half a pool (two simulations per CU) 8 chunks of 5.
constexpr int SEG_L_FULL = 7, SEG_J_FULL = 16, SEG_L_HALF = 5, SEG_J_HALF = 8, SEG_POOL_FULL = 17000;
MPC_HD size_t ws_phi_doubles(int N) { return (size_t)((N + SEG_L_HALF - 1) / SEG_L_HALF + 1) * 144; }
// Residency predicates of the latency engine -- ONE formula for the device (Engine::resident_ok / segment_ok) and for mpcb_setup's choice
// of the launch geometry: per stage the solve sweeps keep K (72) | R~^-1 h_u (6) | e (12) | p (12) in LDS, plus one 12x12
// chunk transition matrix per lane group (`groups` = min(lanes / 16, 16)); the rest of the pool is scratch.
constexpr int RS_PER_STAGE_L = 72 + 6 + 12 + 12;
MPC_HD bool lay_resident_ok(int N, int pool_n, int groups)
{
    const int NS = N + 1, scr = pool_n - (NS * RS_PER_STAGE_L + groups * 144);
    // scratch: the factorisation's double-buffered chunks (>= 6 stages) ; the corrector's gt (18) + w (12) + slots
    return scr >= 4096 && scr >= NS * 30 + 2 * groups * 12 + 16;
}
MPC_HD bool lay_segment_ok(int N, int pool_n, int groups)
{
    if (groups < 8 || pool_n < SEG_POOL_FULL || lay_resident_ok(N, pool_n, groups)) return false;
    const int Jc = groups < SEG_J_FULL ? groups : SEG_J_FULL, T = SEG_L_FULL * Jc;
    const int scr = pool_n - ((T + 1) * RS_PER_STAGE_L + Jc * 144);
    return scr >= (T + 1) * 30 + 2 * groups * 12 + 64;
}

// offset of entry (r, c), r <= c, of a symmetric 12x12 matrix stored as its upper triangle by rows
MPC_HD int tri(int r, int c) { return r * 12 - (r * (r - 1)) / 2 + (c - r); }
MPC_HD int tri_sym(int i, int j) { return i <= j ? tri(i, j) : tri(j, i); }

MPC_HD size_t ws_doubles_per_instance(int N) { return (size_t)(N + 1) * STAGE_DOUBLES + ws_phi_doubles(N) + STATE_DOUBLES; }

MPC_HD Ws ws_carve(double *base, int N)
{
    const size_t n1 = (size_t)N + 1;
    Ws w;
    double *p = base;
    w.G1 = p; p += n1 * W1;
    w.G2 = p; p += n1 * W2;
    w.G3 = p; p += n1 * W3;
    w.G4 = p; p += n1 * W4;
    w.G5 = p; p += n1 * W5;
    w.PH = p; p += ws_phi_doubles(N);
    w.state = p;
    return w;
}

// rows of the per-step trajectory log: z 12 | u 6 | ee_pose 12 | ee_rpy 3 | ee_vel 6 | errors 7
constexpr int LOG_ROWS = 46, LOGB = 8;

// Static LDS working set of one simulation (workgroup); the chunk pool follows it (dynamic LDS).
// Every array is 16-byte aligned: the compiler merges neighbouring doubles into ds_read/write_b128,
// and a b128 DS access off its 16-byte alignment is replayed at ~64 cycles (MI355X_MICROARCH.md, LDS).
struct Smem {
    InstParams P;       // this instance's parameters (lane-indexed reads stay on chip)
    alignas(16) Robot rb;
    Ws w;                  // this instance's workspace pointers: kept here because the engine object lives in
    int n_hor, pool_n;     // scratch memory inside a non-inlined pass (a flat load + full wait per use); LDS is ~10x closer
    int prog;              // progress of the state recursion (last finished stage), Ex::post / await
    int prog1;             // progress of the follower recursion (vector half of the factorisation sweep)
    int flg[2];            // factorisation pipeline: input chunks landed, factor buffers released (counted per background wavefront)
    int flg_pad;
    alignas(16) double mt2[2][16];     // p_{k+1} + P_{k+1} rb_k hand-over slots (host executor only)
    alignas(16) double pv[2][12];
    alignas(16) double Rt[36];      // R~ = H_uu + Gamma_u + B'MB
    alignas(16) double St2[2][72];  // S~ double buffer of the factorisation sweep (stage k read, k-1 written)
    alignas(16) double Kf[72];      // R~^-1 S~
    alignas(16) double dx[2][12];
    alignas(16) double ret[8];      // results a pass hands back to the solver driver (every wavefront writes the same values)
    alignas(16) double cen[4];      // resident sweeps: step length and the three centering sums S0, S1, S2
    alignas(16) double bon[24];     // 1.0 where a bound exists: lower 12 (u 6 | q 6), upper 12 (stage rules: has_comp)
    alignas(16) double red[8][NWV_MAX];   // one partial per wavefront (Ex::put_* / get_*)
    alignas(16) double xhat[12];    // current plant state (feedback, simulator.py:206)
    alignas(16) double u0[6];
    alignas(16) double logv[48];    // [0..20] pose, rpy, J qdot | [24..35] next plant state | [36..42] task errors | lv_dhat: d^ (mpcb_rollout_obs)
    // log columns wait here until LOGB of them leave as contiguous runs (one 64-byte run per row and flush
    // instead of one 8-byte store per row and step)
    alignas(16) double logbuf[LOG_ROWS][LOGB];
};

// Chunk pool sizes (doubles).  The widest pass needs ~500 doubles per stage (+1 halo stage).
constexpr int POOL_MIN_DOUBLES = 2048;
constexpr int POOL_DEFAULT_DOUBLES = 19456;  // 152 KiB cap: one simulation per CU (batch <= 256 per GPU) gets all the LDS left beside Smem
constexpr int LDS_CU_BYTES = 160 * 1024;
// The chunk pool of one simulation when `sims_per_cu` simulations share a CU's LDS (mpcb_setup; the boundary tests read the same
// function through tests/emu): what is left beside Smem, capped at the default, at least the minimum, in whole 16-byte items.
MPC_HD int lay_pool_doubles(int sims_per_cu)
{
    const int fixed = (int)sizeof(Smem) + 64;
    int bytes = LDS_CU_BYTES / (sims_per_cu < 1 ? 1 : sims_per_cu) - fixed;
    if (bytes > POOL_DEFAULT_DOUBLES * 8) bytes = POOL_DEFAULT_DOUBLES * 8;
    if (bytes < POOL_MIN_DOUBLES * 8) bytes = POOL_MIN_DOUBLES * 8;
    return (bytes / 16) * 2;
}

}  // namespace mpcb
