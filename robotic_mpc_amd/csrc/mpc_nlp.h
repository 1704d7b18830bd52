// mpc_nlp.h -- the formulas ABOVE the QP that BOTH engines use (latency engine mpc_core.h, throughput engine mpc_stream.h), in one
// place, as mpc_ipm.h holds the interior-point ones: the plant step, the L1 merit function of the SQP line search and its weights,
// the layout of the trajectory log, the writers of a step's statistics.  oracle/mpc_oracle.c stays an independent restatement.
// Small inline functions of scalars and of ACCESSORS: the callers own the data movement, and every operand keeps the address space
// the caller gave it (an LDS row, an MPC_GLOBAL pointer, a register array) because the operand types are template parameters -- a
// plain `const double *` here would turn them into flat loads (comment above struct Ctx) or push a register array into scratch.
// Everything compiles on the host (tests/emu).
#pragma once
#include <math.h>

#include "mpc_layout.h"

namespace mpcb {
namespace nlp {

// One joint of the plant step (simulation_model.py:93-117): Euler / RK2 (midpoint) / RK3 / RK4 of z' = [qdot; -W (qdot - u)]
MPC_HD void plant_rk(const InstParams &P, int j, double q, double v, double u, double &qn, double &vn)
{
    const double wc = P.wcv[j], dt = P.dt;
    const int integ = (int)P.integ;
    const double k1q = v, k1v = -wc * v + wc * u;
    const double v2 = v + 0.5 * dt * k1v;
    const double k2q = v2, k2v = -wc * v2 + wc * u;
    if (integ == 1) {
        qn = q + dt * k1q; vn = v + dt * k1v;
    } else if (integ == 2) {
        qn = q + dt * k2q; vn = v + dt * k2v;
    } else if (integ == 3) {
        const double v3 = v - dt * k1v + 2.0 * dt * k2v;
        const double k3q = v3, k3v = -wc * v3 + wc * u;
        qn = q + (dt / 6) * (k1q + 4.0 * k2q + k3q); vn = v + (dt / 6) * (k1v + 4.0 * k2v + k3v);
    } else {
        const double v3 = v + 0.5 * dt * k2v;
        const double k3q = v3, k3v = -wc * v3 + wc * u;
        const double v4 = v + dt * k3v;
        const double k4q = v4, k4v = -wc * v4 + wc * u;
        qn = q + (dt / 6) * k1q + (dt / 3) * k2q + (dt / 3) * k3q + (dt / 6) * k4q;
        vn = v + (dt / 6) * k1v + (dt / 3) * k2v + (dt / 3) * k3v + (dt / 6) * k4v;
    }
}

// The same with the joint's bandwidth given (the perturbed rollout, mpcb_rollout_pert: the plant's `wc` is not the model's P.wcv[j]).
// The formulas are restated, not shared: the function above keeps its code.
MPC_HD void plant_rk(const InstParams &P, double wc, double q, double v, double u, double &qn, double &vn)
{
    const double dt = P.dt;
    const int integ = (int)P.integ;
    const double k1q = v, k1v = -wc * v + wc * u;
    const double v2 = v + 0.5 * dt * k1v;
    const double k2q = v2, k2v = -wc * v2 + wc * u;
    if (integ == 1) {
        qn = q + dt * k1q; vn = v + dt * k1v;
    } else if (integ == 2) {
        qn = q + dt * k2q; vn = v + dt * k2v;
    } else if (integ == 3) {
        const double v3 = v - dt * k1v + 2.0 * dt * k2v;
        const double k3q = v3, k3v = -wc * v3 + wc * u;
        qn = q + (dt / 6) * (k1q + 4.0 * k2q + k3q); vn = v + (dt / 6) * (k1v + 4.0 * k2v + k3v);
    } else {
        const double v3 = v + 0.5 * dt * k2v;
        const double k3q = v3, k3v = -wc * v3 + wc * u;
        const double v4 = v + dt * k3v;
        const double k4q = v4, k4v = -wc * v4 + wc * u;
        qn = q + (dt / 6) * k1q + (dt / 3) * k2q + (dt / 3) * k3q + (dt / 6) * k4q;
        vn = v + (dt / 6) * k1v + (dt / 3) * k2v + (dt / 3) * k3v + (dt / 6) * k4v;
    }
}

// One joint of the rollout's disturbance observer (mpcb_rollout_obs; robotic_mpc_amd/observer.py DisturbanceObserver.update, one step
// earlier in time): from the estimate (v, d) that step t used, its measured velocity y and its commanded input u, the estimate of
// step t + 1 -- v+ = a22 v + b2 (u + d) + l1 (y - v), d+ = d + l2 (y - v).  Two chains of fused multiply-adds, written out so that
// both engines and the host emulation round alike.
MPC_HD void observer_next(double a22, double b2, double l1, double l2, double y, double u, double &v, double &d)
{
    const double e = y - v;
    v = fma(a22, v, fma(b2, u + d, l1 * e));
    d = fma(l2, e, d);
}

// ---- SQP line search: MERIT_BACKTRACKING (trajectory_optimizer.py:68; acados alpha_reduction, alpha_min) -------------------------
// trial steps 1, 0.7, 0.49, ... while >= 0.05
constexpr double LS_REDUCTION = 0.7, LS_ALPHA_MIN = 0.05;

// Leineweber's rule for a merit weight (acados merit_backtracking_*_weights): `a` = |multiplier| of the QP just solved, `w` the
// weight so far (not read by the first QP of a solve)
MPC_HD double merit_weight(int sqp_iter, double w, double a) { return sqp_iter == 0 ? a : fmax(a, 0.5 * (w + a)); }

// Stationarity of the QP at stage 0 with respect to x_0 component i (q: i < 6, qdot: i >= 6); its absolute value is the multiplier
// of the eliminated x_0 constraint, which the x_0 merit weights follow.  r1, r2: the stage-0 records of G1 and G2, O_Y holding
// W (r + G delta).
template <class R1, class R2>
MPC_HD double x0_stationarity(const InstParams &P, int i, R1 r1, R2 r2)
{
    if (i < 6) {
        double s = 0.0;
#pragma unroll
        for (int t = 0; t < NTASK; t++) s += r2[O_GQ + t * 6 + i] * r2[O_Y + t];
        return P.dt * s + r1[O_QPI + i] + P.dt * P.lm * r1[O_QW + 6 + i];
    }
    const int jj = i - 6;
    const double uj = r1[O_U + jj] + r1[O_QW + jj], vj = r1[O_X + 6 + jj] + r1[O_QW + 12 + jj];
    const double c2 = P.w_qddot * P.cq[jj] * P.cq[jj];
    return P.dt * (r2[O_GV + jj] * r2[O_Y + 4] + c2 * (vj - uj)) + P.a12[jj] * r1[O_QPI + jj] + P.a22[jj] * r1[O_QPI + 6 + jj] +
           P.dt * P.lm * r1[O_QW + 12 + jj];
}

// The same with the input disturbance d of the model x+ = Ad x + Bd (u + d) (mpcb_step_dist): dj = d_{i-6} enters the qddot term of
// the qdot rows (i >= 6; not read for i < 6).  Restated, not shared: the function above keeps its code.
template <class R1, class R2>
MPC_HD double x0_stationarity(const InstParams &P, int i, R1 r1, R2 r2, double dj)
{
    if (i < 6) return x0_stationarity(P, i, r1, r2);
    const int jj = i - 6;
    const double uj = (r1[O_U + jj] + r1[O_QW + jj]) + dj, vj = r1[O_X + 6 + jj] + r1[O_QW + 12 + jj];
    const double c2 = P.w_qddot * P.cq[jj] * P.cq[jj];
    return P.dt * (r2[O_GV + jj] * r2[O_Y + 4] + c2 * (vj - uj)) + P.a12[jj] * r1[O_QPI + jj] + P.a22[jj] * r1[O_QPI + 6 + jj] +
           P.dt * P.lm * r1[O_QW + 12 + jj];
}

// L1 merit function (acados ocp_nlp_evaluate_merit_fun restated), stage k < N at a trial point: stage cost, weighted dynamics
// defect against the next stage's trial state, weighted bound violations, added to `acc` term by term (a lane that sums several
// stages keeps one running sum).  xx[12] | uu[6]: trial state and input; res(i): task residual i, any reference subtracted;
// xnext(i): component i of the next stage's trial state; mw[36]: merit weights, dynamics 12 | lower 12 (u 6, q 6) | upper 12.
// Branch-free (every lane-dependent branch costs a saved exec mask: the latency engine's pass ran out of SGPRs).
template <class X, class U, class Res, class Xn, class Mw>
MPC_HD void merit_stage(double &acc, const InstParams &P, const X &xx, const U &uu, Res &&res, Xn &&xnext, const Mw &mw, int k)
{
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NTASK; i++) {
        const double r = res(i);
        s += P.w_task[i] * r * r;
    }
#pragma unroll
    for (int j = 0; j < 6; j++) {
        const double qdd = P.cq[j] * (uu[j] - xx[6 + j]);
        s += 2.0 * P.w_u * uu[j] * uu[j] + P.w_qddot * qdd * qdd;
        const double xnq = xnext(j), xnv = xnext(6 + j);
        acc += mw[j] * fabs((xx[j] + P.a12[j] * xx[6 + j] + P.b1[j] * uu[j]) - xnq);
        acc += mw[6 + j] * fabs((P.a22[j] * xx[6 + j] + P.b2[j] * uu[j]) - xnv);
        const double vl = P.umin[j] - uu[j], vu = uu[j] - P.umax[j];
        acc += mw[12 + j] * fmax(vl, 0.0) + mw[24 + j] * fmax(vu, 0.0);
        const double ql = P.qmin[j] - xx[j], qu = xx[j] - P.qmax[j], on = k >= 1 ? 1.0 : 0.0;
        acc += on * (mw[18 + j] * fmax(ql, 0.0) + mw[30 + j] * fmax(qu, 0.0));
    }
    acc += 0.5 * P.dt * s;
}
// ... and the term of the eliminated constraint x_0 = x_hat (stage 0 only): w0[12] its merit weights
template <class W0, class Xh, class X>
MPC_HD void merit_x0(double &acc, const W0 &w0, const Xh &xhat, const X &xx)
{
#pragma unroll
    for (int i = 0; i < 12; i++) acc += w0[i] * fabs(xhat[i] - xx[i]);
}

// ---- trajectory log (mpc_layout.h LOG_ROWS): z 12 | u 6 | ee_pose 12 | ee_rpy 3 | ee_vel 6 | errors 7 ------------------------------
// the value of log row `row`: xhat[12] the plant state, u0[6] its input, logv = [pose 12 | rpy 3 | J qdot 6 | ... | errors 7 at 36]
template <class Xh, class U0, class Lv>
MPC_HD double log_value(int row, const Xh &xhat, const U0 &u0, const Lv &logv)
{
    return row < 12 ? xhat[row] : row < 18 ? u0[row - 12] : row < 30 ? logv[row - 18] : row < 33 ? logv[12 + (row - 30)]
         : row < 39 ? logv[15 + (row - 33)] : logv[36 + (row - 39)];
}
// where log row `row` of instance `inst` goes: its [T1] columns in the arrays of `out`
MPC_HD double *log_row(const Outputs &out, int inst, int row, size_t T1)
{
    return row < 12 ? out.z + ((size_t)inst * 12 + row) * T1
         : row < 18 ? out.u + ((size_t)inst * 6 + (row - 12)) * T1
         : row < 30 ? out.ee_pose + ((size_t)inst * 12 + (row - 18)) * T1
         : row < 33 ? out.ee_rpy + ((size_t)inst * 3 + (row - 30)) * T1
         : row < 39 ? out.ee_vel + ((size_t)inst * 6 + (row - 33)) * T1
                    : out.errors + ((size_t)inst * 7 + (row - 39)) * T1;
}

// ---- a step's statistics, to entry `at` of the arrays of O = Outputs or StepIO: one lane each --------------------------------------
template <class O>
MPC_HD void put_solve(const O &o, size_t at, int lane, int status, int sqp_iter, int qp_iter, double solver_time)
{
    if (lane == 8) { o.status[at] = status; o.sqp_iter[at] = sqp_iter; o.qp_iter[at] = qp_iter; o.solver_time[at] = solver_time; }
}
// cost and acados' residual norms [stat, eq, ineq, comp] of the iterate a step leaves
template <class O>
MPC_HD void put_nlp(const O &o, size_t at, int lane, double cost, double r0, double r1, double r2, double r3)
{
    if (lane == 8) o.cost[at] = cost;
    if (lane >= 12 && lane < 16) o.residuals[at * 4 + (lane - 12)] = lane == 12 ? r0 : (lane == 13 ? r1 : (lane == 14 ? r2 : r3));
}
// The predicted trajectory of a controller step (orc_solver_get_iterate): x_0..x_N and u_0..u_{N-1} of the iterate, G1 records
// `ld` doubles apart, into rows sized for the batch's longest horizon NMAX; the rows beyond this simulation's own are NaN, so that
// nothing stale passes for a prediction.  `nt` lanes.
template <class G>
MPC_HD void put_prediction(const StepIO &io, int inst, int lane, int nt, G g1, size_t ld, int N, int NMAX)
{
    if (io.x_pred) {
        double *xp = io.x_pred + (size_t)inst * (NMAX + 1) * NX;
        for (int e = lane; e < (NMAX + 1) * NX; e += nt) {
            const int k = e / NX, i = e - k * NX;
            xp[e] = k <= N ? g1[(size_t)k * ld + O_X + i] : __builtin_nan("");
        }
    }
    if (io.u_pred) {
        double *up = io.u_pred + (size_t)inst * NMAX * NU;
        for (int e = lane; e < NMAX * NU; e += nt) {
            const int k = e / NU, j = e - k * NU;
            up[e] = k < N ? g1[(size_t)k * ld + O_U + j] : __builtin_nan("");
        }
    }
}

// ---- sensitivities of u0 on a step whose QP the bound-inactive fast path solved (mpcb_step_sens) -----------------------------------
// u0 is then affine in the feedback state and in the task reference: d u0 / d xhat = -K_0, and with M_1 = -B R~_0^-1 (12x6),
// M_{k+1} = (A - B K_k) M_k the reference row of stage k is (d u0 / d yref_k)' = -dt W G_k M_k (5x6), G_k = [GQ_k | e_5 GV_k'] the
// task Jacobian the QP was built from.  One stage of that recursion for lane (j, c), j < 6 joints x c < 6 inputs: Mt holds M_k
// TRANSPOSED (column c at Mt[12 c .. 12 c + 12)), K the gain rows K[12 j + i], G the [GQ 30 | GV 6] columns of the G2 record.
// A and B are diagonal blocks (shift_tail): row j of M is q_j, row 6 + j is qdot_j.
template <class KK, class MM>
MPC_HD void sens_advance(const InstParams &P, int j, int c, const KK &K, const MM &Mt, double &mq, double &mv)
{
    double t0 = 0.0, t1 = 0.0;
#pragma unroll
    for (int i = 0; i < NX; i += 2) { t0 += K[j * 12 + i] * Mt[c * 12 + i]; t1 += K[j * 12 + i + 1] * Mt[c * 12 + i + 1]; }
    const double t = t0 + t1, q = Mt[c * 12 + j], v = Mt[c * 12 + 6 + j];
    mq = q + P.a12[j] * v - P.b1[j] * t;
    mv = P.a22[j] * v - P.b2[j] * t;
}
// entry (i, c), i < NTASK, of (d u0 / d yref_k)'
template <class GG, class MM>
MPC_HD double sens_project(const InstParams &P, int i, int c, const GG &G, const MM &Mt)
{
    double s = 0.0, sv = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) { s += G[i * 6 + j] * Mt[c * 12 + j]; sv += G[30 + j] * Mt[c * 12 + 6 + j]; }
    return -P.dt * P.w_task[i] * (i == 4 ? s + sv : s);
}
// M_1 = -B R~_0^-1: rows j and 6 + j of column c from ri = R~_0^-1 (j, c)
MPC_HD void sens_start(const InstParams &P, int j, double ri, double &mq, double &mv) { mq = -P.b1[j] * ri; mv = -P.b2[j] * ri; }

// ---- sensitivity of u0 to the seven cost weights (mpcb_step_sens_w): w_u, w_qddot, the task weights of g1..g5 -----------------------
// The QP's matrices are affine in the weights, so d u0 / d weight_p = sum_k (d u0 / d g_k) (d/d weight_p of the stage gradient at the
// QP's solution).  M_k above is (d u0 / d gx_k)'; the input gradient reaches u0 through the feed-forward of its own stage,
// Nu_k = (d u0 / d gu_k)' = -K_k M_k (6x6; a perturbation of gu_k moves the backward vector p_k by -K_k' of it, and p_k acts as gx_k
// does), Nu_0 = -R~_0^-1.  With u+ = U_k + du_k, v+ the qdot half of X_k + dx_k and rho = r_k + G_k dx_k (unweighted) the stage
// gradient's derivatives are 2 dt u+ (u rows, w_u), dt cq^2 (u+ - v+) (u rows) and its negative (qdot rows, w_qddot), and
// dt G_i' rho_i (x rows, task weight i).  No weight is divided by: a weight of 0 has its derivative.
// sens_advance that also hands back nu = Nu_k[j][c] (the same arithmetic: M_{k+1} is bit for bit sens_advance's)
template <class KK, class MM>
MPC_HD void sensw_advance(const InstParams &P, int j, int c, const KK &K, const MM &Mt, double &mq, double &mv, double &nu)
{
    double t0 = 0.0, t1 = 0.0;
#pragma unroll
    for (int i = 0; i < NX; i += 2) { t0 += K[j * 12 + i] * Mt[c * 12 + i]; t1 += K[j * 12 + i + 1] * Mt[c * 12 + i + 1]; }
    const double t = t0 + t1, q = Mt[c * 12 + j], v = Mt[c * 12 + 6 + j];
    mq = q + P.a12[j] * v - P.b1[j] * t;
    mv = P.a22[j] * v - P.b2[j] * t;
    nu = -t;
}
// lane (j, c)'s addends of one stage to du0_dw[0][c] (w_u) and du0_dw[1][c] (w_qddot): nu = Nu_k[j][c], mv = M_k[6 + j][c] (0 at
// stage 0), up = u+_kj, vp = v+_kj
MPC_HD void sensw_input(const InstParams &P, int j, double nu, double mv, double up, double vp, double &a_u, double &a_qddot)
{
    a_u = nu * (2.0 * P.dt * up);
    a_qddot = (nu - mv) * (P.dt * P.cq[j] * P.cq[j] * (up - vp));
}
// (G_k M_k)[i][c], i < NTASK: the sum sens_project scales by -dt w_i
template <class GG, class MM>
MPC_HD double sensw_gm(int i, int c, const GG &G, const MM &Mt)
{
    double s = 0.0, sv = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) { s += G[i * 6 + j] * Mt[c * 12 + j]; sv += G[30 + j] * Mt[c * 12 + 6 + j]; }
    return i == 4 ? s + sv : s;
}
// rho_i = r_i + (G_k dx_k)_i, the linearised task residual at the QP's solution: r [5] unweighted, dq / dv [6] the halves of dx_k
template <class GG, class RR, class DQ, class DV>
MPC_HD double sensw_rho(int i, const GG &G, const RR &r, const DQ &dq, const DV &dv)
{
    double s = 0.0, sv = 0.0;
#pragma unroll
    for (int j = 0; j < 6; j++) { s += G[i * 6 + j] * dq[j]; sv += G[30 + j] * dv[j]; }
    return r[i] + (i == 4 ? s + sv : s);
}

// ---- joint-wise terminal cost (mpcb_step_term) -------------------------------------------------------------------------------------
// l_N(x) = 1/2 sum_j [q_j - q_e,j, v_j - v_e,j] [[pqq_j, pqv_j], [pqv_j, pvv_j]] [.]', not scaled by dt.  T: the simulation's record
// [pqq 6 | pqv 6 | pvv 6 | x_e 12] (mpc_layout.h NTERM), wavefront-uniform and read where it is used.  In the Gauss-Newton QP at the
// iterate: H_N = lm I + P, g_N = P (X_N - x_e); the cost and the stationarity rows of stage N take the same two functions.
constexpr int TM_QQ = 0, TM_QV = 6, TM_VV = 12, TM_XE = 18;
// rows q_j and qdot_j of P (x - x_e) at the terminal state's (q, v) of joint j
template <class T>
MPC_HD void term_grad(const T &t, int j, double q, double v, double &gq, double &gv)
{
    const double eq = q - t[TM_XE + j], ev = v - t[TM_XE + 6 + j];
    gq = t[TM_QQ + j] * eq + t[TM_QV + j] * ev;
    gv = t[TM_QV + j] * eq + t[TM_VV + j] * ev;
}
// joint j's term of l_N
template <class T>
MPC_HD double term_cost(const T &t, int j, double q, double v)
{
    const double eq = q - t[TM_XE + j], ev = v - t[TM_XE + 6 + j];
    return 0.5 * (eq * (t[TM_QQ + j] * eq + t[TM_QV + j] * ev) + ev * (t[TM_QV + j] * eq + t[TM_VV + j] * ev));
}
// entry (i, j), i <= j, of the 12x12 terminal weight P (states ordered [q; qdot]): six 2x2 blocks, zero elsewhere
template <class T>
MPC_HD double term_hess(const T &t, int i, int j)
{
    if (i == j) return i < 6 ? t[TM_QQ + i] : t[TM_VV + i - 6];
    return (i < 6 && j == i + 6) ? t[TM_QV + i] : 0.0;
}
// (d u0 / d x_e)(c, j) and (c, 6 + j) = -(M_N' P) there: g_N falls by P e_i when x_e,i grows.  mq = M_N[j][c], mv = M_N[6 + j][c]
template <class T>
MPC_HD void term_sens(const T &t, int j, double mq, double mv, double &dq, double &dv)
{
    dq = -(mq * t[TM_QQ + j] + mv * t[TM_QV + j]);
    dv = -(mq * t[TM_QV + j] + mv * t[TM_VV + j]);
}

}  // namespace nlp
}  // namespace mpcb
