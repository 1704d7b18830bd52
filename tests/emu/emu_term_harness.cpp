// emu_term_harness.cpp -- TEST-ONLY host emulation of the controller step with the joint-wise terminal cost (mpcb_step_term): the
// engine with its TERM flag, Engine<HostExec, true>::control_step<true> (warm-start step) and control_step<true, true> (with the
// sensitivity pass, which then also forms d u0 / d x_e).
//
// Reuses emu_sens_harness.cpp (and through it the controller handle of emu_step_harness.cpp) unchanged.  As mpcb_step_term does, it
// runs the step of emu_step_sens when it is given no terminal cost.  Compiled host-only, loaded only by the terminal-cost tests
// (tests/emu/emu_term.py); not part of libmpcbatch.so.
#include "emu_sens_harness.cpp"

namespace {

template <int NWV, bool SENS>
void emu_step_term_t(EmuCtl &h, const StepIO &io, int reset)
{
    for (int inst = 0; inst < h.pb.batch; inst++) {
        HostExec<NWV> ex{h.sm.get(), h.pool.data()};
        load_constants(ex, &h.P[(size_t)inst], &h.rb);
        Ctx c{&h.pb, ws_carve(h.ws[(size_t)inst].data(), h.pb.N), h.pool_doubles, h.pb.N};
        Engine<HostExec<NWV>, true> eng(ex, c);
        eng.template control_step<true, SENS>(io, inst, reset != 0);
    }
}

template <bool SENS>
int emu_step_term_w(EmuCtl &h, const StepIO &io, int reset)
{
    if (h.waves == 8) emu_step_term_t<8, SENS>(h, io, reset);
    else if (h.waves == 4) emu_step_term_t<4, SENS>(h, io, reset);
    else if (h.waves == 2) emu_step_term_t<2, SENS>(h, io, reset);
    else if (h.waves == 1) emu_step_term_t<1, SENS>(h, io, reset);
    else return 1;
    return 0;
}

}  // namespace

// emu_step_sens with term [batch][NTERM] and du0_dxe [batch][6][12] (may be null); term == null: emu_step_sens.  The caller passes
// ref_changed != 0 with the step that follows a change of the terminal cost, as term_changed of mpcb_step_term does.
// Returns 2 on a full-SQP handle or for du0_dxe without du0_dx, as mpcb_step_term refuses them.
extern "C" int emu_step_term(void *hv, const double *xhat, const double *yref, int ref_changed, const int *warm, int reset, double *u0,
                             int *status, int *sqp_iter, int *qp_iter, double *residuals, double *cost, double *solver_time,
                             double *x_pred, double *u_pred, double *du0_dx, double *du0_dyref, int *valid, const double *term,
                             double *du0_dxe)
{
    if (!term)
        return du0_dxe ? 2 : emu_step_sens(hv, xhat, yref, ref_changed, warm, reset, u0, status, sqp_iter, qp_iter, residuals, cost,
                                           solver_time, x_pred, u_pred, du0_dx, du0_dyref, valid);
    EmuCtl &h = *static_cast<EmuCtl *>(hv);
    if (h.pb.solver_type != 1 || (du0_dx && !valid) || (du0_dxe && !du0_dx)) return 2;
    StepIO io{xhat, u0, status, sqp_iter, qp_iter, residuals, cost, solver_time, x_pred, u_pred};
    io.yref = yref;
    io.ref_changed = ref_changed != 0 ? 1 : 0;
    io.warm = warm;
    io.du0_dx = du0_dx;
    io.du0_dyref = du0_dyref;
    io.sens_valid = valid;
    io.term = term;
    io.du0_dxe = du0_dxe;
    return du0_dx ? emu_step_term_w<true>(h, io, reset) : emu_step_term_w<false>(h, io, reset);
}
