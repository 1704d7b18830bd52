// emu_sensw_harness.cpp -- TEST-ONLY host emulation of the controller step that also returns the sensitivity of u0 to the seven
// cost weights (Engine::control_step<true, true, true> with Engine::sens_pass<true>, mpcb_step_sens_w), and of the run-time weight
// update (mpcb_set_weights: mpc_layout.h put_weights on every simulation's parameter record).
//
// Reuses emu_sens_harness.cpp (and through it the controller handle of emu_step_harness.cpp) unchanged.  As mpcb_step_sens_w does,
// it runs the step of emu_step_sens when it is given nowhere to write du0_dw.  Compiled host-only, loaded only by the weight
// sensitivity tests (tests/emu/emu_sensw.py); not part of libmpcbatch.so.
#include "emu_sens_harness.cpp"

namespace {

template <int NWV>
void emu_step_sensw_t(EmuCtl &h, const StepIO &io, int reset)
{
    for (int inst = 0; inst < h.pb.batch; inst++) {
        HostExec<NWV> ex{h.sm.get(), h.pool.data()};
        load_constants(ex, &h.P[(size_t)inst], &h.rb);
        Ctx c{&h.pb, ws_carve(h.ws[(size_t)inst].data(), h.pb.N), h.pool_doubles, h.pb.N};
        Engine<HostExec<NWV>> eng(ex, c);
        eng.template control_step<true, true, true>(io, inst, reset != 0);
    }
}

}  // namespace

// weights [batch][NWEIGHT]: what the kernel of mpcb_set_weights does to the device records.  The caller passes ref_changed != 0 to
// the next step, as the handle of mpcb_set_weights does by itself.
extern "C" void emu_set_weights(void *hv, const double *weights)
{
    EmuCtl &h = *static_cast<EmuCtl *>(hv);
    for (int i = 0; i < h.pb.batch; i++) put_weights(h.P[(size_t)i], weights + (size_t)i * NWEIGHT);
}

// emu_step_sens with du0_dw [batch][NWEIGHT][6]; du0_dw == null: emu_step_sens.
extern "C" int emu_step_sensw(void *hv, const double *xhat, const double *yref, int ref_changed, const int *warm, int reset, double *u0,
                              int *status, int *sqp_iter, int *qp_iter, double *residuals, double *cost, double *solver_time,
                              double *x_pred, double *u_pred, double *du0_dx, double *du0_dyref, int *valid, double *du0_dw)
{
    if (!du0_dw)
        return emu_step_sens(hv, xhat, yref, ref_changed, warm, reset, u0, status, sqp_iter, qp_iter, residuals, cost, solver_time, x_pred,
                             u_pred, du0_dx, du0_dyref, valid);
    EmuCtl &h = *static_cast<EmuCtl *>(hv);
    if (h.pb.solver_type != 1 || !du0_dx || !valid) return 2;
    StepIO io{xhat, u0, status, sqp_iter, qp_iter, residuals, cost, solver_time, x_pred, u_pred};
    io.yref = yref;
    io.ref_changed = ref_changed != 0 ? 1 : 0;
    io.warm = warm;
    io.du0_dx = du0_dx;
    io.du0_dyref = du0_dyref;
    io.sens_valid = valid;
    io.du0_dw = du0_dw;
    if (h.waves == 8) emu_step_sensw_t<8>(h, io, reset);
    else if (h.waves == 4) emu_step_sensw_t<4>(h, io, reset);
    else if (h.waves == 2) emu_step_sensw_t<2>(h, io, reset);
    else if (h.waves == 1) emu_step_sensw_t<1>(h, io, reset);
    else return 1;
    return 0;
}
