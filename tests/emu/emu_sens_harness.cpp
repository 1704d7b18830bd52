// emu_sens_harness.cpp -- TEST-ONLY host emulation of the controller step that also returns the feedback gain and the reference
// sensitivity of u0 (Engine::control_step<true, true> with Engine::sens_pass, mpcb_step_sens).
//
// Reuses emu_warm_harness.cpp (and through it the controller handle of emu_step_harness.cpp) unchanged and adds the entry point
// with the three output arrays.  As mpcb_step_sens does, it runs the step of emu_step_warm when it is given nowhere to write them.
// Compiled host-only, loaded only by the sensitivity tests (tests/emu/emu_sens.py); not part of libmpcbatch.so.
#include "emu_warm_harness.cpp"

namespace {

template <int NWV>
void emu_step_sens_t(EmuCtl &h, const StepIO &io, int reset)
{
    for (int inst = 0; inst < h.pb.batch; inst++) {
        HostExec<NWV> ex{h.sm.get(), h.pool.data()};
        load_constants(ex, &h.P[(size_t)inst], &h.rb);
        Ctx c{&h.pb, ws_carve(h.ws[(size_t)inst].data(), h.pb.N), h.pool_doubles, h.pb.N};
        Engine<HostExec<NWV>> eng(ex, c);
        eng.template control_step<true, true>(io, inst, reset != 0);
    }
}

}  // namespace

// emu_step_warm with du0_dx [batch][6][12], du0_dyref [batch][N][5][6] (may be null) and valid [batch]; du0_dx == null: emu_step_warm.
// Returns 2 on a full-SQP handle, as mpcb_step_sens refuses one.
extern "C" int emu_step_sens(void *hv, const double *xhat, const double *yref, int ref_changed, const int *warm, int reset, double *u0,
                             int *status, int *sqp_iter, int *qp_iter, double *residuals, double *cost, double *solver_time,
                             double *x_pred, double *u_pred, double *du0_dx, double *du0_dyref, int *valid)
{
    if (!du0_dx)
        return emu_step_warm(hv, xhat, yref, ref_changed, warm, reset, u0, status, sqp_iter, qp_iter, residuals, cost, solver_time, x_pred,
                             u_pred);
    EmuCtl &h = *static_cast<EmuCtl *>(hv);
    if (h.pb.solver_type != 1 || !valid) return 2;
    StepIO io{xhat, u0, status, sqp_iter, qp_iter, residuals, cost, solver_time, x_pred, u_pred};
    io.yref = yref;
    io.ref_changed = ref_changed != 0 ? 1 : 0;
    io.warm = warm;
    io.du0_dx = du0_dx;
    io.du0_dyref = du0_dyref;
    io.sens_valid = valid;
    if (h.waves == 8) emu_step_sens_t<8>(h, io, reset);
    else if (h.waves == 4) emu_step_sens_t<4>(h, io, reset);
    else if (h.waves == 2) emu_step_sens_t<2>(h, io, reset);
    else if (h.waves == 1) emu_step_sens_t<1>(h, io, reset);
    else return 1;
    return 0;
}
