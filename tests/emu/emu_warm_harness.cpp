// emu_warm_harness.cpp -- TEST-ONLY host emulation of the controller step with a per-simulation warm start (Engine::control_step<true>
// with StepIO::warm, mpcb_step_warm).
//
// Reuses emu_step_harness.cpp (the controller handle) unchanged and adds the entry point with the reference and the modes.  As
// mpcb_step_warm does, it runs the plain instantiation of the step when it is given no modes.  Compiled host-only, loaded only by
// the warm-start tests (tests/emu/emu_warm.py); not part of libmpcbatch.so.
#include "emu_step_harness.cpp"

namespace {

template <int NWV>
void emu_step_warm_t(EmuCtl &h, const StepIO &io, int reset)
{
    for (int inst = 0; inst < h.pb.batch; inst++) {
        HostExec<NWV> ex{h.sm.get(), h.pool.data()};
        load_constants(ex, &h.P[(size_t)inst], &h.rb);
        Ctx c{&h.pb, ws_carve(h.ws[(size_t)inst].data(), h.pb.N), h.pool_doubles, h.pb.N};
        Engine<HostExec<NWV>> eng(ex, c);
        eng.template control_step<true>(io, inst, reset != 0);
    }
}

}  // namespace

// One controller step of every instance from xhat [batch][12] against the task reference yref [batch][N][5] (null: the packed
// references), warm [batch] the WARM_* mode of each instance (null: every instance carries).  x_pred / u_pred may be null.
extern "C" int emu_step_warm(void *hv, const double *xhat, const double *yref, int ref_changed, const int *warm, int reset, double *u0,
                             int *status, int *sqp_iter, int *qp_iter, double *residuals, double *cost, double *solver_time,
                             double *x_pred, double *u_pred)
{
    EmuCtl &h = *static_cast<EmuCtl *>(hv);
    StepIO io{xhat, u0, status, sqp_iter, qp_iter, residuals, cost, solver_time, x_pred, u_pred};
    io.yref = yref;
    io.ref_changed = ref_changed != 0 ? 1 : 0;
    io.warm = warm;
    if (!warm) {
        if (h.waves == 8) emu_step_t<8>(h, io, reset);
        else if (h.waves == 4) emu_step_t<4>(h, io, reset);
        else if (h.waves == 2) emu_step_t<2>(h, io, reset);
        else if (h.waves == 1) emu_step_t<1>(h, io, reset);
        else return 1;
        return 0;
    }
    if (h.waves == 8) emu_step_warm_t<8>(h, io, reset);
    else if (h.waves == 4) emu_step_warm_t<4>(h, io, reset);
    else if (h.waves == 2) emu_step_warm_t<2>(h, io, reset);
    else if (h.waves == 1) emu_step_warm_t<1>(h, io, reset);
    else return 1;
    return 0;
}
