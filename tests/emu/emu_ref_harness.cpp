// emu_ref_harness.cpp -- TEST-ONLY host emulation of the controller step against a task reference (Engine::control_step with
// StepIO::yref / ref_changed, mpcb_step_ref).
//
// Reuses emu_step_harness.cpp (the controller handle, emu_step_t) unchanged and adds the entry point with the reference.  Compiled
// host-only, loaded only by the reference tests (tests/emu/emu_ref.py); not part of libmpcbatch.so.
#include "emu_step_harness.cpp"

// One controller step of every instance from xhat [batch][12] against the task reference yref [batch][N][5] (null: the packed
// references); ref_changed != 0: the reference differs from the previous step's.  x_pred / u_pred may be null.
extern "C" int emu_step_ref(void *hv, const double *xhat, const double *yref, int ref_changed, int reset, double *u0, int *status,
                            int *sqp_iter, int *qp_iter, double *residuals, double *cost, double *solver_time, double *x_pred,
                            double *u_pred)
{
    EmuCtl &h = *static_cast<EmuCtl *>(hv);
    StepIO io{xhat, u0, status, sqp_iter, qp_iter, residuals, cost, solver_time, x_pred, u_pred};
    io.yref = yref;
    io.ref_changed = ref_changed != 0 ? 1 : 0;
    if (h.waves == 8) emu_step_t<8>(h, io, reset);
    else if (h.waves == 4) emu_step_t<4>(h, io, reset);
    else if (h.waves == 2) emu_step_t<2>(h, io, reset);
    else if (h.waves == 1) emu_step_t<1>(h, io, reset);
    else return 1;
    return 0;
}
