// emu_surf_harness.cpp -- TEST-ONLY host emulation of the controller step over a scheduled, stage-varying surface (mpcb_step_surf):
// the engine with its SURF flag, Engine<HostExec, 0, 0, 1>::control_step<true> (warm-start step).
//
// Reuses emu_warm_harness.cpp (and through it the controller handle of emu_step_harness.cpp) unchanged.  As mpcb_step_surf does, it
// runs the step of emu_step_warm when it is given no window.  Compiled host-only, loaded only by the surface tests
// (tests/emu/emu_surf.py); not part of libmpcbatch.so.
#include "emu_warm_harness.cpp"

namespace {

template <int NWV>
void emu_step_surf_t(EmuCtl &h, const StepIO &io, int reset)
{
    for (int inst = 0; inst < h.pb.batch; inst++) {
        HostExec<NWV> ex{h.sm.get(), h.pool.data()};
        load_constants(ex, &h.P[(size_t)inst], &h.rb);
        Ctx c{&h.pb, ws_carve(h.ws[(size_t)inst].data(), h.pb.N), h.pool_doubles, h.pb.N};
        Engine<HostExec<NWV>, 0, 0, 1> eng(ex, c);
        eng.template control_step<true>(io, inst, reset != 0);
    }
}

}  // namespace

// emu_step_warm with surf [batch][N][6]; surf == null: emu_step_warm.  The caller passes ref_changed != 0 with the step that follows
// a change of the window, as surf_changed of mpcb_step_surf does.  Returns 2 on a full-SQP handle, as mpcb_step_surf refuses it.
extern "C" int emu_step_surf(void *hv, const double *xhat, const double *yref, int ref_changed, const int *warm, int reset, double *u0,
                             int *status, int *sqp_iter, int *qp_iter, double *residuals, double *cost, double *solver_time,
                             double *x_pred, double *u_pred, const double *surf)
{
    if (!surf)
        return emu_step_warm(hv, xhat, yref, ref_changed, warm, reset, u0, status, sqp_iter, qp_iter, residuals, cost, solver_time, x_pred,
                             u_pred);
    EmuCtl &h = *static_cast<EmuCtl *>(hv);
    if (h.pb.solver_type != 1) return 2;
    StepIO io{xhat, u0, status, sqp_iter, qp_iter, residuals, cost, solver_time, x_pred, u_pred};
    io.yref = yref;
    io.ref_changed = ref_changed != 0 ? 1 : 0;
    io.warm = warm;
    io.surf = surf;
    if (h.waves == 8) emu_step_surf_t<8>(h, io, reset);
    else if (h.waves == 4) emu_step_surf_t<4>(h, io, reset);
    else if (h.waves == 2) emu_step_surf_t<2>(h, io, reset);
    else if (h.waves == 1) emu_step_surf_t<1>(h, io, reset);
    else return 1;
    return 0;
}
