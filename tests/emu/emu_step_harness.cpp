// emu_step_harness.cpp -- TEST-ONLY host emulation of the controller step (Engine::control_step, mpcb_step).
//
// Reuses emu_harness.cpp (HostExec, emu_run, emu_paths) unchanged and adds a handle that keeps every instance's workspace
// between calls, as the device does between mpcb_step launches: emu_ctl_create / emu_step / emu_ctl_destroy.  Compiled
// host-only, loaded only by tests/test_emulation_step.py (tests/emu/emu_step.py); not part of libmpcbatch.so.
#include "emu_harness.cpp"

#include <memory>

namespace {

struct EmuCtl {
    Problem pb;
    Robot rb;
    std::vector<InstParams> P;
    std::vector<std::vector<double>> ws;   // one workspace per instance (mpc_layout.h ws_carve)
    std::unique_ptr<Smem> sm;              // the LDS working set, reused across instances and calls like emu_run's
    std::vector<double> pool;
    int pool_doubles, waves;
};

template <int NWV>
void emu_step_t(EmuCtl &h, const StepIO &io, int reset)
{
    for (int inst = 0; inst < h.pb.batch; inst++) {
        HostExec<NWV> ex{h.sm.get(), h.pool.data()};
        load_constants(ex, &h.P[(size_t)inst], &h.rb);
        Ctx c{&h.pb, ws_carve(h.ws[(size_t)inst].data(), h.pb.N), h.pool_doubles, h.pb.N};
        Engine<HostExec<NWV>> eng(ex, c);
        eng.control_step(io, inst, reset != 0);
    }
}

}  // namespace

extern "C" void *emu_ctl_create(const Problem *pb, const double *robot105, const double *params /* [batch][MPCB_NPARAM] */,
                                int pool_doubles, int waves)
{
    auto *h = new EmuCtl;
    h->pb = *pb;
    std::memcpy(&h->rb, robot105, sizeof(Robot));
    h->P.resize((size_t)pb->batch);
    for (int i = 0; i < pb->batch; i++) pack_inst_params(params + (size_t)i * MPCB_NPARAM, &h->P[(size_t)i]);
    h->ws.assign((size_t)pb->batch, std::vector<double>(ws_doubles_per_instance(pb->N), 0.0));
    h->sm.reset(new Smem);
    std::memset(h->sm.get(), 0, sizeof(Smem));
    h->pool_doubles = pool_doubles > 0 ? pool_doubles : POOL_DEFAULT_DOUBLES;
    h->pool.assign((size_t)h->pool_doubles + 64, 0.0);
    h->waves = waves;
    return h;
}

extern "C" void emu_ctl_destroy(void *h) { delete static_cast<EmuCtl *>(h); }

// One controller step of every instance from xhat [batch][12]; x_pred / u_pred may be null.
extern "C" int emu_step(void *hv, const double *xhat, int reset, double *u0, int *status, int *sqp_iter, int *qp_iter,
                        double *residuals, double *cost, double *solver_time, double *x_pred, double *u_pred)
{
    EmuCtl &h = *static_cast<EmuCtl *>(hv);
    const StepIO io{xhat, u0, status, sqp_iter, qp_iter, residuals, cost, solver_time, x_pred, u_pred};
    if (h.waves == 8) emu_step_t<8>(h, io, reset);
    else if (h.waves == 4) emu_step_t<4>(h, io, reset);
    else if (h.waves == 2) emu_step_t<2>(h, io, reset);
    else if (h.waves == 1) emu_step_t<1>(h, io, reset);
    else return 1;
    return 0;
}
