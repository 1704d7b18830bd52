// emu_combined_harness.cpp -- TEST-ONLY host emulation of the combined controller step and rollout (mpcb_step_combined,
// mpcb_rollout_combined on the latency engine): Engine<HostExec, 1, 1, 1>::control_step<true> and Engine<HostExec, TERM_TABLE,
// DIST_SHARED, 1>::rollout<true, true, true, true>, the same engine code the device kernels instantiate.
//
// Reuses emu_rollpert_harness.cpp (and through it the controller handle of emu_step_harness.cpp) unchanged.  Every table is given:
// the caller fills neutral data for a feature that is off, as the library's host layer does.  Compiled host-only, loaded only by the
// combined tests (tests/emu/emu_combined.py); not part of libmpcbatch.so.
#include "emu_rollpert_harness.cpp"

namespace {

template <int NWV>
void emu_step_combined_t(EmuCtl &h, const StepIO &io, int reset)
{
    for (int inst = 0; inst < h.pb.batch; inst++) {
        HostExec<NWV> ex{h.sm.get(), h.pool.data()};
        load_constants(ex, &h.P[(size_t)inst], &h.rb);
        Ctx c{&h.pb, ws_carve(h.ws[(size_t)inst].data(), h.pb.N), h.pool_doubles, h.pb.N};
        Engine<HostExec<NWV>, 1, 1, 1> eng(ex, c);
        eng.template control_step<true>(io, inst, reset != 0);
    }
}

template <int NWV>
int emu_rollout_combined_t(const Problem *pb, const double *robot105, const double *params, Outputs out, const double *sched,
                           const PlantPert &pert, const TermTab &term, const ObsArg &obs, const double *surf, const int *warm,
                           const int *bounds, int nbounds, int pool_doubles)
{
    Robot rb;
    std::memcpy(&rb, robot105, sizeof(Robot));
    std::vector<double> ws(ws_doubles_per_instance(pb->N));
    if (pool_doubles <= 0) pool_doubles = POOL_DEFAULT_DOUBLES;
    const size_t rows = (size_t)pb->Nsim + pb->N;
    for (int inst = 0; inst < pb->batch; inst++) {
        InstParams P;
        pack_inst_params(params + (size_t)inst * MPCB_NPARAM, &P);
        for (int b = 0; b + 1 < nbounds; b++) {
            // a launch starts from fresh shared memory: only the workspace carries (the observer's estimate in w.state[ST_OBS])
            Smem sm;
            std::memset(&sm, 0, sizeof sm);
            std::vector<double> pool((size_t)pool_doubles + 64, 0.0);
            HostExec<NWV> ex{&sm, pool.data()};
            load_constants(ex, &P, &rb);
            Ctx c{pb, ws_carve(ws.data(), pb->N), pool_doubles, pb->N};
            Engine<HostExec<NWV>, TERM_TABLE, DIST_SHARED, 1> eng(ex, c);
            eng.template rollout<true, true, true, true>(out, inst, bounds[b], bounds[b + 1], sched + (size_t)inst * rows * NTASK,
                                                         plant_pert_of(pert, inst, pb->Nsim), term_tab_of(term, inst, pb->Nsim),
                                                         obs_arg_of(obs, inst, pb->Nsim), surf + (size_t)inst * rows * NSURF, warm[inst]);
        }
    }
    return 0;
}

}  // namespace

// One combined controller step: term [batch][30], dist [batch][6], surf [batch][N][6] (none null), warm [batch] or null (carry).
// Returns 2 on a full-SQP handle or with a null table.
extern "C" int emu_step_combined(void *hv, const double *xhat, const double *yref, int ref_changed, const int *warm, int reset, double *u0,
                                 int *status, int *sqp_iter, int *qp_iter, double *residuals, double *cost, double *solver_time,
                                 double *x_pred, double *u_pred, const double *term, const double *dist, const double *surf)
{
    EmuCtl &h = *static_cast<EmuCtl *>(hv);
    if (h.pb.solver_type != 1 || !term || !dist || !surf) return 2;
    StepIO io{xhat, u0, status, sqp_iter, qp_iter, residuals, cost, solver_time, x_pred, u_pred};
    io.yref = yref;
    io.ref_changed = ref_changed != 0 ? 1 : 0;
    io.warm = warm;
    io.term = term;
    io.dist = dist;
    io.surf = surf;
    if (h.waves == 8) emu_step_combined_t<8>(h, io, reset);
    else if (h.waves == 4) emu_step_combined_t<4>(h, io, reset);
    else if (h.waves == 2) emu_step_combined_t<2>(h, io, reset);
    else if (h.waves == 1) emu_step_combined_t<1>(h, io, reset);
    else return 1;
    return 0;
}

// The combined rollout, one "launch" per interval of bounds [nbounds] (bounds[0] = 0, ascending, last = Nsim); every table given
// (returns 2 otherwise, and on a full-SQP problem)
extern "C" int emu_rollout_combined(const Problem *pb, const double *robot105, const double *params /* [batch][MPCB_NPARAM] */, double *z,
                                    double *u, double *ee_pose, double *ee_rpy, double *ee_vel, int *status, int *sqp_iter, int *qp_iter,
                                    double *residuals, double *cost, double *solver_time, double *errors, double *plant_time,
                                    const double *sched, const double *wcv, const double *u_dist, const double *x_noise,
                                    const double *blocks, const double *x_ref, const double *gain, double *d_hat, const double *surf,
                                    const int *warm, const int *bounds, int nbounds, int pool_doubles, int waves)
{
    if (!blocks || !x_ref || !gain || !d_hat || !surf || !warm || !bounds || nbounds < 2 || pb->solver_type != 1) return 2;
    Outputs out{z, u, ee_pose, ee_rpy, ee_vel, status, sqp_iter, qp_iter, residuals, cost, solver_time, errors, plant_time};
    const PlantPert pert{wcv, u_dist, x_noise};
    const TermTab term{blocks, x_ref};
    const ObsArg obs{gain, d_hat};
    if (waves == 8) return emu_rollout_combined_t<8>(pb, robot105, params, out, sched, pert, term, obs, surf, warm, bounds, nbounds, pool_doubles);
    if (waves == 4) return emu_rollout_combined_t<4>(pb, robot105, params, out, sched, pert, term, obs, surf, warm, bounds, nbounds, pool_doubles);
    if (waves == 2) return emu_rollout_combined_t<2>(pb, robot105, params, out, sched, pert, term, obs, surf, warm, bounds, nbounds, pool_doubles);
    if (waves == 1) return emu_rollout_combined_t<1>(pb, robot105, params, out, sched, pert, term, obs, surf, warm, bounds, nbounds, pool_doubles);
    return 1;
}
