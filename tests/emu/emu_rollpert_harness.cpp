// emu_rollpert_harness.cpp -- TEST-ONLY host emulation of the rollout over a perturbed plant (Engine::rollout<true, true>, the device
// code behind mpcb_rollout_pert on the latency engine).
//
// Reuses emu_rollref_harness.cpp (the scheduled rollout, and through it the controller handle and emu_step_ref: the yardstick the
// perturbed rollout is defined by) unchanged and adds the rollout entry point with the perturbation arrays, and the plant step with an
// explicit bandwidth.  Compiled host-only, loaded only by tests/test_emulation_rollout_pert.py (tests/emu/emu_rollpert.py); not part
// of libmpcbatch.so.
#include "emu_rollref_harness.cpp"

namespace {

template <int NWV>
int emu_rollout_pert_t(const Problem *pb, const double *robot105, const double *params, Outputs out, const double *sched,
                       const PlantPert &pert, int step_chunk, int pool_doubles)
{
    Robot rb;
    std::memcpy(&rb, robot105, sizeof(Robot));
    std::vector<double> ws(ws_doubles_per_instance(pb->N));
    if (pool_doubles <= 0) pool_doubles = POOL_DEFAULT_DOUBLES;
    if (step_chunk <= 0) step_chunk = pb->Nsim;
    const size_t rows = (size_t)pb->Nsim + pb->N;
    for (int inst = 0; inst < pb->batch; inst++) {
        InstParams P;
        pack_inst_params(params + (size_t)inst * MPCB_NPARAM, &P);
        for (int s0 = 0; s0 < pb->Nsim; s0 += step_chunk) {
            // a launch starts from fresh shared memory: only the workspace carries
            Smem sm;
            std::memset(&sm, 0, sizeof sm);
            std::vector<double> pool((size_t)pool_doubles + 64, 0.0);
            HostExec<NWV> ex{&sm, pool.data()};
            load_constants(ex, &P, &rb);
            Ctx c{pb, ws_carve(ws.data(), pb->N), pool_doubles, pb->N};
            Engine<HostExec<NWV>> eng(ex, c);
            const int s1 = s0 + step_chunk < pb->Nsim ? s0 + step_chunk : pb->Nsim;
            eng.template rollout<true, true>(out, inst, s0, s1, sched + (size_t)inst * rows * NTASK, plant_pert_of(pert, inst, pb->Nsim));
        }
    }
    return 0;
}

}  // namespace

// emu_rollout_ref with the perturbation arrays wcv [batch][6], u_dist [batch][Nsim][6], x_noise [batch][Nsim][12] (each may be null)
extern "C" int emu_rollout_pert(const Problem *pb, const double *robot105, const double *params /* [batch][MPCB_NPARAM] */, double *z,
                                double *u, double *ee_pose, double *ee_rpy, double *ee_vel, int *status, int *sqp_iter, int *qp_iter,
                                double *residuals, double *cost, double *solver_time, double *errors, double *plant_time,
                                const double *sched, const double *wcv, const double *u_dist, const double *x_noise, int step_chunk,
                                int pool_doubles, int waves)
{
    Outputs out{z, u, ee_pose, ee_rpy, ee_vel, status, sqp_iter, qp_iter, residuals, cost, solver_time, errors, plant_time};
    const PlantPert pert{wcv, u_dist, x_noise};
    if (waves == 8) return emu_rollout_pert_t<8>(pb, robot105, params, out, sched, pert, step_chunk, pool_doubles);
    if (waves == 4) return emu_rollout_pert_t<4>(pb, robot105, params, out, sched, pert, step_chunk, pool_doubles);
    if (waves == 2) return emu_rollout_pert_t<2>(pb, robot105, params, out, sched, pert, step_chunk, pool_doubles);
    if (waves == 1) return emu_rollout_pert_t<1>(pb, robot105, params, out, sched, pert, step_chunk, pool_doubles);
    return 1;
}

// nlp::plant_rk with the bandwidths given, for one state: z [12], u [6], wcv [6] -> zn [12] (integrator and dt of `params`)
extern "C" void emu_plant_rk_wcv(const double *params, const double *wcv, const double *z, const double *u, double *zn)
{
    InstParams P;
    pack_inst_params(params, &P);
    for (int j = 0; j < 6; j++) nlp::plant_rk(P, wcv[j], z[j], z[6 + j], u[j], zn[j], zn[6 + j]);
}
