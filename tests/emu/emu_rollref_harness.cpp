// emu_rollref_harness.cpp -- TEST-ONLY host emulation of the rollout against a task reference schedule (Engine::rollout<true>, the
// device code behind mpcb_rollout_ref on the latency engine).
//
// Reuses emu_ref_harness.cpp (the controller handle and emu_step_ref: the yardstick the scheduled rollout is defined by) unchanged and
// adds the rollout entry point with the schedule.  Compiled host-only, loaded only by tests/test_emulation_rollout_ref.py
// (tests/emu/emu_rollref.py); not part of libmpcbatch.so.
#include "emu_ref_harness.cpp"

namespace {

template <int NWV>
int emu_rollout_ref_t(const Problem *pb, const double *robot105, const double *params, Outputs out, const double *sched, int step_chunk,
                      int pool_doubles)
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
        Smem sm;
        std::memset(&sm, 0, sizeof sm);
        std::vector<double> pool((size_t)pool_doubles + 64, 0.0);
        HostExec<NWV> ex{&sm, pool.data()};
        for (int s0 = 0; s0 < pb->Nsim; s0 += step_chunk) {
            load_constants(ex, &P, &rb);
            Ctx c{pb, ws_carve(ws.data(), pb->N), pool_doubles, pb->N};
            Engine<HostExec<NWV>> eng(ex, c);
            const int s1 = s0 + step_chunk < pb->Nsim ? s0 + step_chunk : pb->Nsim;
            eng.template rollout<true>(out, inst, s0, s1, sched + (size_t)inst * rows * NTASK);
        }
    }
    return 0;
}

}  // namespace

// emu_run with the schedule sched [batch][Nsim + N][5]
extern "C" int emu_rollout_ref(const Problem *pb, const double *robot105, const double *params /* [batch][MPCB_NPARAM] */, double *z,
                               double *u, double *ee_pose, double *ee_rpy, double *ee_vel, int *status, int *sqp_iter, int *qp_iter,
                               double *residuals, double *cost, double *solver_time, double *errors, double *plant_time,
                               const double *sched, int step_chunk, int pool_doubles, int waves)
{
    Outputs out{z, u, ee_pose, ee_rpy, ee_vel, status, sqp_iter, qp_iter, residuals, cost, solver_time, errors, plant_time};
    if (waves == 8) return emu_rollout_ref_t<8>(pb, robot105, params, out, sched, step_chunk, pool_doubles);
    if (waves == 4) return emu_rollout_ref_t<4>(pb, robot105, params, out, sched, step_chunk, pool_doubles);
    if (waves == 2) return emu_rollout_ref_t<2>(pb, robot105, params, out, sched, step_chunk, pool_doubles);
    if (waves == 1) return emu_rollout_ref_t<1>(pb, robot105, params, out, sched, step_chunk, pool_doubles);
    return 1;
}

// nlp::plant_rk, the plant step built into the rollout, for one state: z [12], u [6] -> zn [12] (parameter record `params`)
extern "C" void emu_plant_rk(const double *params, const double *z, const double *u, double *zn)
{
    InstParams P;
    pack_inst_params(params, &P);
    for (int j = 0; j < 6; j++) nlp::plant_rk(P, j, z[j], z[6 + j], u[j], zn[j], zn[6 + j]);
}
