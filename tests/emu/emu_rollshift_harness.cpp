// emu_rollshift_harness.cpp -- TEST-ONLY host emulation of the rollout with the shift warm start (Engine<HostExec, 0, 0,
// SURF>::rollout<true, true, false, true>, the device code behind mpcb_rollout_warm on the latency engine).
//
// Reuses emu_rollsurf_harness.cpp (and through it the perturbed rollout and its plant step) unchanged and adds the rollout entry
// point with the per-simulation modes, without and with a surface table.  The yardsticks, the emulated steps with a warm-start mode,
// live in emu_warm_harness.cpp and emu_surf_harness.cpp (tests/emu/emu_warm.py, emu_surf.py).  Compiled host-only, loaded only by
// tests/test_emulation_rollout_shift.py (tests/emu/emu_rollshift.py); not part of libmpcbatch.so.
#include "emu_rollsurf_harness.cpp"

namespace {

template <int NWV, int SURF>
int emu_rollout_shift_t(const Problem *pb, const double *robot105, const double *params, Outputs out, const double *sched,
                        const PlantPert &pert, const double *surf, const int *warm, int step_chunk, int pool_doubles)
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
            Engine<HostExec<NWV>, 0, 0, SURF> eng(ex, c);
            const int s1 = s0 + step_chunk < pb->Nsim ? s0 + step_chunk : pb->Nsim;
            if constexpr (SURF != 0)
                eng.template rollout<true, true, false, true>(out, inst, s0, s1, sched + (size_t)inst * rows * NTASK,
                                                              plant_pert_of(pert, inst, pb->Nsim), {}, {}, surf + (size_t)inst * rows * NSURF,
                                                              warm[inst]);
            else
                eng.template rollout<true, true, false, true>(out, inst, s0, s1, sched + (size_t)inst * rows * NTASK,
                                                              plant_pert_of(pert, inst, pb->Nsim), {}, {}, {}, warm[inst]);
        }
    }
    return 0;
}

template <int SURF>
int emu_rollout_shift_w(int waves, const Problem *pb, const double *robot105, const double *params, Outputs out, const double *sched,
                        const PlantPert &pert, const double *surf, const int *warm, int step_chunk, int pool_doubles)
{
    if (waves == 8) return emu_rollout_shift_t<8, SURF>(pb, robot105, params, out, sched, pert, surf, warm, step_chunk, pool_doubles);
    if (waves == 4) return emu_rollout_shift_t<4, SURF>(pb, robot105, params, out, sched, pert, surf, warm, step_chunk, pool_doubles);
    if (waves == 2) return emu_rollout_shift_t<2, SURF>(pb, robot105, params, out, sched, pert, surf, warm, step_chunk, pool_doubles);
    if (waves == 1) return emu_rollout_shift_t<1, SURF>(pb, robot105, params, out, sched, pert, surf, warm, step_chunk, pool_doubles);
    return 1;
}

}  // namespace

// emu_rollout_pert (surf == NULL) or emu_rollout_surf with the warm-start modes warm [batch] (not null; returns 2 otherwise, and on a
// full-SQP problem, as mpcb_rollout_warm refuses it)
extern "C" int emu_rollout_shift(const Problem *pb, const double *robot105, const double *params /* [batch][MPCB_NPARAM] */, double *z,
                                 double *u, double *ee_pose, double *ee_rpy, double *ee_vel, int *status, int *sqp_iter, int *qp_iter,
                                 double *residuals, double *cost, double *solver_time, double *errors, double *plant_time,
                                 const double *sched, const double *wcv, const double *u_dist, const double *x_noise,
                                 const double *surf, const int *warm, int step_chunk, int pool_doubles, int waves)
{
    if (!warm || pb->solver_type != 1) return 2;
    Outputs out{z, u, ee_pose, ee_rpy, ee_vel, status, sqp_iter, qp_iter, residuals, cost, solver_time, errors, plant_time};
    const PlantPert pert{wcv, u_dist, x_noise};
    if (surf) return emu_rollout_shift_w<1>(waves, pb, robot105, params, out, sched, pert, surf, warm, step_chunk, pool_doubles);
    return emu_rollout_shift_w<0>(waves, pb, robot105, params, out, sched, pert, surf, warm, step_chunk, pool_doubles);
}
