"""The oracle and the emulated latency engine against a reference that shares nothing with them (tests/dense_qp.py): the stage
residual and its Jacobian from a homogeneous-transform chain differentiated by complex step, and one Gauss-Newton QP solved
through a pivoted sparse LU of its whole KKT system, with an exact active-set certificate where bounds are active.

ORACLE_VS_DENSE is the committed record of how far the ORACLE's solution of every case lies from the dense one (and of the
dense solve's own LU-vs-refined conditioning estimate).  The bound of every engine-vs-dense comparison, here and in
tests/test_gpu_dense_qp.py, is derived from it: 10 x the case's distance (a different but equally valid order of fp64
operations), floor 1e-12 (the oracle may land within an ulp by luck).  A case whose bound would exceed 1e-9, the project's parity
bar, says nothing and is replaced (tests/dense_qp_cases.py); tests/tools/dense_qp_profile.py writes the table to
profiles/dense_qp_distances.txt.
"""
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)

import dense_qp as dq  # noqa: E402
import dense_qp_cases as dc  # noqa: E402

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

# case id -> (max |oracle - dense| over dX, dU; max |plain LU - refined| of the dense solve), measured on the CPU
ORACLE_VS_DENSE = {
    "N1-rand": (1.11e-16, 1.1e-16),
    "N1-rand-ipm": (2.75e-12, 1.1e-16),
    "N2-rand": (2.22e-16, 1.1e-16),
    "N2-rand-ipm": (2.37e-13, 1.1e-16),
    "N3-rand": (2.22e-16, 1.7e-16),
    "N3-rand-ipm": (5.45e-14, 1.7e-16),
    "N7-rand": (1.33e-15, 6.1e-16),
    "N7-rand-ipm": (4.02e-16, 6.1e-16),
    "N20-rand": (8.10e-15, 5.3e-15),
    "N20-rand-ipm": (5.96e-12, 5.3e-15),
    "N25-rand": (1.22e-15, 6.9e-16),
    "N26-rand": (3.89e-16, 5.6e-16),
    "N26-rand-ipm": (1.75e-15, 5.6e-16),
    "N37-rand": (1.83e-15, 1.7e-15),
    "N38-rand": (6.64e-14, 2.8e-14),
    "N38-rand-ipm": (6.39e-11, 2.8e-14),
    "N42-rand": (2.00e-15, 8.3e-16),
    "N43-rand": (9.96e-16, 1.5e-15),
    "N43-rand-ipm": (5.10e-12, 1.5e-15),
    "N50-rand": (1.33e-15, 8.9e-16),
    "N79-rand": (2.89e-15, 1.3e-15),
    "N80-rand": (2.55e-15, 7.9e-15),
    "N100-rand": (6.11e-15, 5.4e-14),
    "N100-rand-ipm": (1.40e-14, 5.4e-14),
    "N125-rand": (9.39e-14, 4.8e-14),
    "N126-rand": (3.94e-15, 6.1e-16),
    "N126-rand-ipm": (3.77e-15, 6.1e-16),
    "N130-rand": (3.92e-14, 1.6e-14),
    "N130-rand-ipm": (5.04e-13, 1.6e-14),
    "N135-rand": (3.50e-15, 3.4e-15),
    "N136-rand": (2.08e-13, 6.7e-14),
    "N136-rand-ipm": (1.20e-13, 6.7e-14),
    "N140-rand": (1.07e-13, 1.8e-14),
    "N141-rand": (9.19e-14, 1.1e-13),
    "N141-rand-ipm": (7.66e-12, 1.1e-13),
    "N200-rand": (5.16e-15, 6.2e-15),
    "N200-rand-ipm": (6.76e-14, 6.2e-15),
    "N245-rand": (3.54e-12, 1.4e-13),
    "N246-rand": (5.59e-13, 1.0e-13),
    "N246-rand-ipm": (8.73e-14, 1.0e-13),
    "N300-rand": (8.27e-15, 2.3e-14),
    "N20-tight": (6.51e-12, 1.9e-15),
    "N20-tight-ipm": (6.51e-12, 1.9e-15),
    "N130-tight": (2.94e-14, 3.9e-14),
    "N130-tight-ipm": (2.94e-14, 3.9e-14),
    "N20-default": (4.00e-11, 4.9e-15),
    "N20-default-ipm": (4.00e-11, 4.9e-15),
    "N20-ur5": (1.02e-14, 2.2e-15),
    "N20-tool": (2.23e-14, 5.8e-15),
    "N20-ramp": (1.35e-14, 3.6e-15),
    "N20-lm": (1.78e-14, 5.7e-15),
    "N100-lm-ipm": (4.86e-12, 1.6e-14),
}
N_CASES = 52
SEPARATION = dict(active_within=1e-6, free_slack=1e-5)
# max |dense - oracle| over the stage residual r [17] and its Jacobian Jr [17, 18], 200 random draws per robot, pinned at 10 x
# the measured: the task rows (FK chain, complex step) r 1.3e-15, Jr 1.1e-15; the input / acceleration rows r 8.5e-13,
# Jr 2.3e-13 -- these divide by dt = 5e-4 (|qdot| eps / dt = 6.7e-13 per operation, entries (a22 - 1) / dt up to 2000);
# the weighted stage Hessian relative to its largest entry 3.2e-15
ASSEMBLY_TOL = dict(r_task=1.4e-14, J_task=1.2e-14, r_lin=8.6e-12, J_lin=2.3e-12, H_rel=3.3e-14)

CASES = dc.all_cases()
BY_ID = {c["id"]: c for c in CASES}


def test_case_list_is_complete():
    """A silently dropped parametrisation fails: the number of cases, their table entries and what the issue lists."""
    assert len(CASES) == N_CASES and sorted(ORACLE_VS_DENSE) == sorted(BY_ID)
    for N in (1, 2, 3, 7, 20, 50, 79, 80, 100, 130, 200, 245, 246, 300):
        assert f"N{N}-rand" in BY_ID
    for cid in ("N20-tight", "N20-tight-ipm", "N130-tight", "N130-tight-ipm", "N20-default", "N20-default-ipm", "N20-ur5",
                "N20-tool", "N20-ramp", "N20-lm"):
        assert cid in BY_ID
    assert max(dc.tolerance(ORACLE_VS_DENSE, cid) for cid in BY_ID) <= 1e-9
    dts = {c["cfg"]["dt"] for c in CASES}
    assert {5e-4, 2e-3, 0.01, 0.02} <= dts
    assert max(float((c["cfg"]["wcv"] * c["cfg"]["dt"]).max()) for c in CASES) > 2.3
    for c in CASES:
        X, _ = dc.guess(c)
        assert np.abs(c["xhat"] - X[0]).min() > 0          # dx0 != 0 in every component


def test_dense_module_is_independent_of_the_oracle_and_the_engine_sources():
    src = open(os.path.join(HERE, "dense_qp.py")).read()
    for word in ("import oracle", "from oracle", "orc.", "robotic_mpc_amd", "helpers", "reference_checks"):
        assert word not in src.split('"""', 2)[2], word


def _random_stage(rng, robot):
    from robotic_mpc_amd import config, robots

    coeffs = {k: float(v) for k, v in zip("abcdef", rng.normal([-0.1, 0.1, -0.01, 0.01, 0.01, 0.0], 0.05))}
    dt = [5e-4, 2e-3, 0.01, 0.02][int(rng.integers(4))]
    cfg = config.resolve_config(config.base_params(
        robot_name=robot, dt=dt, simulation_time=5.5 * dt, wcv=rng.uniform(60.0, 120.0 if dt == 0.02 else 250.0, 6),
        w_u=float(10 ** rng.uniform(-3, -1.5)), w_qddot=float(10 ** rng.uniform(-2.3, -1)), px_ref=float(rng.uniform(0.3, 0.55)),
        vy_ref=float(rng.uniform(-0.05, 0.08)), surface_coeffs=coeffs, translation_ee_t=tuple(rng.uniform(-0.1, 0.2, 3))))
    cfg["w_task"] = rng.uniform(5.0, 80.0, 5)               # the oracle's parameter record carries the task weights
    return cfg, robots.builtin_chain(robot)


@pytest.mark.parametrize("robot", ["ur10", "ur5"])
def test_assembly_matches_the_oracle_stage_residual(orc, robot):
    """r and Jr over random states, surfaces, tool offsets, bandwidths, sampling times and targets; then the weighted
    Hessian of a stage with random weights.  The distances are rounding of two evaluation orders (ASSEMBLY_TOL)."""
    import reference_checks as rc

    rng = np.random.default_rng(17 if robot == "ur10" else 18)
    worst = dict(r_task=0.0, J_task=0.0, r_lin=0.0, J_lin=0.0, H_rel=0.0)
    for _ in range(200):
        cfg, chain = _random_stage(rng, robot)
        rb, p = orc.make_robot(chain, cfg["t_ee"]), orc.make_params(cfg)
        x = np.concatenate([rng.uniform(-np.pi, np.pi, 6), rng.uniform(-1.5, 1.5, 6)])
        u = rng.uniform(-2.0, 2.0, 6)
        y = rng.normal([0.0, 1.0, 0.0, 0.4, 0.03], 0.1)
        r0, J0 = rc.stage_residual(orc, rb, p, cfg, x, u, y)
        r1, J1 = dq.stage_residual(chain, cfg, x, u, y)
        dr, dJ = np.abs(r1 - r0), np.abs(J1 - J0)
        new = dict(r_task=dr[:5].max(), J_task=dJ[:5].max(), r_lin=dr[5:].max(), J_lin=dJ[5:].max())
        W0, W1 = rc._weights(cfg), dq.weights(cfg)
        H0, H1 = cfg["dt"] * J0.T @ (W0[:, None] * J0), cfg["dt"] * J1.T @ (W1[:, None] * J1)
        new["H_rel"] = np.abs(H1 - H0).max() / np.abs(H0).max()
        worst = {k: max(v, float(new[k])) for k, v in worst.items()}
    print(f"\n[dense] {robot}: max |dense - oracle| " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= ASSEMBLY_TOL[k], (k, v)


def test_complex_step_jacobian_against_central_differences():
    """A coarse cross-check of the differentiation itself (the complex step is exact to rounding; central differences at
    h = 1e-6 are good to about 1e-9 here)."""
    from robotic_mpc_amd import robots

    rng = np.random.default_rng(3)
    cfg, chain = _random_stage(rng, "ur10")
    x, u = np.concatenate([rng.uniform(-2, 2, 6), rng.uniform(-1, 1, 6)]), rng.uniform(-1, 1, 6)
    r, Jr = dq.stage_residual(chain, cfg, x, u)
    z = np.concatenate([u, x])
    for j in range(18):
        d = np.zeros(18); d[j] = 1e-6
        rp = dq.stage_residual(chain, cfg, (z + d)[6:], (z + d)[:6])[0]
        rm = dq.stage_residual(chain, cfg, (z - d)[6:], (z - d)[:6])[0]
        np.testing.assert_allclose(Jr[:, j], (rp - rm) / 2e-6, atol=2e-8, rtol=0)


def test_solve_equality_and_certify_on_random_qps(orc):
    """The dense solver on random OCP-QPs: its solution satisfies the equalities and cannot be improved along them; on bounded
    QPs a point that tests/helpers.qp_kkt_residuals certifies as optimal gets the certificate's three verdicts, a perturbed one
    is at its distance, and the bound-ignoring minimiser of a tight QP is refused."""
    import helpers

    for N, tight in ((1, False), (5, False), (20, True), (60, True)):
        rng = np.random.default_rng(10 + N)
        H, g, b, A, B, lb, ub, dx0 = helpers.random_ocp_qp(rng, N, tight=tight)
        qp = dq.QP(H, g, b, A, B, lb, ub, dx0)
        eq = dq.solve_equality(qp)
        res = np.abs(A @ eq["dX"][:-1].T + B @ eq["dU"].T + b.T - eq["dX"][1:].T).max()
        assert res < 1e-13 and np.abs(eq["dX"][0] - dx0).max() < 1e-15 and eq["lu_vs_refined"] < 1e-11
        v0 = qp.value(eq["w"])
        for _ in range(5):                                  # a direction that keeps the equalities cannot lower the value
            dU = rng.normal(size=(N, 6)) * 1e-3
            dX = np.zeros((N + 1, 12))
            for k in range(N):
                dX[k + 1] = A @ dX[k] + B @ dU[k]
            assert qp.value(eq["w"] + qp.join(dX, dU)) > v0
        q = orc.qp_ipm(H, g, b, A, B, lb, ub, dx0, tol=1e-9, iter_max=80)
        kkt = helpers.qp_kkt_residuals(H, g, b, A, B, lb, ub, dx0, q["w"], q["pi"], q["lam"], q["t"])
        assert q["status"] == 0 and max(kkt.values()) < 1e-7, kkt
        dX, dU = q["w"][:, 6:], q["w"][:N, :6]
        cert = dq.certify(qp, dX, dU)
        assert cert["distance"] < 1e-6 and cert["min_multiplier"] >= 0 and cert["min_slack"] >= 0, cert
        dX, dU = cert["dX"], cert["dU"]                       # the certified optimum itself
        assert dq.certify(qp, dX, dU)["distance"] < 1e-13
        assert cert["n_active"] > 0 or not tight
        off = dq.certify(qp, dX, dU + 1e-7 * rng.choice([-1.0, 1.0], size=dU.shape))     # stays inside the active window
        assert 5e-8 < off["distance"] < 1e-5
        if tight:
            bad = dq.certify(qp, eq["dX"], eq["dU"])          # ignores the bounds: not a solution
            assert not (bad["distance"] < 1e-7 and bad["min_multiplier"] >= 0 and bad["min_slack"] >= 0)


def _distance(case, dX, dU):
    """(distance to the dense solution, the certificate or solve) of a candidate QP step of a case; the certificate's verdict on
    the active set is asserted for cases with active bounds."""
    qp = dc.dense_qp(case)
    if case["active"]:
        cert = dq.certify(qp, dX, dU)
        assert cert["n_active"] > 0 and cert["min_multiplier"] > 0 and cert["min_slack"] >= SEPARATION["free_slack"], cert
        assert cert["candidate_min_slack"] >= SEPARATION["free_slack"], cert
        return cert["distance"], cert
    sol = dc.dense_solution(case)
    idx, lo, hi = qp.bounded()
    assert np.minimum(sol["w"][idx] - lo, hi - sol["w"][idx]).min() >= 0.05        # strictly inside every bound
    return float(max(np.abs(sol["dX"] - dX).max(), np.abs(sol["dU"] - dU).max())), sol


@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_oracle_qp_solvers_against_dense(orc, cid):
    """orc.qp_fast / orc.qp_ipm (qp_tol 1e-12, 200 iterations) on the oracle's own assembly against solve_equality / certify on
    the independent one; the measured distance must stay within the derived bound of its own committed value, and the case
    must separate (active within 1e-6, free slack >= 1e-5, active multipliers > 0)."""
    case = BY_ID[cid]
    o = dc.oracle_solution(orc, case)
    assert o["status"] == 0 and o["accepted"] == (case["fast"] and not case["active"])
    dist, sol = _distance(case, o["dX"], o["dU"])
    print(f"\n[dense] {cid}: |oracle - dense| = {dist:.2e}, LU vs refined = {sol['lu_vs_refined']:.1e}")
    assert dist <= dc.tolerance(ORACLE_VS_DENSE, cid)
    assert sol["lu_vs_refined"] <= 1e-11


# (case, wavefronts, chunk pool in doubles, the sweep family it must take): the pools and wave counts of tests/test_boundaries.py
EMULATED = [
    ("N1-rand", 1, 19392, "resident"), ("N2-rand-ipm", 2, 19392, "resident"), ("N7-rand-ipm", 4, 9152, "resident"),
    ("N20-rand", 4, 19392, "resident"), ("N20-ur5", 4, 19392, "resident"), ("N20-tool", 2, 19392, "resident"),
    ("N20-ramp", 4, 19392, "resident"), ("N20-lm", 8, 19392, "resident"), ("N100-lm-ipm", 8, 19392, "resident"),
    ("N100-rand", 4, 19392, "resident"), ("N100-rand-ipm", 8, 19392, "resident"), ("N125-rand", 8, 19392, "resident"),
    ("N126-rand", 8, 19392, "segment"), ("N130-rand-ipm", 4, 19392, "segment"), ("N136-rand-ipm", 2, 19392, "segment"),
    ("N300-rand", 8, 19392, "segment"), ("N246-rand-ipm", 4, 19392, "segment"),
    ("N141-rand", 1, 19392, "streaming"), ("N141-rand-ipm", 1, 19392, "streaming"), ("N43-rand-ipm", 1, 9152, "streaming"),
    ("N38-rand-ipm", 2, 9152, "streaming"), ("N200-rand", 2, 9152, "streaming"),
    ("N26-rand-ipm", 4, 9152, "register"), ("N130-rand", 8, 9152, "register"), ("N246-rand-ipm", 4, 9152, "register"),
    ("N245-rand", 8, 9152, "register"),
    ("N20-tight", 4, 19392, "resident"), ("N20-default-ipm", 4, 9152, "resident"), ("N130-tight-ipm", 4, 19392, "segment"),
    ("N130-tight", 8, 9152, "register"), ("N130-tight", 1, 9152, "streaming"),
]


@needs_hipcc
@pytest.mark.parametrize("cid,waves,pool,sweep", EMULATED, ids=["%s-w%d-p%d-%s" % e for e in EMULATED])
def test_emulated_latency_engine_against_dense(cid, waves, pool, sweep):
    """Engine::control_step on the host (tests/emu): one reset step of SQP_RTI, minus the initial guess, is the QP's solution."""
    import emu
    import emu_ref

    case = BY_ID[cid]
    N = case["N"]
    assert emu.emu_paths(N, pool, waves)["sweep"] == sweep
    ctl = emu_ref.Controller([case["cfg"]], dc.chain_of(case), pool_doubles=pool, waves=waves)
    y = None if case["yref"] is None else case["yref"][None]
    out = ctl.step(case["xhat"][None], yref=y, ref_changed=y is not None)
    X, U = dc.guess(case)
    assert out["status"][0] == 0
    assert (out["qp_iter"][0] == 1) == (case["fast"] and not case["active"])
    dist, _ = _distance(case, out["x_pred"][0] - X, out["u_pred"][0] - U)
    print(f"\n[dense] {cid} w{waves} pool {pool} {sweep}: |emulated - dense| = {dist:.2e}")
    assert dist <= dc.tolerance(ORACLE_VS_DENSE, cid)
    np.testing.assert_array_equal(out["u0"][0], out["u_pred"][0][0])
    want = dq.nlp_cost(dc.chain_of(case), case["cfg"], out["x_pred"][0], out["u_pred"][0], case["yref"])
    np.testing.assert_allclose(out["cost"][0], want, rtol=1e-10, atol=0)


# |oracle - dense| of the three chained steps of CHAINED_CASE (orc.Solver, no reset), measured on the CPU; the bound of a step is
# 10 x its entry, floor 1e-12, as for the reset steps
CHAINED_ORACLE_VS_DENSE = (1.80e-14, 7.78e-15, 1.09e-15)


def chained_tolerance(k):
    return max(10.0 * CHAINED_ORACLE_VS_DENSE[k], 1e-12)


def test_oracle_chained_steps_against_dense(orc):
    d = dc.chained_distances(BY_ID[dc.CHAINED_CASE], dc.oracle_stepper(orc, BY_ID[dc.CHAINED_CASE]))
    print(f"\n[dense] chained steps: |oracle - dense| = {d}")
    assert len(d) == len(CHAINED_ORACLE_VS_DENSE) and all(v <= chained_tolerance(k) for k, v in enumerate(d))


@needs_hipcc
def test_emulated_chained_steps_against_dense():
    import emu_step

    case = BY_ID[dc.CHAINED_CASE]
    ctl = emu_step.Controller([case["cfg"]], dc.chain_of(case), pool_doubles=19392, waves=4)

    def step(x):
        out = ctl.step(x[None])
        assert out["status"][0] == 0
        return out["x_pred"][0], out["u_pred"][0]

    d = dc.chained_distances(case, step)
    print(f"\n[dense] chained steps: |emulated - dense| = {d}")
    assert all(v <= chained_tolerance(k) for k, v in enumerate(d))
