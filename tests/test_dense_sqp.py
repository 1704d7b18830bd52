"""The full-SQP outer loop of the oracle and of the emulated latency engine against the oracle-free replay of tests/dense_sqp.py:
every iteration's QP step (exact active-set certificate), step length (the L1 merit function with the reference's own Leineweber
weights, evaluated from first principles), the four KKT residual norms, the convergence test and the cost.

The cases (tests/dense_sqp_cases.py) backtrack: step lengths 0.7, 0.49 and 0.343, at iteration 0 (so that later QPs carry non-zero
dynamics defects and dx0, and the merit function's dynamics and x_0 terms are non-zero) and later, with and without active
bounds, at the horizons on both sides of every merit-lane / trial-group switch of the latency engine and of the throughput
engine's 64-stage strips.  A solver is stepped with nlp_solver_max_iter = 1 .. M from a reset each, so that every iterate is seen.

ORACLE_VS_DENSE_SQP is the committed record of the ORACLE's distances per case and iteration: (certificate distance of the QP
step, |res_stat|, |res_eq|, |res_ineq|, |res_comp| differences).  Every bound on an engine, here and in
tests/test_gpu_dense_sqp.py, is 10 x the entry, floor 1e-12 (dense_qp_cases.tolerance's rule); a case whose bound would exceed
1e-9 says nothing and is replaced.  tests/tools/dense_sqp_profile.py writes the table to profiles/dense_sqp_distances.txt.
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
import dense_sqp as ds  # noqa: E402
import dense_sqp_cases as sc  # noqa: E402
from test_dense_qp import SEPARATION  # noqa: E402

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

# case id -> per iteration (certificate, res_stat, res_eq, res_ineq, res_comp): |oracle - dense|, measured on the CPU
ORACLE_VS_DENSE_SQP = {
    "N12-steps": [
        (1.47e-14, 4.44e-16, 0.00e+00, 0.00e+00, 0.00e+00),
        (5.33e-15, 2.66e-15, 0.00e+00, 1.29e-14, 8.43e-16),
        (2.44e-14, 1.33e-15, 0.00e+00, 3.55e-15, 8.04e-16),
        (7.27e-12, 4.44e-16, 0.00e+00, 1.69e-14, 2.14e-15),
        (1.45e-11, 1.85e-13, 0.00e+00, 7.27e-12, 1.44e-15),
        (7.76e-12, 4.82e-14, 0.00e+00, 6.62e-12, 1.44e-12),
        (4.88e-15, 1.43e-13, 0.00e+00, 7.76e-12, 4.74e-14),
        (2.64e-15, 7.58e-14, 0.00e+00, 5.10e-12, 3.83e-14),
    ],
    "N12-active": [
        (5.18e-13, 1.11e-16, 0.00e+00, 0.00e+00, 0.00e+00),
        (2.49e-14, 2.22e-15, 4.44e-16, 5.17e-13, 8.28e-16),
        (2.67e-14, 2.78e-17, 0.00e+00, 2.31e-14, 8.17e-16),
        (7.76e-11, 1.50e-15, 0.00e+00, 2.49e-14, 8.22e-16),
        (2.42e-12, 8.74e-14, 0.00e+00, 7.76e-11, 6.81e-13),
        (8.38e-12, 3.39e-14, 0.00e+00, 2.42e-12, 2.44e-14),
        (1.23e-12, 5.86e-15, 0.00e+00, 8.38e-12, 8.01e-14),
        (5.90e-12, 1.47e-14, 4.44e-16, 1.23e-12, 1.20e-14),
    ],
    "N12-ipm": [
        (2.09e-14, 2.22e-16, 0.00e+00, 0.00e+00, 0.00e+00),
        (4.57e-13, 3.33e-16, 2.22e-16, 1.95e-14, 8.24e-16),
        (2.05e-15, 4.43e-15, 2.22e-16, 4.56e-13, 3.81e-15),
        (4.32e-12, 3.34e-15, 0.00e+00, 1.34e-13, 1.94e-15),
        (4.96e-13, 1.18e-14, 0.00e+00, 4.31e-12, 3.58e-14),
        (8.35e-13, 6.54e-14, 0.00e+00, 1.64e-12, 1.63e-14),
        (6.51e-15, 7.94e-15, 2.22e-16, 1.08e-12, 9.62e-15),
        (1.85e-15, 1.27e-14, 2.22e-16, 3.26e-13, 3.20e-15),
    ],
    "N12-ramp": [
        (2.18e-14, 2.22e-16, 0.00e+00, 0.00e+00, 0.00e+00),
        (4.86e-15, 6.66e-16, 2.22e-16, 2.00e-14, 8.43e-16),
        (1.90e-15, 8.88e-16, 0.00e+00, 3.08e-15, 8.38e-16),
        (1.89e-15, 6.38e-16, 0.00e+00, 8.88e-16, 8.34e-16),
        (3.26e-13, 8.33e-16, 0.00e+00, 8.88e-16, 8.36e-16),
        (8.81e-12, 1.87e-15, 0.00e+00, 3.25e-13, 1.43e-15),
        (3.15e-13, 1.59e-13, 0.00e+00, 8.81e-12, 2.86e-14),
        (3.64e-14, 5.57e-14, 0.00e+00, 2.86e-12, 1.16e-14),
    ],
    "N12-converges": [
        (6.66e-16, 2.22e-16, 0.00e+00, 0.00e+00, 0.00e+00),
        (1.00e-15, 1.39e-17, 1.63e-17, 8.88e-16, 0.00e+00),
        (0.00e+00, 1.39e-17, 3.23e-17, 2.22e-16, 0.00e+00),
        (0.00e+00, 1.39e-17, 3.23e-17, 2.22e-16, 0.00e+00),
    ],
    "N63-merit": [
        (2.82e-13, 0.00e+00, 0.00e+00, 0.00e+00, 0.00e+00),
        (6.51e-14, 2.22e-16, 0.00e+00, 6.39e-14, 0.00e+00),
        (7.28e-14, 1.11e-16, 4.36e-17, 6.31e-14, 0.00e+00),
    ],
    "N64-merit": [
        (2.83e-13, 0.00e+00, 0.00e+00, 0.00e+00, 0.00e+00),
        (3.46e-14, 0.00e+00, 2.78e-17, 6.57e-14, 0.00e+00),
        (2.35e-14, 1.05e-15, 1.60e-17, 3.29e-14, 0.00e+00),
    ],
    "N127-merit": [
        (5.50e-11, 0.00e+00, 0.00e+00, 0.00e+00, 0.00e+00),
        (2.99e-14, 1.55e-15, 0.00e+00, 1.72e-12, 3.77e-15),
        (3.11e-13, 1.33e-15, 0.00e+00, 1.13e-12, 3.73e-13),
    ],
    "N128-merit": [
        (1.58e-12, 1.11e-16, 0.00e+00, 0.00e+00, 0.00e+00),
        (2.64e-11, 8.88e-16, 0.00e+00, 6.09e-13, 0.00e+00),
        (8.26e-14, 6.66e-16, 0.00e+00, 2.50e-13, 3.48e-15),
    ],
    "N255-merit": [
        (7.03e-11, 2.22e-16, 0.00e+00, 0.00e+00, 0.00e+00),
        (5.14e-14, 2.44e-15, 0.00e+00, 1.34e-11, 0.00e+00),
    ],
    "N256-merit": [
        (7.09e-11, 2.22e-16, 0.00e+00, 0.00e+00, 0.00e+00),
        (2.66e-11, 2.66e-15, 0.00e+00, 1.35e-11, 0.00e+00),
    ],
}
N_CASES = 11

CASES = sc.all_cases()
BY_ID = {c["id"]: c for c in CASES}


def test_case_list_is_complete():
    assert len(CASES) == N_CASES and sorted(ORACLE_VS_DENSE_SQP) == sorted(BY_ID)
    assert {c["N"] for c in CASES} == {12, 63, 64, 127, 128, 255, 256}
    for c in CASES:
        assert len(ORACLE_VS_DENSE_SQP[c["id"]]) == c["M"] and c["cfg"]["solver_type"] == 0 and c["cfg"]["qp_tol"] == 1e-12
        assert c["M"] <= (8 if c["N"] == 12 else 2 if c["N"] >= 255 else 3)
        assert max(sc.tolerance(ORACLE_VS_DENSE_SQP, c["id"], it, k) for it in range(c["M"]) for k in range(5)) <= 1e-9, c["id"]
    want = {cid: BY_ID[cid]["want"] for cid in BY_ID}
    assert len(set(want["N12-steps"]["alphas"].values())) >= 3                           # several different step lengths below 1
    assert set(want["N12-active"]["alphas"]) & set(want["N12-active"]["active_at"])       # active bounds on a backtracked iteration
    assert not BY_ID["N12-ipm"]["fast"] and want["N12-ipm"]["alphas"]
    assert BY_ID["N12-ramp"]["yref"] is not None and np.ptp(BY_ID["N12-ramp"]["yref"][:, 3]) > 0 and want["N12-ramp"]["alphas"]
    assert want["N12-converges"]["inactive"] and 0 < want["N12-converges"]["converges"] < BY_ID["N12-converges"]["M"]
    assert all(BY_ID["N12-converges"]["cfg"][k] == 1e-6 for k in ("tol", "tol_eq", "tol_ineq", "tol_comp"))
    for a, b in ((63, 64), (127, 128), (255, 256)):          # each backtracks at iteration 0 or 1; one of a pair at iteration 0
        firsts = [min(want[f"N{N}-merit"]["alphas"]) for N in (a, b)]
        assert max(firsts) <= 1 and min(firsts) == 0, (a, b, firsts)
        assert any(want[f"N{N}-merit"].get("defect_at") for N in (a, b))
    assert ds.FREE_SLACK == SEPARATION["free_slack"] and dq.ACTIVE_TOL == SEPARATION["active_within"]


def test_dense_sqp_module_is_independent_of_the_oracle_and_the_engine_sources():
    src = open(os.path.join(HERE, "dense_sqp.py")).read()
    for word in ("import oracle", "from oracle", "orc.", "robotic_mpc_amd", "helpers", "reference_checks", "emu", "dense_sqp_cases"):
        assert word not in src.split('"""', 2)[2], word


# ------------------------------------------------------------------------------------------- the reference's own checks
def _two_stage():
    from robotic_mpc_amd import config, robots

    cfg = config.resolve_config(config.base_params(prediction_horizon=2, simulation_time=0.05, qdot_min=np.full(6, -0.8),
                                                   qdot_max=np.full(6, 0.8), solver_options={"nlp_solver_type": "SQP"}))
    return cfg, robots.builtin_chain("ur10")


def test_merit_at_a_point_is_cost_plus_the_hand_computed_penalty():
    """Two stages, with every term of the penalty made non-zero by construction: a known dynamics defect e_k added to the
    propagated state, an input 0.25 past its upper and 0.5 past its lower bound, a joint angle 0.1 past qmax at stage 1 (and the same
    angle at stage 0, where no state bound applies), x_0 off xhat by a known d."""
    cfg, chain = _two_stage()
    A, B = dq.lti(cfg["wcv"], cfg["dt"])
    rng = np.random.default_rng(5)
    U = rng.uniform(-0.3, 0.3, (2, 6))
    U[0, 2] = cfg["umax"][2] + 0.25
    U[1, 4] = cfg["umin"][4] - 0.5
    e = rng.uniform(-0.1, 0.1, (2, 12))
    X = np.zeros((3, 12))
    X[0] = np.concatenate([cfg["q0"], cfg["qdot0"]])
    X[0, 1] = cfg["qmax"][1] + 0.1                      # stage 0: not a bound
    X[1] = A @ X[0] + B @ U[0] - e[0]
    X[1, :6] = cfg["q0"]; X[1, 3] = cfg["qmax"][3] + 0.1
    e[0] = A @ X[0] + B @ U[0] - X[1]                   # the defect after pinning the angles
    X[2] = A @ X[1] + B @ U[1] - e[1]
    d = rng.uniform(-0.2, 0.2, 12)
    st = ds.State(2)
    st.w_nu = rng.uniform(0.5, 2.0, (3, 12))
    st.w_lo, st.w_hi = rng.uniform(0.5, 2.0, 48), rng.uniform(0.5, 2.0, 48)
    hand = st.w_nu[0] @ np.abs(d) + st.w_nu[1] @ np.abs(e[0]) + st.w_nu[2] @ np.abs(e[1]) \
        + st.w_hi[2] * 0.25 + st.w_lo[18 + 4] * 0.5 + st.w_hi[18 + 6 + 3] * 0.1
    got = ds.merit(chain, cfg, X, U, X[0] + d, None, st)
    np.testing.assert_allclose(got - dq.nlp_cost(chain, cfg, X, U), hand, rtol=1e-12)
    assert hand > 1.0
    st0 = ds.State(2)                                   # zero weights: the cost alone
    assert ds.merit(chain, cfg, X, U, X[0] + d, None, st0) == dq.nlp_cost(chain, cfg, X, U)


def test_merit_weights_follow_leinewebers_rule():
    a, w = np.array([2.0, 3.0, 0.0, 5.0]), np.array([4.0, 1.0, 6.0, 5.0])
    np.testing.assert_array_equal(ds.merit_weight(True, w, a), a)
    np.testing.assert_array_equal(ds.merit_weight(False, w, a), [3.0, 3.0, 3.0, 5.0])
    assert ds.step_lengths()[:4] == [1.0, 0.7, 0.7 * 0.7, 0.7 * 0.7 * 0.7] and len(ds.step_lengths()) == 10
    assert ds.step_lengths()[8] >= 0.05 > ds.step_lengths()[9]


def test_residual_norms_vanish_at_a_qps_own_kkt_point():
    """A QP of N12-steps (eleven active bounds), re-centred on its certified solution: with the solution's multipliers and slacks
    the four norms are zero to rounding; with any one of them dropped the matching norm is not."""
    case = BY_ID["N12-steps"]
    X, U = sc.dc.guess(case)
    qp = dq.assemble(case["chain"], case["cfg"], X, U, case["xhat"], case["yref"])
    idx, lo, hi = qp.bounded()
    held = {}                                           # position in idx -> the bound it is held at
    for _ in range(100):                                # a plain primal active-set loop, nothing from a solver under test
        pos = sorted(held)
        sol = dq.solve_equality(qp, idx[pos], [held[p] for p in pos])
        w = sol["w"]
        out = [p for p in range(len(idx)) if p not in held and (w[idx[p]] < lo[p] - 1e-12 or w[idx[p]] > hi[p] + 1e-12)]
        if out:
            held.update({p: (lo[p] if w[idx[p]] < lo[p] else hi[p]) for p in out})
            continue
        lam = [(-m if held[p] == lo[p] else m) for p, m in zip(pos, sol["mult"])]
        if not pos or min(lam) >= 0:
            break
        del held[pos[int(np.argmin(lam))]]
    cert = dq.certify(qp, *qp.split(w))
    assert cert["min_multiplier"] > 0 and cert["min_slack"] > 0 and cert["n_active"] > 0
    nu, lam_lo, lam_hi, t_lo, t_hi = ds._qp_point(qp, cert)
    w = cert["w"]
    N = qp.N
    Hw = np.concatenate([np.einsum("kij,kj->ki", qp.H[:N], w[:18 * N].reshape(N, 18)), np.zeros((1, 18))])
    Hw[N, 6:] = qp.H[N][6:, 6:] @ w[18 * N:]
    dX, dU = qp.split(w)
    at = dq.QP(qp.H, qp.g + Hw, qp.b + (dX[:-1] @ qp.A.T + dU @ qp.B.T - dX[1:]), qp.A, qp.B,
               qp.lb - np.vstack([np.hstack([dU, dX[:-1, :6]]), np.zeros((1, 12))]),
               qp.ub - np.vstack([np.hstack([dU, dX[:-1, :6]]), np.zeros((1, 12))]), qp.dx0 - dX[0])
    st = ds.State(N)
    st.nu, st.lam_lo, st.lam_hi, st.t_lo, st.t_hi = nu, lam_lo, lam_hi, t_lo, t_hi
    scale = float(np.abs(qp.g).max())
    res = ds.residuals(at, st)
    assert res[0] <= 1e-12 * max(scale, 1.0) and res[1] <= 1e-14 and res[2] <= 1e-14 and res[3] == 0.0, res
    st.lam_hi = np.zeros_like(lam_hi); st.lam_lo = np.zeros_like(lam_lo)
    assert ds.residuals(at, st)[0] >= 0.5 * max(lam_lo.max(), lam_hi.max())
    st.lam_lo, st.lam_hi, st.t_lo = lam_lo, lam_hi, t_lo + 0.25
    r = ds.residuals(at, st)
    assert abs(r[2] - 0.25) <= 1e-14 and abs(r[3] - 0.25 * lam_lo.max()) <= 1e-12
    res0 = ds.residuals(qp, ds.State(N))                # a reset: t = 0, so res_ineq is the largest distance of the guess to a bound
    assert res0[1] == np.abs(qp.b).max() > 0 and res0[3] == 0.0 and res0[2] == max(np.abs(lo).max(), np.abs(hi).max(), np.abs(qp.dx0).max())


# ------------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_oracle_full_sqp_against_the_dense_replay(orc, cid):
    """Every iteration of the oracle's solve: decisions asserted by the replay, distances within 10 x their committed values."""
    case = BY_ID[cid]
    lines = []
    rows = ds.replay(case, *sc.oracle_runs(orc, case), log=lines.append)
    print(f"\n[dense sqp] oracle {cid}:\n" + "\n".join(lines))
    sc.check_purpose(case, rows)
    sc.check_bounds(ORACLE_VS_DENSE_SQP, case, rows, "oracle")


# ------------------------------------------------------------------------------------- the emulated latency engine
P1, P2 = 19392, 9152        # the chunk pools of tests/test_boundaries.py BOUNDARIES: one and two simulations per CU
# (case, wavefronts, pool, merit lanes per trial point, trial points per pass)
EMULATED = [
    ("N12-steps", 1, P1, 64, 1), ("N12-steps", 2, P1, 128, 1), ("N12-steps", 4, P1, 128, 2), ("N12-steps", 8, P1, 128, 2),
    ("N12-steps", 4, P2, 128, 2), ("N12-steps", 8, P2, 128, 2),
    ("N12-active", 2, P2, 128, 1), ("N12-active", 8, P1, 128, 2), ("N12-ipm", 1, P2, 64, 1), ("N12-ipm", 4, P1, 128, 2),
    ("N12-ramp", 1, P1, 64, 1), ("N12-ramp", 2, P1, 128, 1), ("N12-ramp", 4, P2, 128, 2), ("N12-ramp", 8, P1, 128, 2),
    ("N12-converges", 4, P1, 128, 2), ("N12-converges", 1, P1, 64, 1),
    ("N63-merit", 1, P1, 64, 1), ("N64-merit", 1, P1, 64, 1), ("N63-merit", 4, P1, 128, 2), ("N64-merit", 8, P2, 128, 2),
    ("N127-merit", 2, P1, 128, 1), ("N128-merit", 2, P1, 128, 1), ("N127-merit", 4, P1, 128, 2), ("N128-merit", 4, P1, 256, 1),
    ("N127-merit", 8, P1, 128, 2), ("N128-merit", 8, P1, 256, 2), ("N128-merit", 1, P1, 64, 1),
    ("N128-merit", 4, P2, 256, 1), ("N128-merit", 8, P2, 256, 2),
    ("N255-merit", 4, P1, 256, 1), ("N256-merit", 4, P1, 256, 1), ("N255-merit", 8, P1, 256, 2), ("N256-merit", 8, P1, 512, 1),
]


def test_emulated_list_covers_every_merit_layout():
    """Both sides of every merit switch of tests/test_gpu_boundaries.py LATENCY_MERIT up to N = 256, the horizons at which a
    lane starts to sum several stages, every wave count and both pools."""
    from test_gpu_boundaries import LATENCY_MERIT

    have = {(w, BY_ID[c]["N"], l, g) for c, w, _, l, g in EMULATED}
    assert {m for m in LATENCY_MERIT if m[1] <= 256} <= have
    assert {(1, 63, 64, 1), (1, 64, 64, 1), (2, 127, 128, 1), (2, 128, 128, 1)} <= have
    assert {w for _, w, _, _, _ in EMULATED} == {1, 2, 4, 8} and {p for _, _, p, _, _ in EMULATED} == {P1, P2}
    assert {c for c, *_ in EMULATED} == set(BY_ID)


@needs_hipcc
@pytest.mark.parametrize("cid,waves,pool,lanes,groups", EMULATED, ids=["%s-w%d-p%d-l%d_g%d" % e for e in EMULATED])
def test_emulated_latency_engine_against_the_dense_replay(cid, waves, pool, lanes, groups):
    import emu

    case = BY_ID[cid]
    p = emu.emu_paths(case["N"], pool, waves)
    assert (p["merit_lanes"], p["merit_groups"]) == (lanes, groups), p
    lines = []
    rows = ds.replay(case, *sc.emulated_runs(case, waves, pool), log=lines.append)
    print(f"\n[dense sqp] emulated w{waves} pool {pool} {cid}:\n" + "\n".join(lines))
    sc.check_purpose(case, rows)
    sc.check_bounds(ORACLE_VS_DENSE_SQP, case, rows, f"emulated w{waves} pool {pool}")
