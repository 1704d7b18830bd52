"""The cases of the full-SQP replay (tests/dense_sqp.py; tests/test_dense_sqp.py on the CPU, tests/test_gpu_dense_sqp.py on the
device): one reset solve each with nlp_solver_type "SQP", run M times with nlp_solver_max_iter = 1 .. M so that every iterate of
the solve is seen.

A case is dict(id, raw, cfg, N, M, xhat, yref, fast, chain, want): the parameters are helpers.random_parameter_cfgs draws (seed),
the feedback state is off the packed start by up to +-0.3 rad and +-1 rad/s -- far enough that the Gauss-Newton step overshoots and
the line search backtracks -- and every QP is solved at qp_tol 1e-12, 200 iterations, so that an interior-point solve lands on the
QP's solution to rounding.  `want` names what the case is there for and is asserted on the replay of every solver
(check_purpose): the step lengths by iteration, active bounds, the stopping iteration.

Seeds were chosen by a scan on the CPU (oracle iterates, replayed at qp_tol 1e-12; profiles/dense_sqp_distances.txt lists what was
replaced): seeds at which the purpose is met, every merit decision clears its threshold by 1e-6 |m0|, every residual its tolerance
by a factor 2, and the derived bound (10 x the oracle's distance) stays within 1e-9.
"""
import copy

import numpy as np

import dense_qp_cases as dc
import reference_checks as rc

SQP_OPTS = {"nlp_solver_type": "SQP", "qp_tol": 1e-12, "qp_solver_iter_max": 200}
A1, A2, A3 = 0.7, 0.7 * 0.7, 0.7 * 0.7 * 0.7


def sqp_case(cid, N, seed, M, fast=True, ramp=False, want=None, so=None):
    from robotic_mpc_amd import config

    raw = dc._random_raw(seed, prediction_horizon=N, simulation_time=0.05, solver_options=dict(SQP_OPTS, **(so or {})), qp_fast_path=fast)
    cfg = config.resolve_config(raw)
    rng = np.random.default_rng(seed)
    xhat = np.concatenate([cfg["q0"], cfg["qdot0"]]) + np.concatenate([rng.uniform(-0.3, 0.3, 6), rng.uniform(-1.0, 1.0, 6)])
    yref = rc.ramp_reference(cfg, N, px0=cfg["px_ref"] - 0.01, dpx=0.02 / N, vy0=cfg["vy_ref"], dvy=0.002) if ramp else None
    case = dict(id=cid, robot=cfg["robot_name"], raw=raw, cfg=cfg, N=N, M=M, xhat=xhat, yref=yref, fast=fast, want=want or {})
    case["chain"] = dc.chain_of(case)
    return case


def raw_at(case, m):
    """The case's configuration with nlp_solver_max_iter = m."""
    raw = copy.deepcopy(case["raw"])
    raw["solver_options"] = dict(raw["solver_options"], nlp_solver_max_iter=m)
    return raw


def cfg_at(case, m):
    from robotic_mpc_amd import config

    return config.resolve_config(raw_at(case, m))


# id, N, seed, M, then what the case must show (check_purpose):
#   alphas       {iteration: step length}, the iterations that backtrack (every other one takes the full step)
#   active_at    iterations whose QP has active bounds
#   inactive     no QP of the solve has an active bound
#   converges    the iteration at which the convergence test stops the solve (status 0, inside M)
#   defect_at    iterations whose QP has non-zero dynamics defects and dx0 (the iteration after a backtracked one)
TRAJECTORY = [
    dict(cid="N12-steps", N=12, seed=23, M=8),
    dict(cid="N12-active", N=12, seed=615, M=8),
    dict(cid="N12-ipm", N=12, seed=296, M=8, fast=False),
    dict(cid="N12-ramp", N=12, seed=17, M=8, ramp=True),
    dict(cid="N12-converges", N=12, seed=184, M=4),
]
MERIT_SHAPE = [
    dict(cid="N63-merit", N=63, seed=28, M=3),
    dict(cid="N64-merit", N=64, seed=28, M=3),
    dict(cid="N127-merit", N=127, seed=28, M=3),
    dict(cid="N128-merit", N=128, seed=64, M=3),
    dict(cid="N255-merit", N=255, seed=17, M=2),
    dict(cid="N256-merit", N=256, seed=17, M=2),
]
WANT = {
    "N12-steps": {"alphas": {2: A1, 4: A2, 6: A3}, "active_at": [0, 1, 2, 3, 4, 5, 6, 7]},
    "N12-active": {"alphas": {7: A1}, "active_at": [0, 1, 2, 3, 4, 5, 6, 7]},
    "N12-ipm": {"alphas": {2: A1, 4: A1, 5: A1, 6: A1, 7: A1}, "inactive": True},
    "N12-ramp": {"alphas": {6: A1}, "active_at": [0, 1, 2, 3, 4, 5, 6, 7]},
    "N12-converges": {"inactive": True, "converges": 2},
    "N63-merit": {"alphas": {0: A3}, "inactive": True, "defect_at": [1]},
    "N64-merit": {"alphas": {0: A3}, "inactive": True, "defect_at": [1]},
    "N127-merit": {"alphas": {0: A2, 1: A3, 2: A2}, "active_at": [0, 1, 2], "defect_at": [1]},
    "N128-merit": {"alphas": {0: A2, 1: A1, 2: A2}, "active_at": [1, 2], "defect_at": [1]},
    "N255-merit": {"alphas": {0: A3, 1: A2}, "active_at": [1], "defect_at": [1]},
    "N256-merit": {"alphas": {0: A3, 1: A2}, "active_at": [1], "defect_at": [1]},
}


def all_cases():
    out = []
    for spec in TRAJECTORY + MERIT_SHAPE:
        spec = dict(spec)
        cid = spec.pop("cid")
        out.append(sqp_case(cid, want=WANT.get(cid, {}), **spec))
    ids = [c["id"] for c in out]
    assert len(set(ids)) == len(ids)
    return out


def check_purpose(case, rows):
    """The replay of ANY solver on the case shows what the case is there for (`rows`: what dense_sqp.replay returned)."""
    want = case["want"]
    taken = {i: r["alpha"] for i, r in enumerate(rows) if not r["converged"] and r["alpha"] != 1.0}
    assert taken == want.get("alphas", {}), (case["id"], taken)
    act = [i for i, r in enumerate(rows) if r["n_active"] > 0]
    assert set(want.get("active_at", act)) <= set(act), (case["id"], act)
    if want.get("inactive"):
        assert not act, (case["id"], act)
    conv = [i for i, r in enumerate(rows) if r["converged"]]
    assert (conv[0] if conv else None) == want.get("converges"), (case["id"], conv)
    for i in want.get("defect_at", ()):
        assert rows[i]["defect"] > 1e-3 and rows[i]["penalty0"] > 1e-6, (case["id"], i, rows[i]["defect"], rows[i]["penalty0"])


def tolerance(table, cid, it, k):
    """The bound on an engine's distance k (0: certificate, 1..4: res_stat, res_eq, res_ineq, res_comp) at iteration `it` of a
    case: dense_qp_cases.tolerance's rule on the committed oracle distance, 10 x, floor 1e-12."""
    return max(10.0 * table[cid][it][k], 1e-12)


def distances(rows):
    """replay's rows as the table's tuples (certificate, res_stat, res_eq, res_ineq, res_comp); a converged row has no QP: 0."""
    return [(0.0 if r["cert"] is None else r["cert"], *[float(v) for v in r["res"]]) for r in rows]


def check_bounds(table, case, rows, what):
    """Every distance of every iteration within its derived bound; returns the distances."""
    d = distances(rows)
    assert len(d) == case["M"] == len(table[case["id"]]), (case["id"], len(d))
    for it, row in enumerate(d):
        for k, v in enumerate(row):
            assert v <= tolerance(table, case["id"], it, k), \
                f"{what} {case['id']} iteration {it} {('cert', 'res_stat', 'res_eq', 'res_ineq', 'res_comp')[k]}: {v:.3e} > {tolerance(table, case['id'], it, k):.1e}"
    return d


def oracle_runs(orc, case):
    """(Z, reports) of the oracle: a fresh solver per m = 1 .. M with nlp_solver_max_iter = m."""
    Z, reports = [dc.guess(case)], [None]
    for m in range(1, case["M"] + 1):
        cfg = cfg_at(case, m)
        s = orc.Solver(orc.make_robot(case["chain"], cfg["t_ee"]), orc.make_params(cfg))
        if case["yref"] is not None:
            s.set_reference(case["yref"])
        r = s.step(case["xhat"])
        X, U, _ = s.iterate()
        Z.append((X, U))
        reports.append(dict(status=r["status"], sqp_iter=r["sqp_iter"], residuals=r["res"], cost=r["cost"]))
    return Z, reports


def emulated_runs(case, waves, pool):
    """(Z, reports) of the emulated latency engine (tests/emu): a fresh controller per m, one reset step."""
    import emu_ref

    Z, reports = [dc.guess(case)], [None]
    y = None if case["yref"] is None else case["yref"][None]
    for m in range(1, case["M"] + 1):
        ctl = emu_ref.Controller([cfg_at(case, m)], case["chain"], pool_doubles=pool, waves=waves)
        o = ctl.step(case["xhat"][None], yref=y, ref_changed=y is not None)
        Z.append((o["x_pred"][0], o["u_pred"][0]))
        reports.append(dict(status=int(o["status"][0]), sqp_iter=int(o["sqp_iter"][0]), residuals=o["residuals"][0], cost=float(o["cost"][0])))
    return Z, reports
