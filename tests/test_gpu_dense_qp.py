"""BatchController on the device against the dense KKT reference of tests/dense_qp.py, which shares nothing with the engines or
the oracle: one SQP_RTI reset step with predictions returned, minus the initial guess, is the solution of one Gauss-Newton QP.

Every case of tests/dense_qp_cases.py runs on engine="stream" and on engine="latency" at the default launch geometry; on the
latency engine the cases at both sides of each forced geometry's sweep switch, at N = 20 and N = 130 (with their active-bound
cases) and at N = 300 also run under MPCB_WAVES_PER_SIM / MPCB_SIMS_PER_CU, the switches of tests/test_gpu_boundaries.py.  The
bound of a case is 10 x its committed oracle-vs-dense distance, floor 1e-12 (tests/test_dense_qp.py ORACLE_VS_DENSE); cases
with active bounds are held to the same bound on the distance to their exact active-set certificate, with status 0.

`cost` of a step is acados' get_cost(): the NLP cost at the RETURNED iterate, not the QP's model value; it is compared with the
independent residuals evaluated there.

DENSE_QP_DUMP=<file> collects the measured device-vs-dense distances (tests/tools/dense_qp_profile.py).
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import dense_qp as dq  # noqa: E402
import dense_qp_cases as dc  # noqa: E402
from test_boundaries import BOUNDARIES, _named  # noqa: E402
from test_dense_qp import BY_ID, CASES, ORACLE_VS_DENSE, SEPARATION, chained_tolerance  # noqa: E402

pytestmark = pytest.mark.gpu


def _group_key(c):
    return (c["robot"], tuple(np.asarray(c["cfg"]["t_ee"]).tolist()), c["N"], c["yref"] is not None)


GROUPS = {}
for _c in CASES:
    GROUPS.setdefault(_group_key(_c), []).append(_c["id"])
GROUP_IDS = {k: "%s-N%d%s%s" % (k[0], k[2], "-tool" if k[1] != (0.0, 0.0, 0.1) else "", "-ref" if k[3] else "") for k in GROUPS}
MAIN = {k[2]: k for k in GROUPS if k[0] == "ur10" and k[1] == (0.0, 0.0, 0.1) and not k[3]}

# forced latency geometries (wavefronts per simulation, simulations per CU) -> horizons: both sides of the geometry's sweep switch
# (tests/test_boundaries.py BOUNDARIES), N = 20 and N = 130 with their active-bound cases, N = 300 where seams follow
GEOMETRY_HORIZONS = {
    (1, 1): (20, 130, 140, 141, 300), (2, 1): (20, 130, 135, 136, 300), (4, 1): (20, 125, 126, 130, 300),
    (8, 1): (20, 125, 126, 130, 300), (1, 2): (20, 42, 43, 130), (2, 2): (20, 37, 38, 130),
    (4, 2): (20, 25, 26, 130, 300), (8, 2): (20, 25, 26, 130, 300),
}
RUNS = [("stream", None, k) for k in GROUPS] + [("latency", None, k) for k in GROUPS] + \
       [("latency", geo, MAIN[N]) for geo, Ns in GEOMETRY_HORIZONS.items() for N in Ns]
N_RUNS = 2 * 29 + 38


def _run_id(r):
    engine, geo, key = r
    return "%s%s-%s" % (engine, "" if geo is None else "-w%d_s%d" % geo, GROUP_IDS[key])


def test_run_list_is_complete():
    assert len(GROUPS) == 29 and len(RUNS) == N_RUNS
    assert sorted(c for ids in GROUPS.values() for c in ids) == sorted(BY_ID)
    assert sorted(GEOMETRY_HORIZONS) == sorted(BOUNDARIES)
    for geo, Ns in GEOMETRY_HORIZONS.items():
        first = BOUNDARIES[geo]["sweep"][1][0]
        assert first - 1 in Ns and first in Ns and {_named(geo, N)[0] for N in Ns} >= {s for _, s in BOUNDARIES[geo]["sweep"]}
    for N in (20, 130):                                 # an inactive and an active case wherever a geometry runs these horizons
        kinds = {BY_ID[c]["active"] for c in GROUPS[MAIN[N]]}
        assert kinds == {False, True}


_DEVICE = {}


def _record(cid, tag, dist):
    _DEVICE.setdefault(cid, {})
    _DEVICE[cid][tag] = max(dist, _DEVICE[cid].get(tag, 0.0))
    if os.environ.get("DENSE_QP_DUMP"):
        with open(os.environ["DENSE_QP_DUMP"], "w") as f:
            json.dump(_DEVICE, f, indent=1, sort_keys=True)


def _check(case, out, i, tag, Nmax=None):
    """One simulation of a step's output against the dense reference of its case; returns the distance."""
    N = case["N"]
    X, U = dc.guess(case)
    xp, up = out["x_pred"][i], out["u_pred"][i]
    if Nmax is not None:
        assert np.isnan(xp[N + 1:]).all() and np.isnan(up[N:]).all(), case["id"]
    xp, up = xp[:N + 1], up[:N]
    assert np.isfinite(xp).all() and np.isfinite(up).all() and out["status"][i] == 0, (case["id"], out["status"][i])
    assert (out["qp_iter"][i] == 1) == (case["fast"] and not case["active"]), (case["id"], out["qp_iter"][i])
    qp = dc.dense_qp(case)
    if case["active"]:
        cert = dq.certify(qp, xp - X, up - U)
        assert cert["n_active"] > 0 and cert["min_multiplier"] >= 0 and cert["min_slack"] >= 0, (case["id"], cert)
        assert cert["candidate_min_slack"] >= SEPARATION["free_slack"], (case["id"], cert)
        dist = cert["distance"]
    else:
        sol = dc.dense_solution(case)
        dist = float(max(np.abs(sol["dX"] - (xp - X)).max(), np.abs(sol["dU"] - (up - U)).max()))
    print(f"\n[dense] {tag} {case['id']}: |device - dense| = {dist:.2e} (bound {dc.tolerance(ORACLE_VS_DENSE, case['id']):.1e})")
    _record(case["id"], tag.split()[0], dist)
    assert dist <= dc.tolerance(ORACLE_VS_DENSE, case["id"]), (tag, case["id"], dist)
    np.testing.assert_array_equal(out["u0"][i], up[0])
    want = dq.nlp_cost(dc.chain_of(case), case["cfg"], xp, up, case["yref"])
    np.testing.assert_allclose(out["cost"][i], want, rtol=1e-9, atol=0, err_msg=case["id"])
    return dist


def _step(cases, engine, predict=True):
    from robotic_mpc_amd import BatchController

    ctl = BatchController([c["raw"] for c in cases], engine=engine)
    y = None
    if any(c["yref"] is not None for c in cases):
        y = ctl.default_reference().cpu().numpy()
        for i, c in enumerate(cases):
            if c["yref"] is not None:
                y[i, :c["N"]] = c["yref"]
    out = {k: v.cpu().numpy() for k, v in ctl.step(np.stack([c["xhat"] for c in cases]), predict=predict, yref=y).items()}
    info = ctl.launch_info()
    ctl.close()
    return out, info


@pytest.mark.parametrize("engine,geo,key", RUNS, ids=[_run_id(r) for r in RUNS])
def test_reset_step_against_dense(monkeypatch, engine, geo, key):
    for k in ("MPCB_WAVES_PER_SIM", "MPCB_SIMS_PER_CU", "MPCB_ENGINE"):
        monkeypatch.delenv(k, raising=False)
    if geo is not None:
        monkeypatch.setenv("MPCB_WAVES_PER_SIM", str(geo[0]))
        monkeypatch.setenv("MPCB_SIMS_PER_CU", str(geo[1]))
    cases = [BY_ID[c] for c in GROUPS[key]]
    out, info = _step(cases, engine)
    assert info["engine"] == (1 if engine == "stream" else 0), info
    if geo is not None:
        assert info["waves_per_sim"] == geo[0] and info["pool_bytes"] == 8 * BOUNDARIES[geo]["pool"], info
    tag = "%s%s" % (engine, "" if geo is None else "-w%d_s%d" % geo)
    for i, c in enumerate(cases):
        _check(c, out, i, tag)


def test_fast_path_on_and_off_meet_the_same_dense_solution():
    """N20-rand and N20-rand-ipm are one QP: both answers are within their bounds of ONE dense solution, so of each other."""
    a, b = BY_ID["N20-rand"], BY_ID["N20-rand-ipm"]
    assert dc.dense_solution(a) is dc.dense_solution(b)
    for engine in ("latency", "stream"):
        out, _ = _step([a, b], engine)
        assert out["qp_iter"][0] == 1 and out["qp_iter"][1] > 1
        bound = dc.tolerance(ORACLE_VS_DENSE, a["id"]) + dc.tolerance(ORACLE_VS_DENSE, b["id"])
        assert np.abs(out["u_pred"][0] - out["u_pred"][1]).max() <= bound


def test_ragged_batch_on_the_stream_engine():
    """Horizons {20, 50, 100, 200} in one batch: every simulation against the dense solution at its own N, NaN past it."""
    ids = ["N20-rand", "N20-rand-ipm", "N50-rand", "N100-rand", "N100-rand-ipm", "N200-rand", "N200-rand-ipm", "N20-tight", "N20-default-ipm"]
    cases = [BY_ID[c] for c in ids]
    out, info = _step(cases, "stream")
    assert info["engine"] == 1
    for i, c in enumerate(cases):
        _check(c, out, i, "stream-ragged", Nmax=200)


@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_three_chained_steps_against_dense(engine):
    from robotic_mpc_amd import BatchController

    case = BY_ID[dc.CHAINED_CASE]
    ctl = BatchController([case["raw"]], engine=engine)

    def step(x):
        out = {k: v.cpu().numpy() for k, v in ctl.step(x[None], predict=True).items()}
        assert out["status"][0] == 0
        return out["x_pred"][0], out["u_pred"][0]

    d = dc.chained_distances(case, step)
    ctl.close()
    print(f"\n[dense] chained steps {engine}: |device - dense| = {d}")
    for k, v in enumerate(d):
        _record("chained-step%d" % k, engine, v)
        assert v <= chained_tolerance(k), (k, v)
