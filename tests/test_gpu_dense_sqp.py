"""BatchController's full-SQP step on the device against the oracle-free replay of tests/dense_sqp.py: every SQP iteration's QP
step, step length, the four KKT residual norms, the convergence test and the cost (see tests/test_dense_sqp.py).

The iteration limit is batch-wide, so iterate m of a case comes from a controller of its own built with nlp_solver_max_iter = m:
one reset step with predictions returned.  The cases of one horizon share a batch.  Every case runs on engine="stream" and on
engine="latency" at the default launch geometry; on the latency engine the merit-shape cases also run under MPCB_WAVES_PER_SIM /
MPCB_SIMS_PER_CU on both sides of that geometry's merit-lane / trial-group switches, and N = 12 and N = 128 at one and at two
simulations per CU (the halved pool: the merit pass takes N = 128 in chunks).  The bound of every distance is 10 x the committed
oracle distance of its case, iteration and quantity, floor 1e-12 (tests/test_dense_sqp.py ORACLE_VS_DENSE_SQP).

DENSE_SQP_DUMP=<file> collects the measured device-vs-dense distances (tests/tools/dense_sqp_profile.py).
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)

import dense_sqp as ds  # noqa: E402
import dense_sqp_cases as sc  # noqa: E402
from test_boundaries import BOUNDARIES, _named  # noqa: E402
from test_dense_sqp import BY_ID, CASES, ORACLE_VS_DENSE_SQP  # noqa: E402

pytestmark = pytest.mark.gpu

GROUPS = {}
for _c in CASES:
    GROUPS.setdefault(_c["N"], []).append(_c["id"])

# forced latency geometries (wavefronts per simulation, simulations per CU) -> horizons
GEOMETRY_HORIZONS = {
    (8, 1): (127, 128, 255, 256), (4, 1): (127, 128, 255, 256),
    (1, 1): (12, 128), (2, 1): (12, 128), (4, 2): (12, 128), (8, 2): (12, 128),
}
RUNS = [("stream", None, N) for N in GROUPS] + [("latency", None, N) for N in GROUPS] + \
       [("latency", geo, N) for geo, Ns in GEOMETRY_HORIZONS.items() for N in Ns]
N_RUNS = 2 * 7 + 16


def _run_id(r):
    engine, geo, N = r
    return "%s%s-N%d" % (engine, "" if geo is None else "-w%d_s%d" % geo, N)


def test_run_list_is_complete():
    from test_gpu_boundaries import LATENCY_MERIT

    assert sorted(GROUPS) == [12, 63, 64, 127, 128, 255, 256] and len(RUNS) == N_RUNS
    assert sorted(c for ids in GROUPS.values() for c in ids) == sorted(BY_ID)
    forced = {(geo[0], N) for geo, Ns in GEOMETRY_HORIZONS.items() if geo[1] == 1 for N in Ns}
    assert {(w, N) for w, N, _, _ in LATENCY_MERIT if N <= 256} <= forced          # both sides of every merit switch up to 256
    for geo in ((1, 1), (2, 1), (4, 2), (8, 2)):
        assert GEOMETRY_HORIZONS[geo] == (12, 128)
    assert {BOUNDARIES[g]["pool"] for g in GEOMETRY_HORIZONS} == {19392, 9152}


_DEVICE = {}


def _record(cid, tag, dist):
    have = _DEVICE.setdefault(cid, {}).get(tag)
    _DEVICE[cid][tag] = dist if have is None else [tuple(max(a, b) for a, b in zip(r0, r1)) for r0, r1 in zip(have, dist)]
    if os.environ.get("DENSE_SQP_DUMP"):
        with open(os.environ["DENSE_SQP_DUMP"], "w") as f:
            json.dump(_DEVICE, f, indent=1, sort_keys=True)


def _step(cases, m, engine):
    """One reset step of the cases (one horizon) with nlp_solver_max_iter = m."""
    from robotic_mpc_amd import BatchController

    ctl = BatchController([sc.raw_at(c, m) for c in cases], engine=engine)
    y = None
    if any(c["yref"] is not None for c in cases):
        y = ctl.default_reference().cpu().numpy()
        for i, c in enumerate(cases):
            if c["yref"] is not None:
                y[i, :c["N"]] = c["yref"]
    out = {k: v.cpu().numpy() for k, v in ctl.step(np.stack([c["xhat"] for c in cases]), predict=True, yref=y).items()}
    info = ctl.launch_info()
    ctl.close()
    return out, info


@pytest.mark.parametrize("engine,geo,N", RUNS, ids=[_run_id(r) for r in RUNS])
def test_full_sqp_step_against_the_dense_replay(monkeypatch, engine, geo, N):
    import emu

    for k in ("MPCB_WAVES_PER_SIM", "MPCB_SIMS_PER_CU", "MPCB_ENGINE"):
        monkeypatch.delenv(k, raising=False)
    if geo is not None:
        monkeypatch.setenv("MPCB_WAVES_PER_SIM", str(geo[0]))
        monkeypatch.setenv("MPCB_SIMS_PER_CU", str(geo[1]))
    cases = [BY_ID[c] for c in GROUPS[N]]
    Z = {c["id"]: [sc.dc.guess(c)] for c in cases}
    reports = {c["id"]: [None] for c in cases}
    for m in range(1, max(c["M"] for c in cases) + 1):
        batch = [c for c in cases if c["M"] >= m]
        out, info = _step(batch, m, engine)
        assert info["engine"] == (1 if engine == "stream" else 0), info
        if geo is not None:
            assert info["waves_per_sim"] == geo[0] and info["pool_bytes"] == 8 * BOUNDARIES[geo]["pool"], info
            p = emu.emu_paths(N, info["pool_bytes"] // 8, geo[0])
            assert (p["sweep"], p["merit_lanes"], p["merit_groups"]) == _named(geo, N), p
        for i, c in enumerate(batch):
            assert np.isfinite(out["x_pred"][i]).all() and np.isfinite(out["u_pred"][i]).all(), (c["id"], m)
            np.testing.assert_array_equal(out["u0"][i], out["u_pred"][i][0])
            Z[c["id"]].append((out["x_pred"][i], out["u_pred"][i]))
            reports[c["id"]].append(dict(status=int(out["status"][i]), sqp_iter=int(out["sqp_iter"][i]), residuals=out["residuals"][i],
                                         cost=float(out["cost"][i])))
    tag = "%s%s" % (engine, "" if geo is None else "-w%d_s%d" % geo)
    for c in cases:
        lines = []
        rows = ds.replay(c, Z[c["id"]], reports[c["id"]], log=lines.append)
        print(f"\n[dense sqp] {tag} {c['id']}:\n" + "\n".join(lines))
        sc.check_purpose(c, rows)
        _record(c["id"], tag, sc.distances(rows))
        sc.check_bounds(ORACLE_VS_DENSE_SQP, c, rows, tag)
