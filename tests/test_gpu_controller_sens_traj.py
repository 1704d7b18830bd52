"""BatchController.step(sens_w=True) on the device (mpcb_step_sens_w on both engines) at a linearisation point that differs on every
stage: the trajectory cases of tests/sens_traj_cases.py.  W carried warm-up steps under a curved reference that advances one stage
per step, then the checked step with a [B] shift mask -- every case twice in the batch, one simulation carried and one shifted --
and du0_dx, du0_dyref and du0_dw of the one launch against the dense Jacobians at the engine's own previous prediction, under the
bound of the reset-step tests (tests/test_gpu_controller_sens.py, tests/test_gpu_controller_sensw.py), where every stage of the
iterate is the same and a pass that read another stage's Jacobians, operands or residual would return the same bits.

Latency engine: N = 2, 7, 20, 43, 130 at the default geometry, N = 20 and 130 at every geometry of tests/test_boundaries.py
BOUNDARIES (N = 130: more than one block of the pass wherever the gains are not resident).  Throughput engine, which has no host
emulation: N = 2, 7, 40, 130 and one ragged batch of horizons 3, 12, 40.  The plain pass (sens=True alone) at N = 20 on both.

SENS_DUMP=<file> collects the measured distances (profiles/step_sens_traj_distances.txt)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import dense_qp_cases as dc  # noqa: E402
import sens_traj_cases as tc  # noqa: E402
from test_boundaries import BOUNDARIES  # noqa: E402

pytestmark = pytest.mark.gpu

# (engine, forced (wavefronts per simulation, simulations per CU) or None, horizons of one batch: each twice, carried and shifted)
RUNS = [("latency", None, (N,)) for N in (2, 7, 20, 43, 130)] + \
       [("stream", None, (N,)) for N in (2, 7, 40, 130)] + [("stream", None, (3, 12, 40))] + \
       [("latency", geo, (N,)) for geo in sorted(BOUNDARIES) for N in (20, 130)]
_MEASURED = {}


def _run_id(r):
    return "%s%s-%s" % (r[0], "" if r[1] is None else "-w%d_s%d" % r[1], "+".join("N%d" % N for N in r[2]))


def _dump():
    if os.environ.get("SENS_DUMP"):
        tc.dump(os.environ["SENS_DUMP"], _MEASURED)


def _clean(monkeypatch, geo=None):
    for k in ("MPCB_WAVES_PER_SIM", "MPCB_SIMS_PER_CU", "MPCB_ENGINE"):
        monkeypatch.delenv(k, raising=False)
    if geo is not None:
        monkeypatch.setenv("MPCB_WAVES_PER_SIM", str(geo[0]))
        monkeypatch.setenv("MPCB_SIMS_PER_CU", str(geo[1]))


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _inputs(ctl, sims, j):
    """xhat [B, 12] and yref [B, Nmax, 5] of step j: each simulation's own rollout; rows past its horizon keep the packed reference."""
    x = np.stack([tc.rollout(N)["xhat"][j] for N in sims])
    y = ctl.default_reference().cpu().numpy()
    for i, N in enumerate(sims):
        y[i, :N] = tc.rollout(N)["yref"][j]
    return x, y


def _run(engine, horizons, tag, info=None, **kw):
    """The W warm-up steps of a batch that holds every horizon twice (checked against the dense QP at the engine's own iterate) and
    the checked step: even simulations carry, odd ones shift.  Returns (sims, previous predictions, the checked step's outputs)."""
    from robotic_mpc_amd import BatchController

    sims = [N for N in horizons for _ in tc.MODES]
    ctl = BatchController([tc.case(N)["raw"] for N in sims], engine=engine)
    try:
        prev = [dc.guess(tc.case(N)) for N in sims]
        for j in range(tc.W):
            x, y = _inputs(ctl, sims, j)
            out = _np(ctl.step(x, predict=True, yref=y, **kw))
            for i in range(0, len(sims), 2):
                for k in ("x_pred", "u_pred", "u0", "du0_dx"):
                    np.testing.assert_array_equal(out[k][i], out[k][i + 1], err_msg=k)      # one history for both modes
                prev[i] = prev[i + 1] = tc.check_warmup(sims[i], j, prev[i], out, i, tag)
        x, y = _inputs(ctl, sims, tc.W)
        shift = np.array([m == tc.SHIFTED for _ in horizons for m in tc.MODES])
        out = _np(ctl.step(x, predict=True, yref=y, shift=shift, **kw))
        if info is not None:
            info.update(ctl.launch_info())
    finally:
        ctl.close()
    return sims, prev, out


@pytest.mark.parametrize("engine,geo,horizons", RUNS, ids=[_run_id(r) for r in RUNS])
def test_checked_step_sensitivities_against_dense_at_a_stage_varying_iterate(monkeypatch, engine, geo, horizons):
    _clean(monkeypatch, geo)
    tag = "%s%s" % (engine, "" if geo is None else "-w%d_s%d" % geo) + ("-ragged" if len(horizons) > 1 else "")
    info = {}
    sims, prev, out = _run(engine, horizons, tag, info, sens_w=True)
    assert info["engine"] == (1 if engine == "stream" else 0), info
    if geo is not None:
        assert info["waves_per_sim"] == geo[0] and info["pool_bytes"] == 8 * BOUNDARIES[geo]["pool"], info
    Nmax = max(horizons)
    assert out["du0_dx"].shape == (len(sims), 6, 12) and out["du0_dyref"].shape == (len(sims), Nmax, 5, 6)
    assert out["du0_dw"].shape == (len(sims), 7, 6)
    try:
        for i, N in enumerate(sims):
            # (rows of du0_dyref past the simulation's own horizon are exactly zero: checked inside)
            tc.check_step(N, tc.MODES[i % 2], prev[i], out, i, tag, _MEASURED)
            if i % 2:
                assert np.abs(out["u_pred"][i][:N] - out["u_pred"][i - 1][:N]).max() > 1e-6      # (the two modes are two steps)
    finally:
        _dump()


@pytest.mark.parametrize("engine", ["latency", "stream"])
def test_the_plain_pass_sees_the_same_iterate_bit_for_bit(monkeypatch, engine):
    """sens=True alone at the stage-varying iterate: du0_dx and du0_dyref of a controller that never asked for du0_dw are those of
    the one that did, bit for bit, and are held to dense themselves."""
    _clean(monkeypatch)
    _, _, a = _run(engine, (20,), engine, sens_w=True)
    sims, prev, b = _run(engine, (20,), engine + "-plain", sens=True)
    assert "du0_dw" not in b
    for k in ("u0", "x_pred", "u_pred", "du0_dx", "du0_dyref", "sens_valid", "qp_iter", "status"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for i, N in enumerate(sims):
        tc.check_step(N, tc.MODES[i % 2], prev[i], b, i, engine + "-plain")
