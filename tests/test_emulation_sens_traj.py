"""Host emulation of the latency engine's sensitivity pass (Engine::sens_pass<true> / sens_pass<false> inside
Engine::control_step<true, true, true>) at a linearisation point that differs on every stage: the trajectory cases of
tests/sens_traj_cases.py.  W carried warm-up steps under a curved reference that advances one stage per step, then the checked
step carried and shifted side by side in one batch of two; du0_dx, du0_dyref and du0_dw against the dense Jacobians at the engine's
own previous prediction, under the bound of the reset-step tests.

On the reset step of tests/test_emulation_sens.py / test_emulation_sensw.py every stage holds the same task Jacobians, [qdot | U]
run and residual, so only the indices of K_k and of the QP's step are visible there; here every index of the pass is.  With the
row of G2 read one stage off every reset-step test passes and every test here fails, du0_dyref by 1.3e-03 .. 5.2e-03 (2e9 .. 3e9
bounds) and the task rows of du0_dw by 2e10 .. 6e12 bounds; with the [qdot | U] run and the residual read one stage off the
reset-step tests pass on every case but N20-ramp and the rows of du0_dw here are off by 6e10 .. 6e13 bounds.

Runs: 1, 2, 4 and 8 wavefronts at N = 2, 7, 20; both sides of the sweep switches of tests/test_emulation_sens.py SWITCH; N = 130
at the pool of every launch geometry of tests/test_boundaries.py BOUNDARIES (more than one block of the pass wherever the gains are
not resident).  The throughput engine has no host build: tests/test_gpu_controller_sens_traj.py covers it on the device.

Measured (profiles/step_sens_traj_distances.txt): du0_dx | du0_dyref within 0.11 of the bound everywhere, every row of du0_dw within
0.59 of its bound (row 3 of N26-traj carried, register sweep).

SENS_DUMP=<file> collects the measured distances (profiles/step_sens_traj_distances.txt)."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dense_qp_cases as dc  # noqa: E402
import sens_traj_cases as tc  # noqa: E402
import warm_checks as wc  # noqa: E402
from test_boundaries import BOUNDARIES  # noqa: E402
from test_emulation_sens import POOL, SWITCH, WAVES  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

BASIC = [(N, w, POOL, "resident") for N in (2, 7, 20) for w in WAVES]
SWITCHES = [(int(cid[1:].split("-")[0]), w, pool, sweep) for cid, w, pool, sweep in SWITCH]
GEOMETRIES = [(130, w, BOUNDARIES[(w, s)]["pool"], [f for n, f in BOUNDARIES[(w, s)]["sweep"] if n <= 130][-1]) for w, s in sorted(BOUNDARIES)]
RUNS = BASIC + SWITCHES + GEOMETRIES

_MEASURED = {}


def _dump():
    if os.environ.get("SENS_DUMP"):
        tc.dump(os.environ["SENS_DUMP"], _MEASURED)


def _run(N, waves, pool, tag, **kw):
    """The W warm-up steps (checked against the dense QP at the engine's own iterate) and the checked step of a batch of two:
    simulation 0 carries, simulation 1 shifts.  Returns (the two previous predictions, the checked step's outputs)."""
    import emu_sensw

    c, r = tc.case(N), tc.rollout(N)
    ctl = emu_sensw.Controller([c["cfg"], c["cfg"]], dc.chain_of(c), pool_doubles=pool, waves=waves)
    prev = dc.guess(c)
    for j in range(tc.W):
        out = ctl.step(np.stack([r["xhat"][j]] * 2), yref=r["yref"][j][None], ref_changed=True, warm=[wc.CARRY, wc.CARRY], **kw)
        for k in ("x_pred", "u_pred", "u0", "du0_dx"):
            np.testing.assert_array_equal(out[k][0], out[k][1], err_msg=k)         # one history for both
        prev = tc.check_warmup(N, j, prev, out, 0, tag)
    out = ctl.step(np.stack([r["xhat"][tc.W]] * 2), yref=r["yref"][tc.W][None], ref_changed=True, warm=[wc.CARRY, wc.SHIFT], **kw)
    return prev, out


@pytest.mark.parametrize("N,waves,pool,sweep", RUNS, ids=["N%d-w%d-p%d-%s" % s for s in RUNS])
def test_checked_step_sensitivities_against_dense_at_a_stage_varying_iterate(N, waves, pool, sweep):
    import emu

    assert emu.emu_paths(N, pool, waves)["sweep"] == sweep
    if N == 130 and sweep != "resident":
        assert tc.sens_blocks(N, pool, sweep) > 1
    tag = "emu-w%d-p%d-%s" % (waves, pool, sweep)
    prev, out = _run(N, waves, pool, tag)
    assert np.abs(out["u_pred"][0] - out["u_pred"][1]).max() > 1e-6                # (the two modes are two steps)
    try:
        for i, mode in enumerate(tc.MODES):
            tc.check_step(N, mode, prev, out, i, tag, _MEASURED)
    finally:
        _dump()


@pytest.mark.parametrize("waves", (1, 4))
def test_the_plain_pass_sees_the_same_iterate_bit_for_bit(waves):
    """sens_pass<false> at the stage-varying iterate: du0_dx and du0_dyref of a controller that never asked for du0_dw are those of
    the one that did, bit for bit, and are held to dense themselves."""
    N = 20
    prev, a = _run(N, waves, POOL, "emu-w%d" % waves)
    prev_b, b = _run(N, waves, POOL, "emu-plain-w%d" % waves, sens_w=False)
    assert "du0_dw" not in b
    for k in ("u0", "x_pred", "u_pred", "du0_dx", "du0_dyref", "sens_valid", "qp_iter", "status"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    for i, mode in enumerate(tc.MODES):
        tc.check_step(N, mode, prev_b, b, i, "emu-plain-w%d" % waves)
