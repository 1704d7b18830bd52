"""Host emulation of the rollout with the joint-wise terminal cost (Engine<.., true>::rollout<true, true>, the device code behind
mpcb_rollout_term on the latency engine) against what defines it: the loop of test_emulation_rollout_pert.py whose step is the
emulated controller step WITH a terminal cost (Engine<.., true>::control_step), given the simulation's constant blocks and row t of
its table of terminal references at every step t.  Both sides run the same passes on the same data, so they agree to rounding of the
few operations that differ in order (1e-12): a larger distance is a wiring bug.

Before it compares, every test asserts from the reference loop alone that every step has status 0 and that the loop without the
terminal cost ends up more than 1e-4 away in z."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import term_rollout_cases as trc  # noqa: E402
import test_emulation_rollout_pert as tp  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

# the SQP_RTI cases of test_emulation_rollout_pert.py (one per sweep of the interior-point solve) with every perturbation on, and
# the first of them over the nominal plant
CASES = [c + (True,) for c in tp.CASES if c[2] == "SQP_RTI"] + [tp.CASES[0] + (False,)]
INTS = tp.INTS


def _loop(cfgs, chain, sched, pert, blocks, x_ref, pool, waves):
    """The yardstick: the emulated controller with the terminal cost (blocks, x_ref[:, t]) of step t -- or without one, blocks None --
    stepped from z + x_noise[t] over the perturbed plant step on the host."""
    import emu_rollterm

    steps, N, B = cfgs[0]["Nsim"], cfgs[0]["N"], len(cfgs)
    ctl = emu_rollterm.Controller(cfgs, chain, pool_doubles=pool, waves=waves)
    zt = np.stack([np.concatenate([c["q0"], c["qdot0"]]) for c in cfgs])
    o = dict(z=np.zeros((B, 12, steps + 1)), u=np.zeros((B, 6, steps + 1)), cost=np.zeros((B, steps)), residuals=np.zeros((B, steps, 4)),
             status=np.zeros((B, steps), np.int32), sqp_iter=np.zeros((B, steps), np.int32), qp_iter=np.zeros((B, steps), np.int32))
    o["z"][:, :, 0] = zt
    o["u"][:, :, 0] = np.stack([c["qdot0"] for c in cfgs])                 # u[:, 0] = qdot_0 (simulator.py:81)
    for t in range(steps):
        if blocks is not None:
            ctl.set_terminal(trc.records(blocks, x_ref[:, t]))
        out = ctl.step(zt + pert["x_noise"][:, t], yref=sched[:, t:t + N], ref_changed=True, predict=False)
        for k in ("cost", "residuals") + INTS:
            o[k][:, t] = out[k]
        zt = np.stack([emu_rollterm.plant_rk(c, pert["wcv"][i], zt[i], out["u0"][i] + pert["u_dist"][i, t]) for i, c in enumerate(cfgs)])
        o["z"][:, :, t + 1] = zt
        o["u"][:, :, t + 1] = out["u0"]
    return o


def _nominal(cfgs):
    B, S = len(cfgs), cfgs[0]["Nsim"]
    return {"wcv": np.stack([c["wcv"] for c in cfgs]), "u_dist": np.zeros((B, S, 6)), "x_noise": np.zeros((B, S, 12))}


def _inputs(N, steps, fast, perturbed):
    from robotic_mpc_amd import plant, reference

    cfgs = tp._cfgs(N, steps, "SQP_RTI", fast)
    sched = reference.stack(cfgs)
    pert = plant.stack(cfgs) if perturbed else _nominal(cfgs)
    return cfgs, sched, pert, trc.lqr_blocks(cfgs), trc.table(cfgs, N)


def test_cases_are_the_rti_cases_of_the_perturbed_rollout():
    assert [c[:6] for c in CASES[:-1]] == [c for c in tp.CASES if c[2] == "SQP_RTI"] and len(CASES) == 5
    assert all(c[6] for c in CASES[:-1]) and not CASES[-1][6]


@pytest.mark.parametrize("N,steps,solver,fast,pool,waves,perturbed", CASES)
def test_emulated_rollout_with_a_terminal_cost_is_the_loop_of_the_terminal_step(ur10, N, steps, solver, fast, pool, waves, perturbed):
    import emu_rollterm

    cfgs, sched, pert, blocks, x_ref = _inputs(N, steps, fast, perturbed)
    assert x_ref.shape == (2, steps, 12) and blocks.shape == (2, 6, 3) and blocks[:, :, 0].min() > 100
    assert np.abs(x_ref[:, 1] - x_ref[:, 0]).min() > 0                        # the table moves
    want = _loop(cfgs, ur10, sched, pert, blocks, x_ref, pool, waves)
    assert (want["status"] == 0).all()
    without = _loop(cfgs, ur10, sched, pert, None, None, pool, waves)
    assert np.abs(without["z"] - want["z"]).max() > 1e-4
    got = emu_rollterm.rollout(cfgs, ur10, sched, trc.flat18(blocks), x_ref, **(pert if perturbed else {}), pool_doubles=pool, waves=waves)
    tp._compare(got, want, cfgs, sched)


def test_emulated_rollout_reads_the_row_of_its_step(ur10):
    """Table against constant: the loop that holds row 0 for every step ends up elsewhere, and the rollout is the table's loop."""
    import emu_rollterm

    cfgs, sched, pert, blocks, x_ref = _inputs(20, 7, True, True)
    want = _loop(cfgs, ur10, sched, pert, blocks, x_ref, 0, 4)
    held = _loop(cfgs, ur10, sched, pert, blocks, np.repeat(x_ref[:, :1], 7, axis=1), 0, 4)
    assert (want["status"] == 0).all() and np.abs(held["z"] - want["z"]).max() > 1e-4
    got = emu_rollterm.rollout(cfgs, ur10, sched, trc.flat18(blocks), x_ref, **pert, waves=4)
    tp._compare(got, want, cfgs, sched)


def test_emulated_rollout_does_not_depend_on_the_launch_boundary(ur10):
    import emu_rollterm

    cfgs, sched, pert, blocks, x_ref = _inputs(20, 7, True, True)
    assert np.abs(x_ref[:, 2] - x_ref[:, 3]).min() > 0                        # the rows around the boundary differ
    a = emu_rollterm.rollout(cfgs, ur10, sched, trc.flat18(blocks), x_ref, **pert, waves=4)
    b = emu_rollterm.rollout(cfgs, ur10, sched, trc.flat18(blocks), x_ref, **pert, step_chunk=3, waves=4)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_emulated_rollout_with_zero_blocks_is_the_perturbed_rollout(ur10):
    import emu_rollpert
    import emu_rollterm

    cfgs, sched, pert, _, x_ref = _inputs(20, 7, True, True)
    want = emu_rollpert.rollout(cfgs, ur10, sched, **pert, waves=4)
    got = emu_rollterm.rollout(cfgs, ur10, sched, np.zeros((2, 18)), x_ref, **pert, waves=4)
    for k in ("z", "u", "ee_pose", "ee_rpy", "ee_vel", "errors", "cost", "residuals"):
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-12, err_msg=k)
    for k in INTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
