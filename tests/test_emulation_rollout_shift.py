"""Host emulation of the rollout with the shift warm start (Engine<.., 0, 0, SURF>::rollout<true, true, false, true>, the device code
behind mpcb_rollout_warm on the latency engine) against what defines it: the loop of test_emulation_rollout_pert.py whose step is
the emulated controller step WITH a warm-start mode per simulation (tests/emu/emu_warm.Controller; with a surface table,
emu_surf.Controller), given CARRY at step 0 and the simulation's mode from step 1 on.  Both sides run the same passes on the same
data: they agree to 1e-12, the emulation tier's bound, on every log, with the ints equal.  A larger distance is a wiring bug.

The four SQP_RTI cases of test_emulation_rollout_pert.CASES (one per sweep of the interior-point solve; the pool of 2048 doubles
makes shift_group move the records in several blocks), and the horizons 1 and 2.  Before it compares, every test asserts from the
reference loops alone that every step has status 0, that for N >= 2 the all-carry loop ends more than 1e-4 away in z from the
shifted one, and that for N = 1 the two agree exactly (the shift moves nothing the step reads: the only input stays, x_0 is
replaced by the feedback state and x_1 is formed from them)."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import test_emulation_rollout_pert as tp  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

RTI_CASES = [c for c in tp.CASES if c[2] == "SQP_RTI"]
SHORT = [(1, 10, "SQP_RTI", True, 0, 4), (2, 10, "SQP_RTI", True, 0, 4)]
INTS = tp.INTS
CARRY, SHIFT = 0, 2

_CACHE = {}


def _inputs(ur10, case):
    """(cfgs, sched, pert, the all-carry loop, the all-shift loop) of a case: computed once, shared, never written to."""
    import emu_rollshift
    from robotic_mpc_amd import plant, reference

    if case not in _CACHE:
        N, steps, solver, fast, pool, waves = case
        cfgs = tp._cfgs(N, steps, solver, fast)
        sched, pert = reference.stack(cfgs), plant.stack(cfgs)
        loops = {m: emu_rollshift.step_loop(cfgs, ur10, sched, pert, m, pool=pool, waves=waves) for m in (CARRY, SHIFT)}
        _CACHE[case] = (cfgs, sched, pert, loops[CARRY], loops[SHIFT])
    return _CACHE[case]


def _guards(N, carry, shift, sims=(0, 1)):
    assert (carry["status"] == 0).all() and (shift["status"] == 0).all()
    for i in sims:
        d = np.abs(carry["z"][i] - shift["z"][i]).max()
        print(f"N = {N}, simulation {i}: max |dz| carry against shift = {d:.3e}")
        if N >= 2:
            assert d > 1e-4, (i, d)
        else:
            np.testing.assert_array_equal(carry["z"][i], shift["z"][i])


def _pick(o, i):
    return {k: v[i:i + 1] for k, v in o.items()}


def test_the_modes_are_those_of_the_header():
    import emu_rollshift
    from robotic_mpc_amd import engine

    assert (emu_rollshift.CARRY, emu_rollshift.SHIFT) == (engine.WARM_CARRY, engine.WARM_SHIFT) == (CARRY, SHIFT)
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mpcbatch.h")).read()
    assert "#define MPCB_WARM_CARRY 0" in hdr and "#define MPCB_WARM_SHIFT 2" in hdr


@pytest.mark.parametrize("case", RTI_CASES + SHORT, ids=lambda c: f"N{c[0]}-pool{c[4]}-w{c[5]}")
def test_emulated_shifted_rollout_is_the_loop_of_the_warm_step(ur10, case):
    import emu_rollshift

    N, steps, _, _, pool, waves = case
    cfgs, sched, pert, carry, shift = _inputs(ur10, case)
    _guards(N, carry, shift)
    if pool == 2048:
        assert pool // 96 < N        # a block holds pool / W1 destination stages (mpc_layout.h W1 = 96): 21 of 23, two blocks
    got = emu_rollshift.rollout(cfgs, ur10, sched, SHIFT, **pert, pool_doubles=pool, waves=waves)
    tp._compare(got, shift, cfgs, sched)


def test_mixed_batch_matches_each_simulations_own_loop(ur10):
    """Simulation 0 carries, simulation 1 shifts: one launch, each against its own loop."""
    import emu_rollshift

    case = RTI_CASES[0]
    N, steps, _, _, pool, waves = case
    cfgs, sched, pert, carry, shift = _inputs(ur10, case)
    _guards(N, carry, shift, sims=(1,))
    got = emu_rollshift.rollout(cfgs, ur10, sched, [CARRY, SHIFT], **pert, pool_doubles=pool, waves=waves)
    tp._compare(_pick(got, 0), _pick(carry, 0), cfgs[:1], sched[:1])
    tp._compare(_pick(got, 1), _pick(shift, 1), cfgs[1:], sched[1:])
    # any value other than SHIFT carries
    other = emu_rollshift.rollout(cfgs, ur10, sched, [7, SHIFT], **pert, pool_doubles=pool, waves=waves)
    for k in got:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(other[k], got[k], err_msg=k)


def test_shifted_rollout_does_not_depend_on_the_launch_boundary(ur10):
    """Chunks of 3 steps: the first step of a later launch shifts, the run's first step does not -- bit for bit one launch."""
    import emu_rollshift

    case = RTI_CASES[0]
    N, steps, _, _, pool, waves = case
    cfgs, sched, pert, carry, shift = _inputs(ur10, case)
    _guards(N, carry, shift)
    a = emu_rollshift.rollout(cfgs, ur10, sched, SHIFT, **pert, pool_doubles=pool, waves=waves)
    b = emu_rollshift.rollout(cfgs, ur10, sched, SHIFT, **pert, pool_doubles=pool, waves=waves, step_chunk=3)
    for k in a:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_no_modes_is_the_perturbed_rollout(ur10):
    import emu_rollpert
    import emu_rollshift

    case = RTI_CASES[0]
    N, steps, _, _, pool, waves = case
    cfgs, sched, pert, carry, shift = _inputs(ur10, case)
    got = emu_rollshift.rollout(cfgs, ur10, sched, None, **pert, pool_doubles=pool, waves=waves)
    want = emu_rollpert.rollout(cfgs, ur10, sched, **pert, pool_doubles=pool, waves=waves)
    for k in want:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    # ... and all-carry through the SHIFT instantiation runs the same passes on the same data
    allc = emu_rollshift.rollout(cfgs, ur10, sched, CARRY, **pert, pool_doubles=pool, waves=waves)
    for k in want:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(allc[k], want[k], err_msg=k)


def test_shifted_rollout_over_a_surface_table_is_the_loop_of_the_surface_step(ur10):
    """One case with a surface table: the yardstick's step is the emulated step with a surface window (emu_surf)."""
    import emu_rollshift
    import test_emulation_rollout_surf as ts
    from robotic_mpc_amd import plant, reference, surface

    cfgs = ts._cfgs()[:2]
    sched, pert, surf = reference.stack(cfgs), plant.stack(cfgs), surface.stack(cfgs)
    carry = emu_rollshift.step_loop(cfgs, ur10, sched, pert, CARRY, surf=surf, waves=4)
    shift = emu_rollshift.step_loop(cfgs, ur10, sched, pert, [SHIFT, CARRY], surf=surf, waves=4)
    _guards(ts.N, carry, shift, sims=(0,))
    np.testing.assert_array_equal(carry["z"][1], shift["z"][1])
    got = emu_rollshift.rollout(cfgs, ur10, sched, [SHIFT, CARRY], surf=surf, **pert, waves=4)
    # (test_emulation_rollout_surf._compare is written for its own batch of four)
    from robotic_mpc_amd import analysis

    np.testing.assert_allclose(got["cost"], shift["cost"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["residuals"], shift["residuals"], rtol=0, atol=1e-12)
    for k in INTS:
        np.testing.assert_array_equal(got[k], shift[k], err_msg=k)
    np.testing.assert_allclose(got["z"], shift["z"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got["u"], shift["u"], rtol=0, atol=1e-12)
    for i, c in enumerate(cfgs):
        e = analysis.errors_rows(analysis.compute_errors(got["ee_pose"][i], got["ee_vel"][i], surf[i, :ts.STEPS + 1].T, c["t_ee"],
                                                         c["px_ref"], c["vy_ref"], yref=sched[i, :ts.STEPS + 1]))
        np.testing.assert_allclose(got["errors"][i], e, rtol=0, atol=1e-12)
