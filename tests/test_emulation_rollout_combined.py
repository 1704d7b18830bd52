"""Host emulation of the combined rollout (Engine<.., TERM_TABLE, DIST_SHARED, 1>::rollout<true, true, true, true>, the device code
behind mpcb_rollout_combined on the latency engine) against what defines it: the loop of the emulated COMBINED controller step
(Engine<.., 1, 1, 1>::control_step<true>, tests/emu/emu_combined.py step_loop) with the window, the surface window, the terminal
record [blocks | x_ref[t]] and the observer's estimate d^_t of every step, shifted from step 1 on where the mode says so, over the
perturbed plant on the host.  Both sides run the same passes on the same data: they agree to 1e-12, the emulation tier's bound, on
every log and on d_hat.  A larger distance is a wiring bug -- the order of the observer publication and the shift among them.

Every batch mixes subsets (combined_cases.SUBSETS: all four, none, each alone, pairs) but has ONE horizon: the latency engine, which is
what the host executor runs, takes one horizon per launch (ragged batches exist on the throughput engine alone, which has no
emulation), so mixed horizons are covered on the device only -- tests/test_gpu_rollout_combined.py, N in {1, 2, 7, 12} in one launch.  Before it compares, every test asserts from
the reference loops alone that every step has status 0 and that for each feature a simulation with N >= 2 uses, the loop without it
ends more than 1e-4 away in z.  With N = 2 the surface table reaches u0 through stage 1 alone and its distance is about 1e-4: seed 6
(test_gpu_rollout_shift.py's) gives 8.1e-5 over 10 steps and 9.9e-5 over 14 and was skipped, as were 17, 36 and 46 (7.1e-5 .. 7.9e-5);
seed 16 over 14 steps gives 1.1e-4."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

import combined_cases as cc  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

INTS = ("status", "sqp_iter", "qp_iter")
_CACHE = {}


def _inputs(ur10, n, N, steps, seed, waves, pool=0, subsets=cc.SUBSETS):
    """(cfgs, tables, the reference loop, the loops with one feature off): computed once per case, shared, never written to."""
    import emu_combined
    from robotic_mpc_amd import engine

    key = (n, N, steps, seed, waves, pool, subsets)
    if key not in _CACHE:
        cfgs = cc.resolve(cc.raw(n, N, steps, seed, subsets=subsets))
        tabs = engine.combined_arrays(cfgs)
        want = emu_combined.step_loop(cfgs, ur10, tabs, pool=pool, waves=waves)
        used = {f for c in cfgs for f in cc.uses(c)}
        without = {f: emu_combined.step_loop(cfgs, ur10, tabs, pool=pool, waves=waves, off=(f,)) for f in cc.FEATURES if f in used}
        _CACHE[key] = (cfgs, tabs, want, without)
    return _CACHE[key]


def _compare(got, want):
    for k in ("z", "u", "d_hat"):
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-12, err_msg=k)
    np.testing.assert_allclose(got["cost"], want["cost"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["residuals"], want["residuals"], rtol=0, atol=1e-12)
    for k in INTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("n,N,steps,seed,waves,pool", [(8, 12, 14, 1, 4, 0), (4, 2, 14, 16, 2, 0), (4, 1, 10, 21, 1, 0), (4, 12, 8, 3, 8, 2048)],
                         ids=["N12-every-subset", "N2", "N1", "N12-small-pool"])
def test_emulated_combined_rollout_is_the_loop_of_the_combined_step(ur10, n, N, steps, seed, waves, pool):
    import emu_combined

    cfgs, tabs, want, without = _inputs(ur10, n, N, steps, seed, waves, pool)
    cc.guards(cfgs, want, without)
    got = emu_combined.rollout(cfgs, ur10, tabs, pool_doubles=pool, waves=waves)
    _compare(got, want)
    assert (got["d_hat"][:, 0] == 0).all()
    for i, c in enumerate(cfgs):                      # the estimate leaves zero exactly where there is an observer
        assert (np.abs(got["d_hat"][i, -1]).max() > 1e-3) == ("obs" in cc.uses(c)), i
        # ... and where it meets the shift it moves from step to step, so the order of publication and shift shows in the tail
        if "obs" in cc.uses(c) and "shift" in cc.uses(c):
            assert np.abs(np.diff(want["d_hat"][i], axis=0)).max() > 1e-3, i


def test_launch_boundaries_change_nothing(ur10):
    """[0, 5, 9, 14]: ST_OBS, the shift, row t of the terminal table and window t of the surface table all cross a boundary -- bit
    for bit the single launch."""
    import emu_combined

    cfgs, tabs, _, _ = _inputs(ur10, 8, 12, 14, 1, 4)
    one = emu_combined.rollout(cfgs, ur10, tabs, waves=4)
    cut = emu_combined.rollout(cfgs, ur10, tabs, waves=4, bounds=[0, 5, 9, 14])
    for k in one:
        if k not in ("solver_time", "plant_time"):
            np.testing.assert_array_equal(one[k], cut[k], err_msg=k)


def test_all_neutral_is_the_perturbed_rollout(ur10):
    """No simulation uses a feature: the combined kernels' code on neutral tables gives the perturbed rollout's logs."""
    import emu_combined
    import emu_rollpert
    from robotic_mpc_amd import engine

    cfgs = cc.resolve(cc.raw(2, 12, 8, seed=5, subsets=((),)))
    tabs = engine.combined_arrays(cfgs)
    got = emu_combined.rollout(cfgs, ur10, tabs, waves=4)
    want = emu_rollpert.rollout(cfgs, ur10, tabs["yref"], **tabs["pert"], waves=4)
    assert (got["d_hat"] == 0).all()
    for k in ("z", "u", "ee_pose", "ee_rpy", "ee_vel", "errors", "cost", "residuals"):
        np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-12, err_msg=k)
    for k in INTS:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
