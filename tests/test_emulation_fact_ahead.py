"""MPCB_FACT_AHEAD (csrc/mpc_core.h fact_pass_t): the factorisation sweep's recursion wavefront reads the operands of phase CA that
do not depend on phase B -- the lane's two columns of S~ and the linearisation of the stage -- during phase B and carries them across
the wave fence, the address of its K / R~^-1 column is complete before the stage loop, and phase CA reads K first.  Reads move, no
operation changes, so the host emulation built with the switch on (the default) and off must agree BIT FOR BIT:
  N = 1 and N = 2     the ahead-read of Gamma_u at stage 0 (no stage below: the address is clamped), and a stage below the terminal
                      one that is also stage 0
  N = 12              one window
  N = 15, small pool  chunks of about three stages, so five or six windows: the first stage of a window reads ahead into the
                      halo row of its input buffer
  N = 100             the LDS-resident factor (MODE 1) over several windows at the default pool
  N = 130             segments (MODE 2)
  tight bounds        the interior-point loop: Gamma != 0, several factorisations per step
  terminal cost       the TERM instantiation (the rollout with a joint-wise terminal cost)"""
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emu"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

KEYS = ("z", "u", "ee_pose", "ee_rpy", "ee_vel", "errors", "cost", "residuals", "status", "sqp_iter", "qp_iter")
TIGHT = dict(qdot_min=[-0.8] * 6, qdot_max=[0.8] * 6, qdot_0=[0.5, 0.7, 0.5, 0.0, 0.0, 0.0])   # test_gpu_fact_pipe._cfgs, simulation 1
OFF = "-DMPCB_FACT_AHEAD=0"


def _cfg(**kw):
    from robotic_mpc_amd import config

    kw.setdefault("solver_options", {"nlp_solver_type": "SQP_RTI"})
    return config.resolve_config(config.base_params(**kw))


def _cases():
    return {
        "n1_w1": ([_cfg(prediction_horizon=1, simulation_time=0.05)], dict(waves=1)),
        "n2_w4": ([_cfg(prediction_horizon=2, simulation_time=0.05)], dict(waves=4)),
        "n12_one_window_w4": ([_cfg(prediction_horizon=12, simulation_time=0.05)], dict(waves=4)),
        "n15_seams_w2": ([_cfg(prediction_horizon=15, simulation_time=0.05)], dict(waves=2, pool_doubles=2048)),
        "n100_resident_w4": ([_cfg(prediction_horizon=100, simulation_time=0.03)], dict(waves=4)),
        "n130_segments_w4": ([_cfg(prediction_horizon=130, simulation_time=0.03)], dict(waves=4)),
        "tight_bounds": ([_cfg(prediction_horizon=15, simulation_time=0.05, qp_fast_path=False, **TIGHT)], dict(waves=4)),
    }


EXPECTED_SWEEP = {"n100_resident_w4": "resident", "n130_segments_w4": "segment"}


def _term_inputs():
    import test_emulation_rollout_term as tt

    return tt._inputs(20, 4, True, True)


def _term_run(ur10):
    import emu_rollterm
    import term_rollout_cases as trc

    cfgs, sched, pert, blocks, x_ref = _term_inputs()
    return emu_rollterm.rollout(cfgs, ur10, sched, trc.flat18(blocks), x_ref, **pert, waves=4)


# the child process of the fixture: emu picks its variant from MPC_EMU_DEFINES when it is imported; the terminal-cost harness has one
# library name, so its variant is compiled here, by the loader's own command plus the switch, and loaded in its place
CHILD = r"""
import os, pickle, subprocess, sys
import numpy as np
here, root, job = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path[:0] = [here, os.path.join(here, "emu"), root]
import emu, emu_rollterm
jobs, chain, off, term_lib = pickle.load(open(job, "rb"))
for cfgs, kw, dst in jobs.values():
    np.savez(dst, **emu.run(cfgs, chain, **kw))
subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-O2", "-fPIC", "-shared", "-ffp-contract=off", off,
                       "-o", term_lib, os.path.join(here, "emu", "emu_rollterm_harness.cpp")])
emu_rollterm._LIB = term_lib
import test_emulation_fact_ahead as me
np.savez(os.path.join(os.path.dirname(job), "term.npz"), **me._term_run(chain))
"""


@pytest.fixture(scope="module")
def noahead_outputs(ur10, tmp_path_factory):
    """Every case once through the harnesses built with -DMPCB_FACT_AHEAD=0."""
    d = tmp_path_factory.mktemp("noahead")
    job = str(d / "job.pkl")
    pickle.dump(({n: (c, kw, str(d / (n + ".npz"))) for n, (c, kw) in _cases().items()}, ur10, OFF, str(d / "libmpc_emu_rollterm_noahead.so")),
                open(job, "wb"))
    subprocess.check_call([sys.executable, "-c", CHILD, HERE, os.path.dirname(HERE), job], env=dict(os.environ, MPC_EMU_DEFINES=OFF))
    out = {n: dict(np.load(str(d / (n + ".npz")))) for n in _cases()}
    out["term"] = dict(np.load(str(d / "term.npz")))
    return out


@pytest.mark.parametrize("name", list(_cases()))
def test_emulated_fact_ahead_equals_reads_in_place(ur10, noahead_outputs, name):
    import emu

    cfgs, kw = _cases()[name]
    if name in EXPECTED_SWEEP:   # the case does reach the MODE it is here for
        assert emu.emu_paths(cfgs[0]["N"], kw.get("pool_doubles") or emu.pool_doubles(1), kw["waves"])["sweep"] == EXPECTED_SWEEP[name]
    out = emu.run(cfgs, ur10, **kw)
    assert (out["status"] == 0).all()
    if name == "tight_bounds":
        assert (out["qp_iter"] > 1).all()       # several factorisations per step
    ref = noahead_outputs[name]
    for k in KEYS:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=f"{name} {k}")


def test_emulated_fact_ahead_equals_reads_in_place_with_a_terminal_cost(ur10, noahead_outputs):
    out = _term_run(ur10)
    assert (out["status"] == 0).all()
    ref = noahead_outputs["term"]
    for k in KEYS:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=f"terminal cost {k}")
