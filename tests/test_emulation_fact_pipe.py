"""MPCB_FACT_PIPE (csrc/mpc_core.h fact_pass_t): the factorisation sweep's recursion wavefront eliminates its right-hand sides inside
the LDL' loop, in every lane, and stores K / R~^-1 through one per-lane address.  Only the position of the operations and the lanes
that execute them change, so the host emulation built with the switch on (the default) and off must agree BIT FOR BIT:
on a single chunk, across chunk seams, with the LDS-resident factor (MODE 1), with segments (MODE 2) and when the interior-point
loop factorises several times per step."""
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")

KEYS = ("z", "u", "ee_pose", "ee_rpy", "ee_vel", "errors", "cost", "residuals", "status", "sqp_iter", "qp_iter")
TIGHT = dict(qdot_min=[-0.8] * 6, qdot_max=[0.8] * 6, qdot_0=[0.5, 0.7, 0.5, 0.0, 0.0, 0.0])   # tests/golden/make_golden.py rti_tight_bounds


def _cfg(**kw):
    from robotic_mpc_amd import config

    kw.setdefault("solver_options", {"nlp_solver_type": "SQP_RTI"})
    return config.resolve_config(config.base_params(**kw))


def _cases():
    return {
        "n3_w1": ([_cfg(prediction_horizon=3, simulation_time=0.05)], dict(waves=1)),
        "n15_seams_w2": ([_cfg(prediction_horizon=15, simulation_time=0.05)], dict(waves=2, pool_doubles=2048)),
        "n30_resident_w4": ([_cfg(prediction_horizon=30, simulation_time=0.05)], dict(waves=4)),
        "n130_segments_w4": ([_cfg(prediction_horizon=130, simulation_time=0.03)], dict(waves=4)),
        "tight_bounds": ([_cfg(prediction_horizon=15, simulation_time=0.05, qp_fast_path=False, **TIGHT)], dict(waves=4)),
    }


EXPECTED_SWEEP = {"n30_resident_w4": "resident", "n130_segments_w4": "segment"}


@pytest.fixture(scope="module")
def nopipe_outputs(ur10, tmp_path_factory):
    """Every case once through the harness built with -DMPCB_FACT_PIPE=0 (a child process: the variant is chosen when emu is imported)."""
    d = tmp_path_factory.mktemp("nopipe")
    job = str(d / "job.pkl")
    pickle.dump(({n: (c, kw, str(d / (n + ".npz"))) for n, (c, kw) in _cases().items()}, ur10), open(job, "wb"))
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import emu, pickle; "
            "jobs, chain = pickle.load(open(sys.argv[1], 'rb'))\n"
            "for cfgs, kw, dst in jobs.values(): np.savez(dst, **emu.run(cfgs, chain, **kw))"
            % (os.path.join(HERE, "emu"), os.path.dirname(HERE)))
    subprocess.check_call([sys.executable, "-c", code, job], env=dict(os.environ, MPC_EMU_DEFINES="-DMPCB_FACT_PIPE=0"))
    return {n: dict(np.load(str(d / (n + ".npz")))) for n in _cases()}


@pytest.mark.parametrize("name", list(_cases()))
def test_emulated_fact_pipe_equals_separate_phases(ur10, nopipe_outputs, name):
    import emu

    cfgs, kw = _cases()[name]
    if name in EXPECTED_SWEEP:   # the case does reach the MODE it is here for
        assert emu.emu_paths(cfgs[0]["N"], kw.get("pool_doubles") or emu.pool_doubles(1), kw["waves"])["sweep"] == EXPECTED_SWEEP[name]
    out = emu.run(cfgs, ur10, **kw)
    if name == "tight_bounds":
        assert (out["qp_iter"] > 1).all()       # several factorisations per step
    ref = nopipe_outputs[name]
    for k in KEYS:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=f"{name} {k}")
