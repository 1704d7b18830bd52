"""MPCB_FACT_AHEAD on the device (csrc/mpc_core.h fact_pass_t; tests/test_emulation_fact_ahead.py has the host side): the default
library and a build with -DMPCB_FACT_AHEAD=0 run the same small rollouts, and every result array except the timings must agree BIT
FOR BIT -- the switch moves LDS reads in the instruction stream, it changes no operation.  Once per launch geometry that
tests/test_gpu_fact_pipe.py lists, and once through the default choice; horizons: N = 1 (stage 0 is the only stage: the clamped
ahead-read), N = 12 (one window), N = 100 (the LDS-resident factor over several windows) and N = 130 (segments, fact_pass_t<2>)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_gpu_fact_pipe import GEOMETRIES, TIMING, _cfgs  # noqa: E402

pytestmark = pytest.mark.gpu

RUNS = ((1, 0.03, 3), (12, 0.2, 20), (100, 0.05, 5), (130, 0.02, 2))   # N, simulation time, MPC steps it makes


@pytest.fixture(scope="module")
def noahead_lib():
    from robotic_mpc_amd import build

    return build.build_variant("noahead", ["MPCB_FACT_AHEAD=0"])


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "default" if g is None else "w%d_s%d" % g)
def test_fact_ahead_is_bit_identical_on_the_device(ur10, noahead_lib, monkeypatch, geom):
    from robotic_mpc_amd import engine

    if geom is not None:
        monkeypatch.setenv("MPCB_WAVES_PER_SIM", str(geom[0]))
        monkeypatch.setenv("MPCB_SIMS_PER_CU", str(geom[1]))
    for N, T, steps in RUNS:
        cfgs = _cfgs(N, T)
        outs = []
        for lib in (None, noahead_lib):
            e = engine.MpcBatchEngine(0, lib_path=lib)
            try:
                outs.append(e.run(cfgs, ur10))
                if geom is not None:
                    assert e.launch_info()["waves_per_sim"] == geom[0]
            finally:
                e.close()
        ahead, ref = outs
        assert ahead["status"].shape == (4, steps)
        if N >= 12:                                # (with one stage the fast path solves the tight-bound simulation's QPs outright)
            assert (ref["qp_iter"][1] > 1).any()   # the tight-bound simulation went through the interior-point loop
        for k in ref:
            if k not in TIMING:
                np.testing.assert_array_equal(ahead[k], ref[k], err_msg=f"N={N} {k}")
