"""The closed loop of tests/step_dist_closed_loop.py on the emulated latency engine (CPU): offset-free tracking with the observer's
estimate in the prediction model.  This is where RHO_EMULATED, the figure the device test's bound derives from, is measured."""
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)

import dense_qp_cases as dc  # noqa: E402
import step_dist_closed_loop as cl  # noqa: E402

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")


def emulated_step():
    import emu_dist
    import torch

    from robotic_mpc_amd import config

    cfg = config.resolve_config(cl.raw_config())
    ctl = emu_dist.Controller([cfg] * cl.B, dc.chain_of(dict(cfg=cfg)), pool_doubles=19392, waves=4)

    def step(x, d_hat):
        kw = {} if d_hat is None else dict(dist=d_hat.numpy())
        out = ctl.step(x.numpy(), **kw)
        assert (out["status"] == 0).all()
        return torch.from_numpy(out["u0"].copy()), torch.from_numpy(out["x_pred"][:, 1].copy())
    return step


@needs_hipcc
def test_emulated_closed_loop_is_offset_free():
    K, nom, unc, comp, d = cl.three_runs(emulated_step)
    f = cl.figures(K, nom, unc, comp, d)
    print(f"\n[dist] closed loop, emulated: K = {K}, {f}")
    assert f["d_err"] <= 1e-7
    assert f["pred_comp"] <= 1e-9
    # the uncompensated prediction misses the next state by |Bd d| in every step: >= b2 min_i max_j |d_ij| / 2
    assert f["pred_unc"] >= 0.4 * np.abs(d).max(axis=1).min()
    assert cl.RHO == 10.0 * cl.RHO_EMULATED
    # the committed figure is this measurement (to its two printed digits)
    assert 0.9 * cl.RHO_EMULATED <= f["ratio"] <= 1.1 * cl.RHO_EMULATED, f["ratio"]
