"""The conditions on the trajectory cases of tests/sens_traj_cases.py, each from the dense reference alone (no engine): validity,
discrimination, conditioning, the rounding share, the block count of sens_pass at N = 130, the shift against warm_checks.shift_iterate, and the
committed oracle-vs-dense distances re-measured.  A later edit of a case cannot quietly void what the emulation and the device
tests rely on.

Measured: every QP of every case clears every bound by more than 2.5 (wanted: 0.05).  With the linearisation point rolled by one
stage du0_dyref moves by at least 4.0e8 bounds, du0_dx by 2.8e9 and the least row of du0_dw by 1.4e9; at the flat guess by at
least 1.6e9, 1.1e11 and 1.5e10 (wanted: 100; du0_dx needs no exemption).  One ulp of the iterate moves du0_dx | du0_dyref by at
most 0.17 of the bound and a row of du0_dw by at most 0.24; one ulp of 1 in the task residuals by at most 0.15 and 0.25 (wanted:
a quarter).  With the packed alignment target 1, or one 0.03 below it, the w_task[1] row of du0_dw fails the last condition at
most horizons (0.4 .. 1.5 of its bound): tests/sens_traj_cases.py reference()."""
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "emu"))
sys.path.insert(0, HERE)

import dense_qp as dq  # noqa: E402
import dense_qp_cases as dc  # noqa: E402
import sens_checks as sc  # noqa: E402
import sens_traj_cases as tc  # noqa: E402
import sensw_checks as sw  # noqa: E402
from test_boundaries import BOUNDARIES  # noqa: E402

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc needed to build the emulation harness")


def test_the_table_has_every_case_and_every_step():
    assert sorted(tc.TRAJ_ORACLE_VS_DENSE) == sorted(tc.cid(N) for N in tc.HORIZONS)
    assert all(len(v) == tc.W + 2 for v in tc.TRAJ_ORACLE_VS_DENSE.values())
    assert [s[0] for s in tc.steps_of(2)] == ["step%d" % j for j in range(tc.W)] + list(tc.MODES)
    assert max(tc.tolerance(N, s[0]) for N in (2, 141) for s in tc.steps_of(N)) <= 1e-9          # the project's parity bar


def test_the_reference_is_curved_and_advances_one_stage_per_step():
    c = tc.case(20)
    y0, y1 = tc.reference(c["cfg"], 20, 0), tc.reference(c["cfg"], 20, 1)
    np.testing.assert_array_equal(y0[1:], y1[:-1])
    for col in (3, 4):
        assert np.abs(np.diff(y0[:, col], 2)).max() > 1e-4          # neither constant nor linear in the stage


@pytest.mark.parametrize("N", (2, 20, 43))
def test_the_shift_is_the_one_of_warm_checks(orc, N):
    import warm_checks as wc

    c, r = tc.case(N), tc.rollout(N)
    X, U = r["X"][tc.W], r["U"][tc.W]
    Xs, Us = tc.shift_iterate(c["cfg"], X, U)
    Xo, Uo = wc.shift_iterate(orc, c["cfg"], X, U)
    np.testing.assert_array_equal(Us, Uo)
    np.testing.assert_array_equal(Xs[:N], Xo[:N])
    # the two discretisations (dense_qp.lti, orc.lti) differ in rounding: x_N to a few ulp of a joint angle
    np.testing.assert_allclose(Xs[N], Xo[N], atol=1e-14, rtol=0)
    assert np.abs(Xs - X).max() > 1e-4 and np.abs(Us - U).max() > 1e-4           # (and it moves the iterate)


def test_the_stage_cache_returns_the_bits_of_the_plain_evaluation():
    c, r = tc.case(7), tc.rollout(7)
    chain = dc.chain_of(c)
    for k in (0, 3, 6):
        for y in (None, r["yref"][1][k]):
            p = dq.stage_residual(chain, c["cfg"], r["X"][2][k], r["U"][2][k], y)
            with tc.stages_once():
                m = dq.stage_residual(chain, c["cfg"], r["X"][2][k], r["U"][2][k], y)
            np.testing.assert_array_equal(p[0], m[0])
            np.testing.assert_array_equal(p[1], m[1])
    assert dq.stage_residual is tc._plain_stage_residual


@pytest.mark.parametrize("N", tc.HORIZONS)
def test_validity_every_step_clears_every_bound(N):
    c = tc.case(N)
    worst = np.inf
    for label, X, U, xhat, y in tc.steps_of(N):
        with tc.stages_once():
            qp = dq.assemble(dc.chain_of(c), c["cfg"], X, U, xhat, y)
            worst = min(worst, tc.clearance(qp, dq.solve_equality(qp)))
    print(f"\n[sens-traj] {tc.cid(N)}: least clearance of a bound over {tc.W + 2} QPs = {worst:.3f}")
    assert worst >= tc.CLEARANCE
    # the iterate of the checked step is off the flat guess on every stage, and no two stages of it are alike
    r = tc.rollout(N)
    X0, U0 = dc.guess(c)
    assert np.abs(r["X"][tc.W] - X0)[1:].max(axis=1).min() > 1e-4 and np.abs(r["U"][tc.W] - U0).max(axis=1).min() > 1e-4
    assert len({r["X"][tc.W][k].tobytes() for k in range(N + 1)}) == N + 1


@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("N", tc.HORIZONS)
def test_discrimination_and_conditioning(N, mode):
    """A stage mix-up is not within the bound: the Jacobians of the point rolled by one stage and of the flat guess are at least 100
    bounds from the true ones, for du0_dx, du0_dyref and every live row of du0_dw; and every bound is below 1e-6 of max |J|
    (asserted inside sens_checks.bound / sensw_checks.bounds)."""
    ref, refw = tc.dense_reference(N, mode)
    e = tc.eps(N, mode)
    b, bw = sc.bound(ref, e), sw.bounds(refw, e)
    assert b <= sc.CONDITION * ref["scale"] and (bw <= sw.CONDITION * refw["scale"]).all()
    rows = tc.live_rows(N)
    for which in ("rolled", "flat"):
        o, ow = tc.dense_reference(N, mode, which)
        fx = np.abs(o["Jx"] - ref["Jx"]).max() / b
        fy = np.abs(o["Jy"] - ref["Jy"]).max() / b
        fw = (np.abs(ow["J"] - refw["J"]).max(axis=1) / bw)[rows]
        print(f"\n[sens-traj] {tc.cid(N)} {mode} {which}: in bounds, du0_dx moves by {fx:.1e}, du0_dyref by {fy:.1e}, the rows of "
              f"du0_dw by {fw.min():.1e} .. {fw.max():.1e}")
        assert fy >= tc.DISCRIMINATION and (fw >= tc.DISCRIMINATION).all() and fx >= tc.DISCRIMINATION, (fx, fy, fw)


@pytest.mark.parametrize("mode", tc.MODES)
@pytest.mark.parametrize("N", tc.HORIZONS)
def test_one_ulp_of_the_iterate_or_of_the_task_residuals_stays_within_a_quarter_of_every_bound(N, mode):
    """The bounds are a few ulp of a row (10 x the reference's own noise, or 10 x an oracle-vs-dense distance that is itself a few
    ulp at short horizons).  What a one-ulp move of the iterate, or one ulp of 1 in the task residuals g - yref, does to the dense
    Jacobians is the reference's own error and everybody's; a case where that fills the bound would test rounding luck, not the
    pass, and is replaced (sens_traj_cases.SEEDS)."""
    for residual in (False, True):
        f, fw = tc.ulp_floor(N, mode, residual=residual)
        print(f"\n[sens-traj] {tc.cid(N)} {mode}: one ulp of {'the task residuals' if residual else '(X, U)'} moves (du0_dx | du0_dyref) "
              f"by {f:.2f} of its bound, the rows of du0_dw by {np.array2string(fw, precision=2)}")
        assert f <= tc.ULP_SHARE and (fw <= tc.ULP_SHARE).all()


@pytest.mark.parametrize("N", (7, 20))
def test_the_weight_reference_agrees_with_central_differences_off_the_flat_guess(N):
    """Guards against a sign error of the reference at a stage-varying point (sensw_checks.central_differences): 1e-6 of the row."""
    c, r = tc.case(N), tc.rollout(N)
    X, U = tc.point(c, tc.SHIFTED, r["X"][tc.W], r["U"][tc.W])
    _, refw = tc.dense_reference(N, tc.SHIFTED)
    with tc.stages_once():
        cd = sw.central_differences(dc.chain_of(c), c["cfg"], X, U, r["xhat"][tc.W], r["yref"][tc.W])
    assert (np.abs(cd - refw["J"]).max(axis=1) <= sw.CD_AGREE * refw["scale"]).all()


@pytest.mark.parametrize("N", tc.HORIZONS)
def test_oracle_distances_stay_within_the_committed_ones(orc, N):
    d = [tc.oracle_distance(orc, N, s[0]) for s in tc.steps_of(N)]
    print(f"\n[sens-traj] {tc.cid(N)}: |oracle - dense| = " + ", ".join("%.2e" % v for v in d))
    assert all(v <= w for v, w in zip(d, tc.TRAJ_ORACLE_VS_DENSE[tc.cid(N)])), (d, tc.TRAJ_ORACLE_VS_DENSE[tc.cid(N)])


@needs_hipcc
def test_n130_gives_the_pass_more_than_one_block_at_every_non_resident_geometry():
    """The stage loop of Engine::sens_pass<true> walks blocks of CH stages (csrc/mpc_core.h); a wrong index at the step k0 += CH
    shows only where stages 1 .. N - 1 do not fit one block.  Resident geometries stage through the scratch of the resident map,
    whose size the emulation does not report: they are not counted on."""
    import emu

    non_resident = 0
    for (waves, spc), g in sorted(BOUNDARIES.items()):
        sweep = emu.emu_paths(130, g["pool"], waves)["sweep"]
        blocks = tc.sens_blocks(130, g["pool"], sweep)
        print(f"\n[sens-traj] w{waves}_s{spc} pool {g['pool']} {sweep}: blocks of sens_pass<true> at N = 130: {blocks}")
        if sweep != "resident":
            non_resident += 1
            assert blocks > 1, (waves, spc, blocks)
            assert tc.sens_blocks(20, g["pool"], "streaming") == 1
    assert non_resident == 6
