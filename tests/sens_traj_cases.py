"""The trajectory cases of the sensitivity tests (tests/test_sens_traj_cases.py and tests/test_emulation_sens_traj.py on the CPU,
tests/test_gpu_controller_sens_traj.py on the device): du0_dx, du0_dyref and du0_dw of a step whose linearisation point differs on
every stage.

On a reset step the iterate is the flat guess of dense_qp_cases.guess: the task Jacobians, the [qdot | U] run and (without a
per-stage reference) the task residual are the same on every stage, so a pass that read them from the wrong stage would return
the same bits.  A trajectory case gets off the flat guess with W carried RTI steps under a CURVED per-stage reference that
advances one stage per step, on a plant that is not the model (dense_qp_cases.chained_distances: the exact discretisation at
80 % of the bandwidths plus a seeded +-1e-3 perturbation), and checks step W in both modes: carried (linearised at the
iterate of step W - 1) and shifted (at that iterate moved one stage, MPCB_WARM_SHIFT).

Everything here is the dense reference alone (tests/dense_qp.py): the rollout is (X_{j+1}, U_{j+1}) = (X_j, U_j) +
solve_equality(assemble(chain, cfg, X_j, U_j, xhat_j, yref_j)) from the guess.  The feedback states an engine under test is fed
are the rollout's, so its iterate stays within rounding of the rollout's; its Jacobians are nevertheless held to the dense ones
at ITS OWN previous prediction (check_step), the construction of chained_distances, so that rounding does not compound.

The conditions on a case (tests/test_sens_traj_cases.py asserts each from the reference alone):
  validity        on every step the equality-constrained minimiser clears every bound by 0.05 (dense_qp_cases.SEEDS): the fast
                  path accepts, sens_valid is 1
  discrimination  the dense Jacobians with the linearisation point rolled by one stage, and at the flat guess, are at least
                  DISCRIMINATION = 100 bounds away from the true ones: what the bound admits cannot be a stage mix-up
  conditioning    every bound <= 1e-6 of max |J| (sens_checks.bound, sensw_checks.bounds)
  rounding share  one ulp of the linearisation point, and one ulp of 1 in the task residuals, move the dense Jacobians by no more
                  than ULP_SHARE = a quarter of any bound (ulp_floor): the bounds are a few ulp of a row, and a case where the
                  reference's own unseen rounding fills them would test luck
The bound is the project's: 10 x max(the reference's own noise, eps x scale) with eps the step's committed oracle-vs-dense
distance TRAJ_ORACLE_VS_DENSE, measured on the CPU at the rollout's linearisation points.
"""
import contextlib

import numpy as np

import dense_qp as dq
import dense_qp_cases as dc
import reference_checks as rc
import sens_checks as sc
import sensw_checks as sw

W = 2                           # carried warm-up steps before the checked one
CARRIED, SHIFTED = "carried", "shifted"
MODES = (CARRIED, SHIFTED)
DISCRIMINATION = 100.0
CLEARANCE = 0.05                # of every bound, on every step (the rule of dense_qp_cases.SEEDS)
# 2, 7: a short single block; 20; 43; 130: more than one block of sens_pass<true> at every non-resident geometry; 26, 37 / 38,
# 42 / 43, 126, 140 / 141: both sides of the sweep switches of tests/test_emulation_sens.py SWITCH; 3, 12, 40: the ragged batch
HORIZONS = (2, 3, 7, 12, 20, 26, 37, 38, 40, 42, 43, 126, 130, 140, 141)

# |oracle - dense| over dX, dU of the QP at the dense rollout's linearisation point (reference_checks.oracle_qp solved by
# orc.qp_fast against solve_equality), measured on the CPU: the W warm-up steps, the checked step carried, the checked step shifted
TRAJ_ORACLE_VS_DENSE = {
    "N2-traj": (8.89e-16, 2.99e-16, 2.79e-16, 2.92e-16),
    "N3-traj": (6.67e-16, 1.74e-16, 3.34e-16, 3.01e-16),
    "N7-traj": (2.00e-15, 4.86e-16, 7.79e-16, 6.72e-16),
    "N12-traj": (9.33e-15, 1.09e-15, 6.81e-16, 7.36e-16),
    "N20-traj": (1.34e-14, 3.28e-15, 1.37e-15, 1.20e-15),
    "N26-traj": (1.76e-14, 5.61e-15, 1.28e-15, 1.68e-15),
    "N37-traj": (2.71e-14, 2.14e-14, 4.64e-15, 4.20e-15),
    "N38-traj": (2.49e-14, 3.96e-14, 9.05e-15, 4.11e-15),
    "N40-traj": (2.45e-14, 5.33e-14, 1.74e-14, 6.28e-15),
    "N42-traj": (2.23e-14, 6.07e-14, 4.67e-15, 5.39e-15),
    "N43-traj": (2.09e-14, 4.89e-14, 1.30e-14, 1.14e-14),
    "N126-traj": (4.93e-14, 3.58e-13, 2.10e-13, 1.15e-13),
    "N130-traj": (7.49e-14, 3.12e-13, 5.06e-14, 2.86e-14),
    "N140-traj": (1.06e-13, 2.02e-13, 1.54e-13, 1.26e-13),
    "N141-traj": (1.22e-13, 1.46e-13, 1.34e-13, 9.06e-14),
}


# the xhat draw of a horizon: the first of 9000 + N, + 1000, ... at which the reference alone meets every condition above (chosen on
# the CPU; every horizon but N = 3 keeps the first)
SEEDS = {**{N: 9000 + N for N in HORIZONS}, 3: 12003}


def cid(N):
    return "N%d-traj" % N


_CASES = {}


def case(N):
    """The default configuration with the bounds there, far from the solution (dense_qp_cases.INSIDE), at horizon N."""
    if N not in _CASES:
        assert N in HORIZONS
        _CASES[N] = dc._case(cid(N), dc._base(N, **dc.INSIDE), False, SEEDS[N])
    return _CASES[N]


def reference(cfg, N, j):
    """The task reference of step j, [N, 5]: reference_checks.ramp_reference k0 = j stages in, plus a sinusoid and a quadratic in
    px and a sinusoid in vy -- neither constant nor linear in the stage, and bounded however long the horizon.  Every target also
    stands well off what the arm can reach within the horizon (the surface distance 0.1, the alignment about 0.6 where the arm
    holds 1, the roll 0.2, px 0.3 and vy 0.1 off), so that no linearised task residual rho = r + G dx of the QP's solution is
    small: rho multiplies every addend of its row of du0_dw, and r = g - yref carries one ulp of 1 of rounding in any
    implementation, the dense one included, which neither the reference's d_ref nor the oracle-vs-dense distance sees.  With the
    packed alignment target 1 the residual g2 - 1 is a difference of two numbers near 1 and the w_task[1] row rests on that
    rounding alone (ulp_floor; tests/test_sens_traj_cases.py holds every case to a quarter of every bound)."""
    y = rc.ramp_reference(cfg, N, k0=j, px0=0.30, dpx=0.0004)
    k = np.arange(N) + j
    y[:, 0] += 0.1 + 0.01 * np.sin(0.3 * k + 1.0)
    y[:, 1] = 0.6 + 0.01 * np.cos(0.25 * k)
    y[:, 2] += 0.2 + 0.02 * np.sin(0.17 * k + 2.0)
    y[:, 3] += 0.02 * np.sin(0.21 * k) + 2e-6 * k * k
    y[:, 4] += 0.1 + 0.02 * np.cos(0.37 * k)
    return y


def shift_iterate(cfg, X, U):
    """MPCB_WARM_SHIFT restated with dense_qp.lti: u_k <- u_{k+1} with the last input held, x_k <- x_{k+1},
    x_N <- Ad x_N + Bd u_{N-1} (tests/test_sens_traj_cases.py: equal to warm_checks.shift_iterate)."""
    N = U.shape[0]
    A, B = dq.lti(cfg["wcv"], cfg["dt"])
    Xs, Us = X.copy(), U.copy()
    Xs[:N] = X[1:N + 1]
    Us[:N - 1] = U[1:N]
    Xs[N] = A @ X[N] + B @ U[N - 1]
    return Xs, Us


def roll_iterate(X, U):
    """The linearisation point a pass that reads stage k + 1 for stage k would see: X[k] <- X[k+1], U[k] <- U[k+1], last repeated."""
    return np.vstack([X[1:], X[-1:]]), np.vstack([U[1:], U[-1:]])


def point(c, mode, X, U):
    return (X, U) if mode == CARRIED else shift_iterate(c["cfg"], X, U)


# ------------------------------------------------------------------------------------------------- the stage evaluations, once
_STAGES = {}
_plain_stage_residual = dq.stage_residual


def _memo_stage_residual(chain, cfg, x, u, yref_k=None):
    """dense_qp.stage_residual, bit for bit, with the complex-step evaluation of a stage kept: the task outputs and the Jacobian
    do not depend on the weights or the reference, and the weight Jacobian assembles every stage fifteen times."""
    x, u = np.asarray(x, float), np.asarray(u, float)
    key = (id(chain), float(cfg["dt"]), np.asarray(cfg["wcv"], float).tobytes(), np.asarray(cfg["coeffs"], float).tobytes(),
           np.asarray(cfg["t_ee"], float).tobytes(), x.tobytes(), u.tobytes())
    if key not in _STAGES:
        _STAGES[key] = _plain_stage_residual(chain, cfg, x, u, np.zeros(5))          # g - 0 is g
    r0, Jr = _STAGES[key]
    r = r0.copy()
    r[:5] = r0[:5] - (dq.packed_reference(cfg) if yref_k is None else np.asarray(yref_k, float))
    return r, Jr


@contextlib.contextmanager
def stages_once():
    dq.stage_residual = _memo_stage_residual
    try:
        yield
    finally:
        dq.stage_residual = _plain_stage_residual
        if len(_STAGES) > 20000:
            _STAGES.clear()


# ------------------------------------------------------------------------------------------------------------ the dense rollout
_ROLLOUTS = {}


def rollout(N):
    """The dense rollout of the case, computed once per session and left unchanged: dict(xhat [W+1, 12], yref [W+1, N, 5],
    X, U: the W + 1 iterates (X[0], U[0] the guess), sol: solve_equality of the W warm-up steps)."""
    if N not in _ROLLOUTS:
        c = case(N)
        cfg, chain = c["cfg"], dc.chain_of(c)
        Ap, Bp = dq.lti(0.8 * np.asarray(cfg["wcv"]), cfg["dt"])
        rng = np.random.default_rng(77)
        X, U = dc.guess(c)
        x = c["xhat"].copy()
        out = dict(xhat=[], yref=[], X=[X], U=[U], sol=[])
        with stages_once():
            for j in range(W + 1):
                y = reference(cfg, N, j)
                out["xhat"].append(x)
                out["yref"].append(y)
                if j == W:
                    break
                sol = dq.solve_equality(dq.assemble(chain, cfg, X, U, x, y))
                X, U = X + sol["dX"], U + sol["dU"]
                out["sol"].append(sol)
                out["X"].append(X)
                out["U"].append(U)
                x = Ap @ x + Bp @ U[0] + rng.uniform(-1e-3, 1e-3, 12)
        _ROLLOUTS[N] = {k: (v if k == "sol" else np.stack(v)) for k, v in out.items()}
    return _ROLLOUTS[N]


def steps_of(N):
    """Every QP of the case: (label, X, U, xhat, yref) of the W warm-up steps and of the checked step in both modes, at the dense
    rollout's linearisation points -- the order of a TRAJ_ORACLE_VS_DENSE entry."""
    r, c = rollout(N), case(N)
    out = [("step%d" % j, r["X"][j], r["U"][j], r["xhat"][j], r["yref"][j]) for j in range(W)]
    for mode in MODES:
        X, U = point(c, mode, r["X"][W], r["U"][W])
        out.append((mode, X, U, r["xhat"][W], r["yref"][W]))
    return out


def clearance(qp, sol):
    """The least distance of the equality-constrained minimiser to a bound of the QP."""
    idx, lo, hi = qp.bounded()
    return float(np.minimum(sol["w"][idx] - lo, hi - sol["w"][idx]).min())


def eps(N, label):
    return TRAJ_ORACLE_VS_DENSE[cid(N)][[s[0] for s in steps_of(N)].index(label)]


def tolerance(N, label):
    """The bound on |engine - dense| of a step's QP solution: 10 x its committed distance, floor 1e-12 (dense_qp_cases.tolerance)."""
    return max(10.0 * eps(N, label), 1e-12)


def oracle_distance(orc, N, label):
    """|oracle - dense| of one step: the oracle's own assembly solved by orc.qp_fast against solve_equality of the dense QP."""
    c = case(N)
    _, X, U, xhat, y = [s for s in steps_of(N) if s[0] == label][0]
    rb = orc.make_robot(dc.chain_of(c), c["cfg"]["t_ee"])
    q = orc.qp_fast(*rc.oracle_qp(orc, rb, c["cfg"], X, U, xhat, y))
    assert q["accepted"], (N, label)
    with stages_once():
        sol = dq.solve_equality(dq.assemble(dc.chain_of(c), c["cfg"], X, U, xhat, y))
    return float(max(np.abs(q["w"][:, 6:] - sol["dX"]).max(), np.abs(q["w"][:N, :6] - sol["dU"]).max()))


# ------------------------------------------------------------------------------------------------------------ the Jacobians
def jacobians(c, X, U, xhat, y):
    """(sens_checks.dense_jacobians, sensw_checks.dense_weight_jacobian) of the QP at (X, U)."""
    with stages_once():
        return (sc.dense_jacobians(dc.chain_of(c), c["cfg"], X, U, xhat, y),
                sw.dense_weight_jacobian(dc.chain_of(c), c["cfg"], X, U, xhat, y))


_REFS = {}


def dense_reference(N, mode, which="true"):
    """The dense Jacobians of the checked step at the dense rollout's own point (`true`), at that point rolled by one stage
    (`rolled`) and at the flat guess (`flat`), the feedback state and the reference the same: once per session, unchanged."""
    key = (N, mode, which)
    if key not in _REFS:
        c, r = case(N), rollout(N)
        X, U = point(c, mode, r["X"][W], r["U"][W])
        if which == "rolled":
            X, U = roll_iterate(X, U)
        elif which == "flat":
            X, U = dc.guess(c)
        _REFS[key] = jacobians(c, X, U, r["xhat"][W], r["yref"][W])
    return _REFS[key]


def sens_blocks(N, pool, sweep, sensw=True):
    """The blocks the stage loop of Engine::sens_pass (csrc/mpc_core.h) walks at horizon N with a chunk pool of `pool` doubles, in
    a geometry whose gains are not resident (the block size of a resident one comes from the resident map's scratch): per stage
    [GQ | GV] 36, a row of dy 30, K_k 72 and, with du0_dw, the 36 staged operands, beside the two M buffers and the partial sums."""
    if sweep == "resident":
        return None
    per = 36 + 30 + 72 + (36 if sensw else 0)
    ch = max(1, min((pool - 2 * 72 - (3 * 36 if sensw else 0)) // per, N))
    return -(-(N - 1) // ch)


ULP_SHARE = 0.25


def ulp_floor(N, mode, residual=False):
    """How far one ulp moves the dense Jacobians, in bounds: (of du0_dx | du0_dyref, [7] of the rows of du0_dw).  Every entry of the
    linearisation point (X, U) nudged to the next double up, and down: every implementation reads the iterate in double, so this
    much is nobody's error, and a case whose bound it fills tests rounding luck.  `residual`: instead, every task residual moved by
    one ulp of 1, 2^-52, all one way and alternating from stage to stage -- the task outputs are sums of numbers of order 1
    (positions in metres, direction cosines), so g - yref carries that much rounding in any implementation, the dense one
    included, and neither d_ref nor the oracle-vs-dense distance sees it."""
    c, r = case(N), rollout(N)
    X, U = point(c, mode, r["X"][W], r["U"][W])
    y = r["yref"][W]
    ref, refw = dense_reference(N, mode)
    b, bw = sc.bound(ref, eps(N, mode)), sw.bounds(refw, eps(N, mode))
    u = 2.0 ** -52
    alt = np.where(np.arange(N) % 2 == 0, u, -u)[:, None]
    moves = ((X, U, y + u), (X, U, y + alt)) if residual else \
        ((np.nextafter(X, np.inf), np.nextafter(U, np.inf), y), (np.nextafter(X, -np.inf), np.nextafter(U, -np.inf), y))
    f, fw = 0.0, np.zeros(sw.NWEIGHT)
    for Xp, Up, yp in moves:
        o, ow = jacobians(c, Xp, Up, r["xhat"][W], yp)
        f = max(f, sc.distance(ref, o["Jx"], o["Jy"]) / b)
        fw = np.maximum(fw, np.abs(ow["J"] - refw["J"]).max(axis=1) / bw)
    return f, fw


def live_rows(N):
    """The rows of du0_dw that are not zero by structure (sensw_checks: with one stage the five task rows are)."""
    return slice(0, 2) if N == 1 else slice(0, sw.NWEIGHT)


def check_step(N, mode, prev, out, i, tag, record=None):
    """Simulation i of the checked step's outputs `out` against the dense Jacobians at the engine's own previous prediction
    `prev` = (x_pred [N+1, 12], u_pred [N, 6]) of step W - 1, shifted here for the shifted mode, with the step's feedback state and
    reference: the assertions of the issue.  Prints every figure before it asserts; returns (distance, bound) of
    (du0_dx | du0_dyref) and the per-row ones of du0_dw."""
    c, r = case(N), rollout(N)
    X, U = point(c, mode, np.asarray(prev[0])[:N + 1], np.asarray(prev[1])[:N])
    ref, refw = jacobians(c, X, U, r["xhat"][W], r["yref"][W])
    e = eps(N, mode)
    b, bw = sc.bound(ref, e), sw.bounds(refw, e)
    dx, dy, dwj = out["du0_dx"][i], out["du0_dyref"][i], out["du0_dw"][i] if "du0_dw" in out else None
    assert out["status"][i] == 0 and out["qp_iter"][i] == 1 and out["sens_valid"][i] == 1, (tag, N, mode, out["qp_iter"][i])
    d = sc.distance(ref, dx, dy, N)
    du = float(np.abs(out["u0"][i] - ref["u0"]).max())
    print(f"\n[sens-traj] {tag} {cid(N)} {mode}: |J - J_dense| = {d:.2e} (bound {b:.1e}, d_ref {ref['d_ref']:.1e}, max |J| "
          f"{ref['scale']:.2e}), |u0 - dense| = {du:.2e} (bound {tolerance(N, mode):.1e})")
    if record is not None:
        record[(tag, cid(N), mode, -1)] = (d, b, ref["d_ref"], 0.0, ref["scale"])
    dw = None
    if dwj is not None:
        dw = sw.distances(refw, dwj)
        for p in range(sw.NWEIGHT):
            print(f"[sens-traj] {tag} {cid(N)} {mode} row {p}: |dw - J| = {dw[p]:.2e} (bound {bw[p]:.1e}, d_ref "
                  f"{refw['d_ref'][p]:.1e}, A {refw['A'][p]:.2e}, max |J| {refw['scale'][p]:.2e})")
            if record is not None:
                record[(tag, cid(N), mode, p)] = (dw[p], bw[p], refw["d_ref"][p], refw["A"][p], refw["scale"][p])
    assert np.isfinite(dx).all() and np.isfinite(dy).all(), (tag, N, mode)
    assert d <= b, (tag, N, mode, d, b)
    assert du <= tolerance(N, mode), (tag, N, mode, du)
    assert (dy[0] == 0.0).all(), (tag, N, mode)                  # x_0 is pinned to xhat: exactly zero, not small
    assert (dy[N:] == 0.0).all(), (tag, N, mode)                 # rows past the simulation's own horizon (ragged batches)
    if dwj is not None:
        assert np.isfinite(dwj).all() and (dw <= bw).all(), (tag, N, mode, dw, bw)
    return (d, b), (dw, bw)


SANITY = 1e-6       # |engine iterate - dense rollout|: rounding that compounds over W steps, printed; a loose guard, not a bound


def check_warmup(N, j, prev, out, i, tag):
    """Warm-up step j of simulation i: the engine's step from ITS previous iterate `prev` (the guess for j = 0) is the solution of
    the dense QP there within the step's tolerance, and its iterate stays near the dense rollout's."""
    c, r = case(N), rollout(N)
    assert out["status"][i] == 0 and out["qp_iter"][i] == 1, (tag, N, j, out["qp_iter"][i])
    xp, up = out["x_pred"][i][:N + 1], out["u_pred"][i][:N]
    with stages_once():
        sol = dq.solve_equality(dq.assemble(dc.chain_of(c), c["cfg"], prev[0], prev[1], r["xhat"][j], r["yref"][j]))
    d = float(max(np.abs(xp - prev[0] - sol["dX"]).max(), np.abs(up - prev[1] - sol["dU"]).max()))
    off = float(max(np.abs(xp - r["X"][j + 1]).max(), np.abs(up - r["U"][j + 1]).max()))
    print(f"\n[sens-traj] {tag} {cid(N)} step {j}: |step - dense| = {d:.2e} (bound {tolerance(N, 'step%d' % j):.1e}), "
          f"|iterate - dense rollout| = {off:.2e}")
    assert d <= tolerance(N, "step%d" % j), (tag, N, j, d)
    assert off <= SANITY, (tag, N, j, off)
    return xp.copy(), up.copy()


def dump(path, measured):
    with open(path, "w") as f:
        for (tag, c, mode, p), v in sorted(measured.items()):
            row = "J    " if p < 0 else "row %d" % p
            f.write("%-30s %-10s %-8s %s  distance %.2e  bound %.1e  d_ref %.1e  A %.2e  max|J| %.2e\n" % ((tag, c, mode, row) + tuple(v)))
