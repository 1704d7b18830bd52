"""The reference of the sensitivity tests (mpcb_step_sens): the Jacobians of u0 of one Gauss-Newton QP by central differences of
the dense KKT solve of tests/dense_qp.py, shared by the emulation and the device tests.

u0 = U_0 + du_0 with du the minimiser of the bound-free QP that dense_qp.assemble builds at an iterate.  The feedback state enters
it through dx_0 = xhat - X_0 alone and the task reference through the gradient of its own stage, g_k = dt Jr' W r with the task
rows of r shifted by -yref_k: the perturbed QPs are formed by exactly those two lines of assemble (the stage Jacobian from
dense_qp.stage_residual), and all of them are solved with ONE pivoted sparse LU of the KKT matrix dense_qp._kkt assembles -- the
matrix solve_equality factorises -- as a block of right-hand sides; the base solution is checked against solve_equality itself.
The map is affine, so central differences at two step sizes agree up to rounding: their disagreement is the reference's own noise.
"""
import numpy as np
import scipy.sparse.linalg as spla

import dense_qp as dq

STEPS = (1e-3, 1e-2)
MARGIN = 10.0            # the project's margin of dense-QP comparisons (dense_qp_cases.tolerance)
CONDITION = 1e-6         # no asserted bound may exceed this fraction of max |J|: a wrong term is an O(1) relative error


def dense_jacobians(chain, cfg, X, U, xhat, yref=None):
    """dict(Jx [6, 12] = d u0 / d xhat, Jy [N, 5, 6] = (d u0 / d yref_k)', d_ref: max disagreement of the two step sizes,
    scale: max |J|, u0)."""
    X, U = np.asarray(X, float), np.asarray(U, float)
    N = U.shape[0]
    qp = dq.assemble(chain, cfg, X, U, xhat, yref)
    K, rhs, n = dq._kkt(qp, np.zeros(0, dtype=int), np.zeros(0))
    lu = spla.splu(K.tocsc())
    base = lu.solve(rhs)
    ref = dq.solve_equality(qp)
    assert np.abs(base[:n] - ref["w"]).max() <= 1e-9 * max(1.0, np.abs(ref["w"]).max())
    W, dt = dq.weights(cfg), float(cfg["dt"])
    # d rhs / d parameter: xhat_j moves dx0_j (row n + j); yref_k[c] moves r_c of stage k by -1, so -g_k by +dt Jr' W e_c
    cols = []
    for j in range(12):
        v = np.zeros_like(rhs)
        v[n + j] = 1.0
        cols.append(v)
    memo = {}
    for k in range(N):
        key = (X[k].tobytes(), U[k].tobytes())
        if key not in memo:
            memo[key] = dq.stage_residual(chain, cfg, X[k], U[k], None)[1]
        Jr = memo[key]
        for c in range(5):
            v = np.zeros_like(rhs)
            e = np.zeros(dq.NR)
            e[c] = 1.0
            v[dq.NW * k:dq.NW * k + dq.NW] = dt * Jr.T @ (W * e)
            if k == N:
                raise AssertionError
            cols.append(v)
    D = np.stack(cols, axis=1)
    J = []
    for h in STEPS:
        up = lu.solve(rhs[:, None] + h * D)[:6]
        dn = lu.solve(rhs[:, None] - h * D)[:6]
        J.append((up - dn) / (2.0 * h))
    d_ref = float(np.abs(J[0] - J[1]).max())
    Jm = J[0]
    Jx = Jm[:, :12].copy()
    Jy = Jm[:, 12:].reshape(6, N, 5).transpose(1, 2, 0).copy()
    return dict(Jx=Jx, Jy=Jy, d_ref=d_ref, scale=float(max(np.abs(Jx).max(), np.abs(Jy).max())), u0=U[0] + ref["dU"][0])


def bound(ref, eps_case):
    """10 x max(the reference's own noise, the case's committed solver-vs-dense distance relative to max |J|), which must stay
    below CONDITION x max |J|."""
    b = MARGIN * max(ref["d_ref"], eps_case * ref["scale"])
    assert b <= CONDITION * ref["scale"], (b, ref["scale"])
    return b


def distance(ref, du0_dx, du0_dyref, N=None):
    N = ref["Jy"].shape[0] if N is None else N
    return float(max(np.abs(du0_dx - ref["Jx"]).max(), np.abs(du0_dyref[:N] - ref["Jy"]).max()))
