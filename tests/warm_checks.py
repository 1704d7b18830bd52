"""The shift of a warm start (MPCB_WARM_SHIFT, include/mpcbatch.h) restated in numpy, shared by the emulation and the device tests."""
import numpy as np

import reference_checks as rc

CARRY, RESET, SHIFT = 0, 1, 2


def shift_iterate(orc, cfg, X, U):
    """(X [N+1,12], U [N,6]) moved one stage towards stage 0: u_k <- u_{k+1} with u_{N-1} held, x_k <- x_{k+1}, and
    x_N <- Ad x_N + Bd u_{N-1} from the old x_N and the held input."""
    N = U.shape[0]
    A, B = rc.lti_matrices(orc, cfg)
    Xs, Us = X.copy(), U.copy()
    Xs[:N] = X[1:N + 1]
    Us[:N - 1] = U[1:N]
    Xs[N] = A @ X[N] + B @ U[N - 1]
    return Xs, Us


def qp_step(orc, rb, chain, cfg, X, U, xhat, y, out=None):
    """The iterate after the exact Gauss-Newton QP step from (X, U): the oracle's fast path, or -- where that rejects the QP, or the
    engine's step `out` = (x_pred, u_pred, qp_iter) was an interior-point solve -- the active-set certificate of the independently
    assembled dense QP at the engine's result.  None when neither is available (fast path rejected and no engine result)."""
    if out is not None and out[2] != 1:
        return rc.gn_qp_step(orc, rb, cfg, X, U, xhat, y, backend="dense", chain=chain, candidate=(out[0], out[1]))
    return rc.gn_qp_step(orc, rb, cfg, X, U, xhat, y)
