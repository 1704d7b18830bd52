"""Independent checks of the controller step against a task reference, shared by the emulation and the device tests: the
Gauss-Newton QP step at a given iterate (from the oracle's primitives, or independently of the oracle through tests/dense_qp.py),
and a dense least-squares solve of the NLP."""
import numpy as np


def _weights(cfg):
    return np.concatenate([np.asarray(cfg["w_task"], float), np.full(6, 2.0 * cfg["w_u"]), np.full(6, cfg["w_qddot"])])


def g_ref(cfg):
    """The packed task reference [0, 1, 0, px_ref, vy_ref] of a resolved configuration."""
    return np.array([0.0, 1.0, 0.0, cfg["px_ref"], cfg["vy_ref"]])


def lti_matrices(orc, cfg):
    a12, a22, b1, b2 = orc.lti(cfg["wcv"], cfg["dt"])
    A = np.zeros((12, 12)); B = np.zeros((12, 6))
    A[:6, :6] = np.eye(6); A[:6, 6:] = np.diag(a12); A[6:, 6:] = np.diag(a22)
    B[:6] = np.diag(b1); B[6:] = np.diag(b2)
    return A, B


def stage_residual(orc, rb, p, cfg, x, u, yref_k):
    """orc.stage_residual with the task rows taken against the target yref_k instead of the packed g_ref."""
    r, Jr = orc.stage_residual(rb, p, x, u)
    r = r.copy()
    r[:5] += g_ref(cfg) - yref_k
    return r, Jr


def oracle_qp(orc, rb, cfg, X, U, xhat, yref):
    """The Gauss-Newton QP at the iterate (X [N+1,12], U [N,6]) under the reference yref [N,5], built from the oracle's
    primitives: (H, g, b, A, B, lb, ub, dx0) as orc.qp_fast / orc.qp_ipm take them."""
    p = orc.make_params(cfg)
    N, dt, lm = cfg["N"], cfg["dt"], float(cfg.get("levenberg_marquardt", 0.0))
    W = _weights(cfg)
    A, B = lti_matrices(orc, cfg)
    H = np.zeros((N + 1, 18, 18)); g = np.zeros((N + 1, 18)); b = np.zeros((N + 1, 12))
    lb = np.full((N + 1, 12), -1e30); ub = np.full((N + 1, 12), 1e30)
    for k in range(N):
        r, Jr = stage_residual(orc, rb, p, cfg, X[k], U[k], yref[k])
        H[k] = dt * Jr.T @ (W[:, None] * Jr) + dt * lm * np.eye(18)
        g[k] = dt * Jr.T @ (W * r)
        b[k] = A @ X[k] + B @ U[k] - X[k + 1]
        lb[k, :6] = np.asarray(cfg["umin"]) - U[k]; ub[k, :6] = np.asarray(cfg["umax"]) - U[k]
        if k >= 1:
            lb[k, 6:] = np.asarray(cfg["qmin"]) - X[k, :6]; ub[k, 6:] = np.asarray(cfg["qmax"]) - X[k, :6]
    H[N, 6:, 6:] += lm * np.eye(12)
    return H, g, b, A, B, lb, ub, xhat - X[0]


def gn_qp_step(orc, rb, cfg, X, U, xhat, yref, backend="oracle", chain=None, candidate=None):
    """The iterate after one full Gauss-Newton QP step from (X [N+1,12], U [N,6]) under the reference yref [N,5].

    backend "oracle": the QP from the oracle's primitives, solved by the bound-inactive fast path (orc.qp_fast); None when the
    fast path rejects the QP.
    backend "dense": the QP by the independent assembly of tests/dense_qp.py (`chain`: the kinematic chain), solved with the
    active set read off `candidate` = (x_pred, u_pred) -- the exact active-set certificate of dense_qp.certify, whatever the
    engine's QP solver did; the certificate's multipliers and slacks are asserted here, the caller compares the iterate."""
    if backend == "dense":
        import dense_qp as dq

        qp = dq.assemble(chain, cfg, X, U, xhat, yref)
        cert = dq.certify(qp, candidate[0] - X, candidate[1] - U)
        assert cert["min_multiplier"] >= 0 and cert["min_slack"] >= 0, cert
        return X + cert["dX"], U + cert["dU"]
    q = orc.qp_fast(*oracle_qp(orc, rb, cfg, X, U, xhat, yref))
    if not q["accepted"]:
        return None
    return X + q["w"][:, 6:], U + q["w"][:cfg["N"], :6]


def dense_nlp_solve(orc, rb, cfg, xhat, yref, u_init):
    """The NLP of one MPC step (states eliminated through x_{k+1} = Ad x_k + Bd u_k, x_0 = xhat, bounds ignored) by
    scipy.optimize.least_squares over the stacked sqrt(dt W) r_k; returns U [N, 6]."""
    from scipy.optimize import least_squares

    p = orc.make_params(cfg)
    N, dt = cfg["N"], cfg["dt"]
    sw = np.sqrt(dt * _weights(cfg))
    A, B = lti_matrices(orc, cfg)

    def fun(z):
        U = z.reshape(N, 6)
        x = np.asarray(xhat, float).copy()
        out = []
        for k in range(N):
            out.append(sw * stage_residual(orc, rb, p, cfg, x, U[k], yref[k])[0])
            x = A @ x + B @ U[k]
        return np.concatenate(out)

    sol = least_squares(fun, np.asarray(u_init, float).ravel(), xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=2000)
    return sol.x.reshape(N, 6)


def ramp_reference(cfg, N, k0=0, px0=0.36, dpx=0.002, vy0=0.03, dvy=0.001):
    """A per-stage ramp in px_ref and vy_ref (the other targets packed): row k = stage k of a step that starts k0 stages in."""
    y = np.tile(g_ref(cfg), (N, 1))
    k = np.arange(N) + k0
    y[:, 3] = px0 + dpx * k
    y[:, 4] = vy0 + dvy * np.sin(0.3 * k)
    return y
